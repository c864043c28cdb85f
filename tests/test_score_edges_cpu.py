"""The step-edge cluster (tests/edge_cases.py) does what it claims, judged by the oracle, integer arithmetic on the
built rows and engine.row_eval alone — otherwise the GPU tests of tests/test_score_edges_gpu.py could pass vacuously —
and the host program tests/native/fma_score_check.cpp (the fast-path formula and the weight-sum divisions against
int64 division)."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import edge_cases as ec_
from edge_cases import C, CAPS, J, N_ALIGNED, SLOTS, SLOT_NAMES, least, most
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import make_config

ROOT = pathlib.Path(__file__).resolve().parents[1]
FIT_NAME = ("cpu", "memory", ec_.BATCH_CPU, ec_.BATCH_MEM)
FIT_RES = (nat.RES_CPU, nat.RES_MEMORY, nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY)


def _rows(ec):
    cfg = ec_.config("shipped")
    return cfg, engine.build_node_rows(cfg, ec.view), engine.build_pod_rows(cfg, ec.view, np.arange(ec.n_pods))


def _operands(nrow, prow, s):
    """(cap, base, pr) of slot s from one built node row and one built pod row, as Python ints."""
    if s < 4:
        r = FIT_RES[s]
        base = nrow["nonzero_requested"][s] if s < 2 else nrow["requested"][r]
        return int(nrow["alloc"][r]), int(base), int(prow["fit_score_request"][r])
    return int(nrow["la_alloc"][s - 4]), int(nrow["la_used"][0][s - 4]), int(prow["la_estimate"][s - 4])


def _designated(i, s):
    """The adjacent pod pair of slot s that aligned node i is built for."""
    j = i % J
    return (4 * j + 2, 4 * j + 3) if s in (2, 3) else (4 * j, 4 * j + 1)


def _single_resource_config(s, most_allocated):
    if s < 4:
        return make_config(fit_resources={FIT_NAME[s]: 1}, fit_strategy="MostAllocated" if most_allocated else "LeastAllocated")
    return make_config(resource_weights={("cpu", "memory")[s - 4]: 1})


@pytest.mark.parametrize("most_allocated", [False, True], ids=["least", "most"])
def test_every_quotient_sits_on_a_step(most_allocated):
    """Per slot and cap class: every quotient k reachable with a non-negative base occurs as the oracle's score of a
    pair whose neighbour (request + 1) scores k − 1 (MostAllocated: the neighbour scores k, the pair k − 1).  Reachable:
    LeastAllocated k ≤ 99 (100 needs a request of 0) with cap − ceil(k·cap/100) ≥ the class's largest request (each (class, k)
    meets one of the class's two pod pairs, so only what both reach is demanded), for the caps from 12,800 up that is
    every k in 1..99 (MostAllocated 1..100); a cap below 100 has fewer quotients than 101 and steps larger than one,
    there every adjacent request pair (req, req + 1), the class's largest request ≤ req < cap, must occur."""
    ec = ec_.edge_cluster(most_allocated)
    cfg, nrows, prows = _rows(ec)
    for s in range(SLOTS):
        is_most = most_allocated and s < 4
        if most_allocated and s >= 4:
            continue   # LoadAware has one strategy: covered by the LeastAllocated cluster
        f = most if is_most else least
        sc = _single_resource_config(s, is_most)
        plane = ec_.oracle.eval_matrix(sc, ec.view, ec.pair_pods, ec.view.now_ns)[1 if s < 4 else 2]
        seen = [set() for _ in range(C)]
        pr_max = [0] * C
        for i in range(N_ALIGNED):
            p0, p1 = _designated(i, s)
            a, base, pr0 = _operands(nrows[i], prows[p0], s)
            a1, base1, pr1 = _operands(nrows[i], prows[p1], s)
            assert (a, base, pr0 + 1) == (a1, base1, pr1) and a == CAPS[i % C] and base >= 0, (SLOT_NAMES[s], i)
            q0, q1 = f(base + pr0, a), f(base + pr1, a)
            # the integers from the built rows are the oracle's scores of these pairs
            assert (q0, q1) == (int(plane[p0, i]), int(plane[p1, i])), (SLOT_NAMES[s], i, a, base, pr0)
            seen[i % C].add((q0, q1, base + pr0))
            pr_max[i % C] = max(pr_max[i % C], pr0)
        for c, a in enumerate(CAPS):
            got = {(q0, q1) for q0, q1, _ in seen[c]}
            if a >= 100:
                if is_most:
                    want = {k for k in range(1, 101) if ec_.ceil_div(k * a, 100) - 1 >= pr_max[c]}
                    full = set(range(1, 101))
                    missing = {k for k in want if (k - 1, k) not in got}
                else:
                    want = {k for k in range(1, 100) if a - ec_.ceil_div(k * a, 100) >= pr_max[c]}
                    full = set(range(1, 100))
                    missing = {k for k in want if (k, k - 1) not in got}
                assert not missing, (SLOT_NAMES[s], a, sorted(missing))
                assert a < 12_800 or want == full, (SLOT_NAMES[s], a)
                assert len(want) >= 1
            else:
                reqs = {r for _, _, r in seen[c]}
                assert reqs >= set(range(pr_max[c], a)), (SLOT_NAMES[s], a, sorted(reqs))
                assert got >= {(f(r, a), f(r + 1, a)) for r in range(pr_max[c], a)}


def test_requests_span_the_admitted_range():
    """The effective requests run from 1 to beyond 2^34, and the largest request the engine admits is in the batch."""
    ec = ec_.edge_cluster()
    _, _, prows = _rows(ec)
    pr = prows["fit_score_request"][ec.pair_pods]
    assert pr[pr > 0].min() == 1 and pr.max() > 1 << 34 and prows["la_estimate"][ec.pair_pods].max() > 1 << 34
    assert prows["request"][ec.filter_pods[2]][nat.RES_MEMORY] == ec_.VAL_LIMIT - 1


def test_row_eval_equals_oracle_on_the_aligned_pairs():
    """The host's per-pair evaluation (kg_row_eval: the exact int64 path) on every aligned (node, designated pod)
    pair, and on the filter, big-base and negative-base nodes, equals the oracle."""
    ref = ec_.reference("shipped", True)
    ec = ref.ec
    cfg, nrows, prows = _rows(ec)
    pairs = [(i, p) for i in range(N_ALIGNED) for s in (0, 2) for p in _designated(i, s)]
    pairs += [(int(n), int(p)) for n in ec.filter_nodes for p in ec.filter_pods]
    pairs += [(int(n), int(p)) for n in ec.big_nodes for p in (0, 4 * C, 4 * C + 2)]
    pairs += [(int(n), int(p)) for n in ec.neg_nodes for p in ec.neg_pods if ref.mask[p, n]]
    assert sum(ref.mask[p, n] for n in ec.neg_nodes for p in ec.neg_pods) >= len(ec.neg_nodes)
    for i, p in pairs:
        got = engine.row_eval(cfg, nrows[i:i + 1], prows[p:p + 1], ec.view.now_ns)
        assert got[:3] == (bool(ref.mask[p, i]), int(ref.fit[p, i]), int(ref.la[p, i])), (i, p)


def test_filter_operands_are_exact():
    """free == request is feasible and free == request − 1 is not, at 2^33 + 5 and at KG_VAL_LIMIT − 1."""
    ref = ec_.reference("shipped")
    fn, fp = ref.ec.filter_nodes, ref.ec.filter_pods
    for pod, nodes in ((fp[0], fn[:2]), (fp[1], fn[:2]), (fp[2], fn[2:])):
        assert ref.mask[pod, nodes[0]] and not ref.mask[pod, nodes[1]]


def _two_best(total_row):
    order = np.argsort(-total_row, kind="stable")
    return int(order[0]), int(order[1])


def test_top1_is_decided_by_one_score_point():
    """At least one pod's best node beats the runner-up by exactly one point of the total: an off-by-one score there
    changes the placement."""
    for name in ("shipped", "most_w", "slot_fit600"):
        ref = ec_.reference(name)
        n = 0
        for p in range(ref.ec.n_pods):
            b, r = _two_best(ref.total[p])
            n += ref.total[p, r] >= 0 and ref.total[p, b] - ref.total[p, r] == 1
        assert n >= 1, name


@pytest.mark.parametrize("name", ec_.BIG_CONFIGS)
def test_big_weights_reach_key_bit_31(name):
    """Plugin weights in the tens of thousands: some pod's best total is ≥ 2^21, so its per-tile key
    ((total + 1) << 10 | …) has bit 31 set, the limit key fits 32 bits, and some pod's two best nodes lie in
    different 1,024-node tiles (the tile merge decides)."""
    ref = ec_.reference(name)
    assert ref.best_total.max() >= 1 << 21
    assert ((int(ref.best_total.max()) + 1) << 10 | 1023) < 1 << 32
    assert ((100 * 40_000 + 1) << 10 | 1023) < 1 << 32
    split = 0
    for p in range(ref.ec.n_pods):
        b, r = _two_best(ref.total[p])
        split += ref.total[p, r] >= 0 and b // nat.TILE != r // nat.TILE
    assert split >= 1


def test_negative_variant_holds_the_recorded_tuples():
    """The three recorded tuples are pairs of the negative cluster (their exact quotients 83, 76, 45 on the Fit and
    LoadAware slots), and the sweep nodes put the NEG_X pair on steps with bases in (−2^49, 0)."""
    ec = ec_.edge_cluster(False, True)
    cfg, nrows, prows = _rows(ec)
    for t, ((a, base, pr), want) in enumerate(zip(ec_.NEG_TUPLES, (83, 76, 45))):
        node = ec.neg_nodes[t]
        fit_pod, la_pod = ec.neg_pods[2 * t: 2 * t + 2]
        for s, pod in ((0, fit_pod), (1, fit_pod), (4, la_pod), (5, la_pod)):
            assert _operands(nrows[node], prows[pod], s) == (a, base, pr)
        assert least(base + pr, a) == want
    steps = 0
    for node in ec.neg_nodes[len(ec_.NEG_TUPLES):]:
        for s in (0, 1, 4, 5):
            a, base, pr = _operands(nrows[node], prows[ec.neg_sweep_pods[0]], s)
            assert -(1 << 49) < base < 0 and 0 <= base + pr <= a
            steps += least(base + pr, a) == least(base + pr + 1, a) + 1
    assert steps >= 200


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fma_score_matches_int64_division(tmp_path):
    """tests/native/fma_score_check.cpp: R and F from kg_finalize_fit_r / kg_finalize_la_r, fma, the clamps, and the
    three weight-sum divisions (every W ≤ 600, every s ≤ 100·W) against int64 division."""
    exe = tmp_path / "fma_score_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'koordinator_amd' / 'csrc'}", str(ROOT / "tests" / "native" / "fma_score_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " bad 0 " in out.stdout
