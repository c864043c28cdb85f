"""Output containment and history independence of matrix mode (kg_eval, kg_cycle_one with planes).

Every other matrix test compares the cells that should have been written; these assert that nothing else was, and that
the result does not depend on what the buffers held.  Each case (tests/matrix_cases.py: one family per writer of the
planes, at the widths, shards and pod counts where the addressing changes) runs into guarded device buffers
(tests/guarded_out.py: [guard | payload | guard] per plane) twice, prefilled with 0x00 and with 0xFF (an illegal
score, and every stale mask bit set), and asserts:

  * guards: every byte outside the payloads, and every byte of a plane that was not requested, still holds the prefill;
  * parity: in-range cells and top1 (ties to the lowest node) equal the oracle's;
  * mask pad bits: columns [width, 64·words) of the last word are 0;
  * prefill independence: the two runs agree byte for byte on the in-range cells and the mask's pad bits;
  * host path: one Engine.eval per family variant (the shard [1024, 2100)) equals the device run over the same cells.

The score, NUMA and Reservation pad columns [width, 64·words) are unspecified and not compared.  An empty shard
returns KG_OK, writes top1 = 0 (with reservation slots loaded: the best reservation node, which every shard
reports) and touches nothing else.

The small shapes keep k_eval_numa2's grid form at z = 8 and never reach its z < 8 splits (taken when
blocks · z ≥ 2 · resident workgroups); those stay with the full-size tests (tests/test_fullsize_gpu.py).
"""
import numpy as np
import pytest

import matrix_cases as mc
from guarded_out import PLANES, GuardedOutputs, specified_cells
from koordinator_amd import engine

pytestmark = pytest.mark.gpu

PREFILLS = (0x00, 0xFF)


@pytest.fixture(scope="module")
def dev():
    import torch   # torch's HIP context first: it does not initialise beside a live engine
    d = torch.device("cuda", 0)
    torch.zeros(1, device=d)
    torch.cuda.synchronize(d)
    return d


def _requested(case):
    want = mc.planes_of(case)
    return tuple(k for k in PLANES if want[k])


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=what + ": " + k)


def _guarded_runs(case, eng, dev, request):
    """The case on `eng` once per prefill: guards, parity and pad bits per run, then the two runs against each other.
    Returns the specified cells."""
    now = mc.inputs(case).now_ns
    runs = []
    for prefill in PREFILLS:
        got = GuardedOutputs(case.n_pods, case.width, prefill, dev).eval(eng, now, request)
        mc.check_against_reference(case, got)
        runs.append(specified_cells(got, case.width))
    _same(runs[0], runs[1], f"{case.id}: prefill 0x00 against 0xFF")
    return runs[0]


def _run(case, dev):
    request = _requested(case)
    with mc.make_engine(case) as eng:
        cells = _guarded_runs(case, eng, dev, request)
        if case.width == 0:
            if case.family != "rsv":
                assert not cells["top1"].any()
        if (case.begin, case.end) == (1024, 2100):   # the host path (outputs staged back to back in scratch)
            want = mc.planes_of(case)
            res = eng.eval(mc.inputs(case).now_ns, numa_scores=want["numa"], rsv_scores=want["rsv"])
            host = {"mask": res["mask"], "scores": res["scores"], "top1": res["top1"]}
            if want["numa"]:
                host["numa"] = res["numa_scores"]
            if want["rsv"]:
                host["rsv"] = res["rsv_scores"]
            _same(specified_cells(host, case.width), cells, f"{case.id}: host path against device path")


def _params(family):
    return pytest.mark.parametrize("case", mc.FAMILIES[family], ids=lambda c: c.id)


@_params("class")
def test_guard_class_path(case, dev):
    """k_eval3, plain and LoadAware-uniform work items, the 2- and 4-resource kinds; every listed width and shard."""
    _run(case, dev)


@_params("dup")
def test_guard_duplicate_rows(case, dev):
    """k_eval3_dup: repeated rows in a shuffled queue, singles on the plain path."""
    _run(case, dev)


@_params("slow")
def test_guard_slow_nodes(case, dev):
    """k_fix_slow: slow nodes in the first and last column of the range and in columns 63 and 64; one just outside
    each end of a shard, which must leave no trace."""
    _run(case, dev)


@_params("la_extra")
def test_guard_loadaware_extra_weights(case, dev):
    """k_eval2's LAX form with its KGD_XSLOW fix-up, and k_eval_exact."""
    _run(case, dev)


@_params("numa")
def test_guard_numa(case, dev):
    """k_eval_numa2: grid / queued × combined / fused, plain and equivalent-pod batches (eval_eq, k_eq_rows<8> /
    <16>)."""
    _run(case, dev)


@_params("bind")
def test_guard_numa_cpuset_batch(case, dev):
    """k_numa_bind_fix: cpuset pods on NUMA-policy nodes."""
    _run(case, dev)


@_params("rsv")
def test_guard_reservation_quota(case, dev):
    """k_pod_gate, k_rsv_eval, k_rsv_reduce, k_quota_apply; the Reservation plane is guarded too."""
    _run(case, dev)


@pytest.mark.parametrize("case", mc.SUBSET_CASES, ids=lambda c: f"{c.family}-{c.id}")
def test_guard_output_subsets(case, dev):
    """Mask only, scores only, top1 only, NUMA plane only, top1 + NUMA plane: each produced plane equals the same
    plane of the all-outputs run, each unrequested buffer is untouched end to end (GuardedOutputs.collect)."""
    with mc.make_engine(case) as eng:
        everything = _guarded_runs(case, eng, dev, ("mask", "scores", "top1", "numa"))
        for subset in mc.SUBSETS:
            request = tuple(subset.split("+"))
            cells = _guarded_runs(case, eng, dev, request)
            assert set(cells) == set(request)
            _same(cells, {k: everything[k] for k in request}, f"{case.id}: subset {subset}")


@pytest.mark.parametrize("n_nodes,begin,end", mc.CYCLE_SHAPES, ids=lambda v: str(v))
def test_guard_cycle_one_device_planes(n_nodes, begin, end, dev):
    """kg_cycle_one with device planes: guards intact, planes and key equal kg_eval's for the same pod, whatever the
    buffers held."""
    import cycle_cases as cc
    case = mc.Case("class", "shipped", n_nodes, begin, end, 8)
    inp = mc.inputs(case)
    cfg = cc.config("shipped")
    rows = engine.build_pod_rows(cfg, inp.view, inp.idx)
    request = ("mask", "scores", "top1", "numa")
    with mc.make_engine(case) as eng:
        batch = _guarded_runs(case, eng, dev, request)
        for p in range(case.n_pods):
            runs = []
            for prefill in PREFILLS:
                out, got = GuardedOutputs(1, case.width, prefill, dev).cycle_one(eng, rows[p:p + 1], inp.now_ns, request)
                assert int(out.key) == int(batch["top1"][p]) and int(got["top1"][0]) == int(out.key)
                runs.append(specified_cells(got, case.width))
                _same(runs[-1], {k: batch[k][p:p + 1] for k in request}, f"{case.id}: pod {p} against kg_eval")
            _same(runs[0], runs[1], f"{case.id}: pod {p}, prefill 0x00 against 0xFF")
