"""Score exactness on the GPU at the fp64 bounds, the weight limits and key bit 31: the step-edge cluster of
tests/edge_cases.py (every aligned node on a step of a score quotient, caps up to 2^41 − 1, requests up to about 2^34
and KG_VAL_LIMIT − 1) through every implementation of the pair formula, against the oracle by exact equality.
tests/test_score_edges_cpu.py asserts that the cluster has the properties these tests rely on."""
import numpy as np
import pytest

import edge_cases as ec_
from koordinator_amd import _native as nat
from koordinator_amd import engine

pytestmark = pytest.mark.gpu


def _engine(ref, node_rows=None, pod_rows=None):
    eng = engine.Engine(ref.cfg)
    try:
        eng.load_snapshot(engine.build_node_rows(ref.cfg, ref.ec.view) if node_rows is None else node_rows)
        eng.set_pods(engine.build_pod_rows(ref.cfg, ref.ec.view, ref.idx) if pod_rows is None else pod_rows)
    except Exception:
        eng.close()
        raise
    return eng


def _key(total, node):
    return 0 if node < 0 else ((int(total) + 1) << 32) | (0xFFFFFFFF - int(node))


@pytest.mark.parametrize("name", ["shipped", "most4", "w3_5", "big_20000", "big_39999"])
def test_class_path_distinct_rows(name):
    """k_eval3 (the class path: every pod's Fit weight sum and the LoadAware weight sum are powers of two, no pod is
    restricted; the pair pods' rows are distinct apart from the small-cap classes' shared ones, which take
    k_eval3_dup).  shipped: the packed FULL && W1 form; most4: MostAllocated (the min(q, 100) clamp); w3_5: plugin
    weights 3 / 5, the W1 = false form; big_*: plugin weights 20000 / 20000 and 39999 / 1, per-tile keys beyond
    bit 31 (total + 1 ≥ 2^21)."""
    ref = ec_.reference(name)
    with _engine(ref) as eng:
        assert eng.spill_count() == 0 and eng.restricted_count() == 0
        ec_.check_eval(ref, eng.eval(ref.ec.view.now_ns))


@pytest.mark.parametrize("name", ["shipped", "w3_5", "big_39999"])
def test_class_path_duplicate_rows(name):
    """k_eval3_dup: designated pods repeated 2, 9 and 70 times in a shuffled queue (each row evaluated once, written
    to every pod of it), planes and top-1 against the oracle and a top-1-only pass equal to the full one."""
    rng = np.random.default_rng(17)
    picks = [4 * j + d for j in (0, ec_.C, ec_.C + 2, ec_.C + 13, 4, 12) for d in (0, 1, 2, 3)]
    order = np.concatenate([np.repeat(picks[0:8], 2), np.repeat(picks[8:16], 9), np.repeat(picks[16:18], 70),
                            np.arange(ec_.N_PAIR_PODS)])
    rng.shuffle(order)
    ref = ec_.reference(name, False, False, tuple(int(x) for x in order))
    with _engine(ref) as eng:
        full = eng.eval(ref.ec.view.now_ns)
        keys = eng.eval(ref.ec.view.now_ns, mask=False, scores=False)
    ec_.check_eval(ref, full)
    np.testing.assert_array_equal(keys["top1"], full["top1"])


@pytest.mark.parametrize("name", ["slot_pow2", "slot_fit6", "slot_fit599", "slot_fit600", "slot_la599", "most_w",
                                  "slot_most", "slot_big_20000", "slot_big_39999"])
def test_slot_kernels(name):
    """k_eval2 (the slot kernels, 4 slots): a LoadAware weight sum of 3 sends the batch off the class path
    (cls_prepare returns), the LoadAware mean is div_w<false> (fp32 reciprocal).  slot_pow2: power-of-two Fit sums
    (shift); slot_fit6 / 599 / 600: the Fit mean by div_w<false> at weight sums 6, 599 and the validation limit 600;
    slot_la599: LoadAware weights 300 / 299; most_w: MostAllocated weights 2 / 1 / 3 (cpu / memory pods sum 3, so the
    batch is here under the default LoadAware weights too); slot_most: the same with LoadAware sum 3; slot_big_*: keys
    beyond bit 31 on this path."""
    ref = ec_.reference(name)
    with _engine(ref) as eng:
        assert eng.spill_count() == 0 and eng.restricted_count() == 0
        ec_.check_eval(ref, eng.eval(ref.ec.view.now_ns))


@pytest.mark.parametrize("name", ["big_20000", "slot_big_39999"])
def test_sharded_keys_beyond_bit_31(name):
    """The second tile alone (set_shard(1024, N)): k_eval3 / k_eval2 with a column offset, keys beyond bit 31."""
    ref = ec_.reference(name)
    n = ref.ec.n_nodes
    with _engine(ref) as eng:
        eng.set_shard(nat.TILE, n)
        ec_.check_eval(ref, eng.eval(ref.ec.view.now_ns), n - nat.TILE, nat.TILE)


@pytest.mark.parametrize("name", ["shipped", "slot_fit600"])
def test_restricted_pods(name):
    """k_eval_elig (+ k_eval2 for the unrestricted pods): two thirds of the pods carry an eligibility class
    (set_eligibility); the scores are the pair's own, feasibility and top-1 honour the class."""
    ref = ec_.reference(name)
    P, N = ref.ec.n_pods, ref.ec.n_nodes
    cls = np.arange(P) % 3
    masks = np.stack([np.arange(N) % 5 != 2, np.arange(N) % 7 != 3])
    want = ec_.restricted(ref, cls, masks)
    rows = engine.build_pod_rows(ref.cfg, ref.ec.view, ref.idx)
    rows["elig_class"] = cls
    eng = engine.Engine(ref.cfg)
    with eng:
        eng.load_snapshot(engine.build_node_rows(ref.cfg, ref.ec.view))
        eng.set_eligibility(masks)
        eng.set_pods(rows)
        assert eng.restricted_count() == int((cls != 0).sum()) and eng.spill_count() == 0
        ec_.check_eval(want, eng.eval(ref.ec.view.now_ns))


@pytest.mark.parametrize("name", ["shipped", "slot_fit6"])
def test_spill_pods(name):
    """k_eval_spill: the wide variant's batch uses 12 resources, the 8-slot map keeps cpu, memory, batch-cpu and
    batch-memory (the step-aligned ones, requested by most pods) and the pods that need a resource outside it are
    spill pods; the other pods take k_eval2 with 8 slots."""
    ref = ec_.reference(name, False, True)
    rows = engine.build_pod_rows(ref.cfg, ref.ec.view, ref.idx)
    n_slots, slot_res, spill = engine.batch_slot_map(ref.cfg, rows)
    assert n_slots == 8 and set(slot_res[:4]) >= {nat.RES_CPU, nat.RES_MEMORY}
    assert {nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY} <= set(slot_res.tolist())
    assert spill.sum() == 4 and set(np.flatnonzero(spill)) == set(ref.ec.wide_pods[:4].tolist())
    with _engine(ref, pod_rows=rows) as eng:
        assert eng.spill_count() == int(spill.sum())
        ec_.check_eval(ref, eng.eval(ref.ec.view.now_ns))


@pytest.mark.parametrize("name", ["shipped", "most4"])
def test_exact_path_control(name):
    """kg_pair_exact (k_fix_slow): the same cluster with every node outside the fp64 bounds — mid-cpu, scored by the
    config but requested by no pod, has an allocatable of 2^43 — gives planes identical to the fast-path run."""
    ref = ec_.reference(name)
    cfg = ec_.config(name, fit_resources={"cpu": 1, "memory": 1, ec_.BATCH_CPU: 1, ec_.BATCH_MEM: 1,
                                          "kubernetes.io/mid-cpu": 1})
    nodes = ref.ec.view.nodes.copy()
    nodes["allocatable"]["v"][:, nat.RES_MID_CPU] = 1 << 43
    nodes["allocatable"]["present"] |= np.uint32(1 << nat.RES_MID_CPU)
    view = ref.ec.view.with_nodes(nodes)
    m, f, l = ec_.oracle.eval_matrix(cfg, view, ref.idx, view.now_ns)
    assert (m == ref.mask).all() and (f == ref.fit).all() and (l == ref.la).all()
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(engine.build_node_rows(cfg, view))
        eng.set_pods(engine.build_pod_rows(cfg, view, ref.idx))
        slow = eng.eval(view.now_ns)
    with _engine(ref) as eng:
        fast = eng.eval(view.now_ns)
    ec_.check_eval(ref, slow)
    for k in ("mask", "top1"):
        np.testing.assert_array_equal(slow[k], fast[k])
    np.testing.assert_array_equal(slow["scores"][:, :ref.ec.n_nodes], fast["scores"][:, :ref.ec.n_nodes])


@pytest.mark.parametrize("name", ["shipped", "most4", "big_39999"])
def test_cycle_one(name):
    """k_cycle_one (Engine.cycle_one, commit=False, planes=True) for designated pods of every cap class, the filter
    pods included: planes and key equal the batch reference."""
    ref = ec_.reference(name)
    N = ref.ec.n_nodes
    rows = engine.build_pod_rows(ref.cfg, ref.ec.view, ref.idx)
    pods = [4 * j + d for j in range(0, ec_.J, 3) for d in (0, 1, 3)] + ref.ec.filter_pods.tolist()
    with _engine(ref, pod_rows=rows[:1]) as eng:
        for p in pods:
            res = eng.cycle_one(rows[p:p + 1], ref.ec.view.now_ns, commit=False, planes=True)
            assert res["key"] == _key(ref.best_total[p], ref.best_node[p]), p
            np.testing.assert_array_equal(engine.unpack_mask(res["mask"], N)[0], ref.mask[p])
            np.testing.assert_array_equal(res["scores"][0, :N, 0], ref.fit[p])
            np.testing.assert_array_equal(res["scores"][0, :N, 1], ref.la[p])


def _host_eval(cfg, nrows, prows, nodes, now_ns):
    """mask, fit, la [P][len(nodes)] of the host's exact per-pair evaluation (kg_row_eval) on built rows."""
    out = np.zeros((3, len(prows), len(nodes)), np.int64)
    for x, n in enumerate(nodes):
        for p in range(len(prows)):
            out[:, p, x] = engine.row_eval(cfg, nrows[n:n + 1], prows[p:p + 1], now_ns)[:3]
    return out


@pytest.mark.parametrize("name", ["shipped", "slot_fit600"])
def test_device_finalize_after_commit(name):
    """k_commit's kg_finalize_node on the device (kg_divmod64_fp with numerators up to about 2^57): designated
    (pod, node) pairs of the large caps, and small pods onto nodes whose bases are just below 2^50, are committed;
    the snapshot then equals the host rows after engine.row_commit, the committed nodes' columns equal the host's
    exact evaluation of those rows and every other column the oracle's."""
    ref = ec_.reference(name)
    ec, now = ref.ec, ref.ec.view.now_ns
    nrows = engine.build_node_rows(ref.cfg, ec.view)
    prows = engine.build_pod_rows(ref.cfg, ec.view, ref.idx)
    big_class = [i for i in range(0, ec_.N_ALIGNED, 19) if ec_.CAPS[i % ec_.C] >= 1 << 36]
    pairs = [(4 * (i % ec_.J) + (x % 4), i) for x, i in enumerate(big_class)][:32]
    pairs += [(4 * (x % ec_.C), int(n)) for x, n in enumerate(ec.big_nodes[:10])]
    assert len(pairs) >= 40 and len({n for _, n in pairs}) == len(pairs)
    with _engine(ref, nrows, prows) as eng:
        for p, n in pairs:
            assert eng.commit(p, n)
            engine.row_commit(ref.cfg, nrows[n:n + 1], prows[p:p + 1])
        res = eng.eval(now)
        np.testing.assert_array_equal(eng.download(), nrows)
    touched = np.array([n for _, n in pairs])
    bases = nrows["nonzero_requested"][touched]
    assert ((bases > (1 << 50) - (1 << 24)) & (bases < 1 << 50)).any()   # 100·(cap − base) near −2^57
    m, f, l = _host_eval(ref.cfg, nrows, prows, touched, now)
    N = ec.n_nodes
    mask = engine.unpack_mask(res["mask"], N)
    np.testing.assert_array_equal(mask[:, touched], m.astype(bool))
    np.testing.assert_array_equal(res["scores"][:, touched, 0], f)
    np.testing.assert_array_equal(res["scores"][:, touched, 1], l)
    rest = np.setdiff1d(np.arange(N), touched)
    np.testing.assert_array_equal(mask[:, rest], ref.mask[:, rest])
    np.testing.assert_array_equal(res["scores"][:, rest, 0], ref.fit[:, rest])
    np.testing.assert_array_equal(res["scores"][:, rest, 1], ref.la[:, rest])
    total = ref.total.copy()
    w = int(ref.cfg["weight_fit"]) * f + int(ref.cfg["weight_loadaware"]) * l
    total[:, touched] = np.where(m.astype(bool), w, -1)
    node, tot = engine.decode_top1(res["top1"])
    np.testing.assert_array_equal(tot, total.max(axis=1))
    np.testing.assert_array_equal(node, np.where(total.max(axis=1) >= 0, total.argmax(axis=1), -1))


@pytest.mark.parametrize("chunk", [1, 16])
@pytest.mark.parametrize("name", ["shipped", "most4"])
def test_placement(name, chunk):
    """kg_place (k_eval3's top-k form per chunk, k_resolve re-deriving the touched nodes' planes on the device between
    pods) against the sequential oracle, at place_chunk 1 and 16; the snapshot after it equals the host replay."""
    ref = ec_.reference(name)
    cfg = ec_.config(name, place_chunk=chunk)
    view = ref.ec.view
    nrows = engine.build_node_rows(cfg, view)
    prows = engine.build_pod_rows(cfg, view, ref.idx)
    ref_nodes, ref_scores = ec_.oracle.schedule(cfg, view, ref.idx, view.now_ns)
    assert (ref_nodes >= 0).sum() >= ec_.N_PAIR_PODS // 2
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(nrows)
        eng.set_pods(prows)
        nodes, scores = eng.place(view.now_ns)
        after = eng.download()
    np.testing.assert_array_equal(nodes, ref_nodes)
    np.testing.assert_array_equal(scores, ref_scores)
    for p, n in enumerate(nodes):
        if n >= 0:
            engine.row_commit(cfg, nrows[n:n + 1], prows[p:p + 1])
    np.testing.assert_array_equal(after, nrows)


@pytest.mark.parametrize("name", ["shipped", "most4", "slot_pow2", "slot_fit600"])
def test_negative_bases(name):
    """Bases in (−2^49, 0) whose sum with the designated pod's request lies in [0, cap] (the three recorded tuples and
    the sweep pair of the negative variant), on the class path (shipped, most4: k_eval3 / k_eval3_dup) and on k_eval2
    (slot_*): kg_finalize_* hands these nodes to the exact path (kg_pair_exact).  While negative bases were admitted
    to the fast path these cases failed: F is far outside [0, 100] there and its ulp exceeds 1/cap."""
    ec = ec_.edge_cluster(ec_.is_most(name), True)
    ref = ec_.reference(name, True, False, tuple(int(p) for p in ec.neg_pods))
    sub = ref.mask[:, ec.neg_nodes]
    assert sub.sum() >= len(ec.neg_nodes) and sub.any(axis=0).all()
    with _engine(ref) as eng:
        ec_.check_eval(ref, eng.eval(ec.view.now_ns), feasible_only=True)
