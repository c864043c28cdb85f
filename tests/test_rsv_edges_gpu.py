"""The designed Reservation / ElasticQuota clusters (tests/rsv_edge_cases.py; what they contain is proved from the
oracle in tests/test_rsv_edges_cpu.py) on the HIP engine: matrix mode bit for bit against oracle.eval_matrix5 (mask,
Fit, LoadAware, NUMA, the normalized Reservation plane, top1) and kg_place against oracle.schedule2 (nodes, scores,
reservation and quota states, snapshot rows)."""
import functools
import os
import uuid

import numpy as np
import pytest

import rsv_edge_cases as rc
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import make_config, shipped_profile
from oracle import oracle

pytestmark = pytest.mark.gpu

RSV = ("NodeResourcesFit", "LoadAwareScheduling", "Reservation")
RSV_EQ = RSV + ("ElasticQuota",)
PROFILE = RSV_EQ + ("NodeNUMAResource",)
W_MAX = 40000 - 2   # kg_config_validate: the plugin weights sum to at most 40000 (Fit 1 + LoadAware 1 beside it)
SHAPE_PODS = ("P", "M99", "OUT32", "T", "M33", "S", "I", "Z", "OA", "OD", "R", "Q", "M100", "plain", "F1:pass", "Q0:pass")


def _engine(cfg, view, idx):
    eng = engine.Engine(cfg)
    eng.load_snapshot(engine.build_node_rows(cfg, view))
    if int(cfg["enabled_plugins"]) & nat.PLUGIN_RESERVATION and len(view.rsv_arr):
        eng.set_reservations(view.rsv_arr)
    if int(cfg["enabled_plugins"]) & nat.PLUGIN_ELASTICQUOTA:
        eng.set_quotas(view.quota_arr)
    eng.set_pods(engine.build_pod_rows(cfg, view, idx))
    return eng


def _compare(cfg, res, ref, b=0, e=None, top1=True):
    m, fit, la, numa, rsv, t1 = ref
    e = m.shape[1] if e is None else e
    W = e - b
    np.testing.assert_array_equal(engine.unpack_mask(res["mask"], W), m[:, b:e], err_msg="mask")
    np.testing.assert_array_equal(res["scores"][:, :W, 0], fit[:, b:e], err_msg="fit")
    np.testing.assert_array_equal(res["scores"][:, :W, 1], la[:, b:e], err_msg="loadaware")
    if int(cfg["enabled_plugins"]) & nat.PLUGIN_NUMA:
        np.testing.assert_array_equal(res["numa_scores"][:, :W], numa[:, b:e], err_msg="numa")
    np.testing.assert_array_equal(res["rsv_scores"][:, :W], rsv[:, b:e], err_msg="reservation plane")
    if top1:
        np.testing.assert_array_equal(res["top1"], t1, err_msg="top1")


def _check_matrix(cfg, view, idx):
    with _engine(cfg, view, idx) as eng:
        res = eng.eval(view.now_ns)
    ref = oracle.eval_matrix5(cfg, view, idx, view.now_ns)
    _compare(cfg, res, ref)
    return ref


@functools.lru_cache(maxsize=None)
def _one_copy():
    return rc.make_rsv_edge_cluster(1)


CONFIGS = {
    "rsv-alone": lambda: make_config(plugins=("Reservation",)),
    "fit+la+rsv": lambda: shipped_profile(plugins=RSV),
    "quota": lambda: shipped_profile(plugins=RSV_EQ),
    "quota-parents": lambda: shipped_profile(plugins=RSV_EQ, eq_check_parent_quota=1),
    "numa": lambda: shipped_profile(plugins=PROFILE, weight_numa=2, eq_check_parent_quota=1),
    "w1": lambda: make_config(plugins=RSV_EQ, weight_reservation=1),
    "w7-most": lambda: make_config(plugins=RSV_EQ, weight_fit=3, weight_loadaware=2, weight_reservation=7,
                                   fit_strategy="MostAllocated"),
    "wmax": lambda: make_config(plugins=RSV_EQ, weight_reservation=W_MAX),
}


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("part", [0, 1, 2])
def test_one_copy_matrix(name, part):
    """Every family of one copy, a third of its pods per case, per plugin set and Reservation weight."""
    ec = _one_copy()
    idx = np.arange(ec.n_pods)[part::3]
    assert 8 <= len(idx) <= 24
    m, _, _, _, rsv, top1 = _check_matrix(CONFIGS[name](), ec.view, idx)
    assert m.any() and rsv.max() == 100 and (top1 > 0).any()


@pytest.mark.parametrize("plain_first", [True, False], ids=["plain-lower", "plain-higher"])
@pytest.mark.parametrize("weight", [1, 7, W_MAX])
def test_base_total_tie_keeps_the_lowest_index(plain_first, weight):
    """A reservation node and a plain node with equal totals: the reservation-node best merged into top1 keeps the
    lower index, whichever of the two it is."""
    tc = rc.tie_cluster(plain_first)
    cfg = make_config(plugins=RSV, weight_reservation=weight)
    m, fit, la, _, _, top1 = _check_matrix(cfg, tc.view, np.arange(tc.n_pods))
    assert m.all() and (fit[:, 0] == fit[:, 1]).all() and (la[:, 0] == la[:, 1]).all()
    assert (engine.decode_top1(top1)[0] == 0).all()


@pytest.mark.parametrize("n_rn,variant", [(n, v) for n in rc.GPU_SHAPES for v in (0, 1) if n >= 64 or v == 0])
def test_shapes(n_rn, variant):
    """n_rn reservation nodes around the wave, block and unroll-trip sizes of rsv_best_block, the decisive entries
    (preferred node, largest raw, best key) at group edges, at the last rank and past rank 2048."""
    ec = rc.make_rsv_edge_cluster(-(-n_rn // 100) + 1, n_rn=n_rn, at=rc.decisive_ranks(n_rn, variant))
    idx = [ec.pod(t) for t in SHAPE_PODS]
    _check_matrix(shipped_profile(plugins=RSV_EQ), ec.view, idx)


def test_shards():
    """set_shard windows that cut through the reservation nodes, hold none of them, and leave the preferred nodes
    outside: the window's plane columns, then the max over the shards' top1 against the unsharded oracle."""
    ec = rc.make_rsv_edge_cluster(6, n_rn=600, n_plain=1500)
    N = len(ec.view.nodes)
    windows = ((0, 1024), (1024, 2048), (2048, N))
    assert ec.rn.max() < 2048 < N and ((ec.rn >= 1024) & (ec.rn < 2048)).any() and (ec.rn < 1024).any()
    idx = sorted({ec.pod(t) for t in ("P", "T", "OA")} | set(range(0, ec.n_pods, 3)))
    cfg = shipped_profile(plugins=RSV_EQ)
    ref = oracle.eval_matrix5(cfg, ec.view, idx, ec.view.now_ns)
    pref = engine.decode_top1(ref[5])[0]
    assert (pref[[idx.index(ec.pod(t)) for t in ("P", "T", "OA")]] < 1024).all()   # outside the two upper windows
    best = np.zeros(len(idx), np.uint64)
    with _engine(cfg, ec.view, idx) as eng:
        for b, e in windows:
            eng.set_shard(b, e)
            res = eng.eval(ec.view.now_ns)
            _compare(cfg, res, ref, b, e, top1=False)
            best = np.maximum(best, res["top1"].astype(np.uint64))
    np.testing.assert_array_equal(best, ref[5])


@pytest.mark.parametrize("P", [1024, 1025])
def test_entry_passes(P):
    """A matrix batch at and past KG_RSV_POD_CHUNK pods: the second entry pass."""
    ec = rc.make_rsv_edge_cluster(1, n_rn=65)
    idx = np.arange(P) % ec.n_pods
    ref = _check_matrix(shipped_profile(plugins=RSV_EQ), ec.view, idx)
    assert ref[4][P - 1].max() == ref[4][(P - 1) % ec.n_pods].max()


def test_device_outputs_equal_host_outputs():
    import torch
    dev = torch.device("cuda", 0)   # torch's HIP context first (it does not initialise beside a live engine)
    ec = _one_copy()
    idx = np.arange(ec.n_pods)[::3]
    P, W = len(idx), (len(ec.view.nodes) + 63) // 64
    mask = torch.zeros((P, W), dtype=torch.int64, device=dev)
    scores = torch.zeros((P, W * 64, 2), dtype=torch.uint8, device=dev)
    rsv = torch.zeros((P, W * 64), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(P, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    cfg = shipped_profile(plugins=RSV_EQ)
    with _engine(cfg, ec.view, idx) as eng:
        host = eng.eval(ec.view.now_ns)
        eng.eval_device(ec.view.now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr(), 0, rsv.data_ptr())
        eng.sync()
    _compare(cfg, host, oracle.eval_matrix5(cfg, ec.view, idx, ec.view.now_ns))
    np.testing.assert_array_equal(mask.cpu().numpy().view(np.uint64), host["mask"])
    np.testing.assert_array_equal(scores.cpu().numpy(), host["scores"])
    np.testing.assert_array_equal(rsv.cpu().numpy(), host["rsv_scores"])
    np.testing.assert_array_equal(top1.cpu().numpy().view(np.uint64), host["top1"])


def test_required_affinity_without_any_reservation():
    """An affinity-required pod on an engine that holds no reservation at all, beside a pod without the affinity."""
    ec = _one_copy()
    v = rc.build_view([u for u in ec.units if not u["rsv"]], rc.family_pods(), rc.family_quotas())
    idx = [ec.pod("NONE"), ec.pod("NONEn"), ec.pod("F1:pass"), ec.pod("P")]
    m = _check_matrix(shipped_profile(plugins=RSV_EQ), v, idx)[0]
    assert m.any(axis=1).tolist() == [False, True, False, True]


# ---- placement -----------------------------------------------------------------------------------------------------

def _place_and_compare(eng, cfg, view, idx, shard=None):
    """kg_place (under `shard`: kg_place_sharded on one loopback rank) against oracle.schedule2: nodes, scores,
    reservation and quota states, and the snapshot rows replayed with row_commit.  A rank evaluates its shard's plain
    nodes and every reservation node (koord_gpu.h, kg_rsv_set), so the reference cycle runs on the view with the
    plain nodes outside the shard closed (no pod slot left: NodeResourcesFit rejects them)."""
    ref_view = view
    if shard is not None:
        b, e = shard
        nodes_ref = view.nodes.copy()
        plain = np.ones(len(nodes_ref), bool)
        plain[view.rsv_arr["node"]] = False
        plain[b:e] = False
        nodes_ref["allowed_pods"][plain] = 0
        ref_view = view.with_nodes(nodes_ref)
        eng.set_shard(b, e)
        eng.comm_init_loopback(0, 1, f"/kg_rsv_edges_{os.getpid()}_{uuid.uuid4().hex[:8]}")
        nodes, scores = eng.place_sharded(view.now_ns)
    else:
        nodes, scores = eng.place(view.now_ns)
    after = eng.download()
    rsv_after = eng.download_reservations()
    q_after = eng.download_quotas() if len(view.quota_arr) else None
    ref_nodes, ref_scores, ref_rsv, ref_q = oracle.schedule2(cfg, ref_view, idx, view.now_ns)
    np.testing.assert_array_equal(nodes, ref_nodes)
    np.testing.assert_array_equal(scores, ref_scores)
    np.testing.assert_array_equal(rsv_after["n_assigned"], ref_rsv["n_assigned"])
    np.testing.assert_array_equal(rsv_after["allocated"]["v"], ref_rsv["allocated"]["v"])
    if q_after is not None:
        np.testing.assert_array_equal(q_after["used"]["v"], ref_q["used"]["v"])
        np.testing.assert_array_equal(q_after["non_preemptible_used"]["v"], ref_q["non_preemptible_used"]["v"])
    rows = engine.build_node_rows(cfg, view)
    prow = engine.build_pod_rows(cfg, view, idx)
    for p, n in enumerate(nodes):
        if n >= 0:
            engine.row_commit(cfg, rows[n:n + 1], prow[p:p + 1])
    np.testing.assert_array_equal(after, rows)
    return ref_nodes


def _check_place(cfg, view, idx, shard=None):
    with _engine(cfg, view, idx) as eng:
        return _place_and_compare(eng, cfg, view, idx, shard)


@pytest.mark.parametrize("check_parent", [0, 1])
@pytest.mark.parametrize("chunk", [1, 16, 64])
def test_queue_placement(chunk, check_parent):
    """The queue whose reductions change inside a chunk: an allocate-once reservation holding the class's only order
    (inside a chunk of 16 and across its boundary), a Restricted reservation and two quota groups filled to the
    limit, a commit on the node holding its group's best base key, a commit on a plain node in between."""
    qc = rc.make_queue_cluster()
    cfg = shipped_profile(plugins=RSV_EQ, place_chunk=chunk, eq_check_parent_quota=check_parent)
    nodes = _check_place(cfg, qc.view, np.arange(qc.n_pods))
    assert (nodes == -1).sum() == 2 + check_parent


@pytest.mark.parametrize("chunk", [1, 16, 64])
def test_one_copy_placement(chunk):
    """Every pod of the family cluster through kg_place, twice over (the second round meets the first one's state)."""
    ec = _one_copy()
    cfg = shipped_profile(plugins=RSV_EQ, place_chunk=chunk, eq_check_parent_quota=1)
    _check_place(cfg, ec.view, np.concatenate([np.arange(ec.n_pods)] * 2))


@pytest.mark.parametrize("chunk", [1, 16, 64])
@pytest.mark.parametrize("variant", ["order", "raw", "far"])
def test_wide_class_placement(variant, chunk):
    """1023, 1024, 1025 and 1500 scored entries per pod (the resolve prefetches 1024 of them into LDS); the deciding
    entry is the last rank's.  "far": it is never the chosen node, so no pod finds it on the chunk's touched list."""
    wc = rc.make_wide_class_cluster(variant)
    cfg = shipped_profile(plugins=RSV, place_chunk=chunk, weight_reservation=1 if variant == "far" else 5000)
    nodes = _check_place(cfg, wc.view, np.arange(wc.n_pods))
    last = wc.node(f"w:{len(wc.rn) - 1}")
    assert (nodes >= 0).all() and ((nodes != last).all() if variant == "far" else nodes[0] == last)


def test_fallback_reduce():
    """131,073 reservation nodes: more entry groups than the resolve's flags cover, so it reduces over every entry
    (rsv_best_block on 512 threads).  6 pods in chunks of 4, and one matrix pass."""
    fv = rc.make_fallback_cluster()
    cfg = shipped_profile(plugins=RSV, place_chunk=4)
    idx = np.arange(6)
    with _engine(cfg, fv, idx) as eng:
        res = eng.eval(fv.now_ns)
        _compare(cfg, res, oracle.eval_matrix5(cfg, fv, idx, fv.now_ns))
        ref_nodes = _place_and_compare(eng, cfg, fv, idx)
    assert (ref_nodes[:5] >= 2048 * 64 - 4).all()


SHARD_PAD = 1100   # plain nodes in the middle of the queue cluster: the A2 family and 40 fillers sit past node 1024


@pytest.mark.parametrize("shard", ["lower", "upper"])
@pytest.mark.parametrize("chunk", [1, 16, 64])
def test_queue_placement_one_sharded_rank(chunk, shard):
    """kg_place_sharded on one loopback rank whose shard excludes part of the reservation nodes: the lower window
    leaves the A2 family outside, the upper one the A family, B, X and the best plain node.  Every reservation node
    stays a candidate (their entries are evaluated on every rank); the plain nodes outside the window do not."""
    qc = rc.make_queue_cluster(pad=SHARD_PAD)
    N = len(qc.view.nodes)
    b, e = (0, 1024) if shard == "lower" else (1024, N)
    assert ((qc.rn >= b) & (qc.rn < e)).any() and ((qc.rn < b) | (qc.rn >= e)).any()
    assert (qc.node("A2:once") >= 1024) and (qc.node("X") < 1024) and qc.node("plain:best") < 1024
    cfg = shipped_profile(plugins=RSV_EQ, place_chunk=chunk, eq_check_parent_quota=1)
    nodes = _check_place(cfg, qc.view, np.arange(qc.n_pods), (b, e))
    outside = [n for n in nodes.tolist() if n >= 0 and not b <= n < e]
    assert outside and all(qc.units[n]["rsv"] for n in outside)   # reservation nodes outside the shard are chosen
