"""Node eligibility classes on the GPU (kg_elig_set / kg_elig_update, kg_pod_row.elig_class, k_eval_elig): every path
where the engine chooses or reports a node honours the class of a restricted pod.

Matrix mode is compared with the oracle restricted in numpy (tests/elig_cases.py: mask AND class, scores where the
mask is set, top-1 over the restricted mask); placement with a host replay through engine.row_eval / row_commit, one
twin case with oracle.schedule itself (classes as named scalar resources), and Reservation + ElasticQuota placement
with the sequence of one-pod kg_pods_set + kg_eval + kg_commit.  N = 2500 nodes (3 tiles, the last partial; 39 full
mask words and 4 bits), P = 37 pods; the preconditions that keep these tests from passing vacuously are asserted from
the oracle in tests/test_elig_cpu.py (the light ones again here, on the cached answers)."""
import os

import numpy as np
import pytest

import elig_cases as ec
from koordinator_amd import _native as nat
from koordinator_amd import engine

pytestmark = pytest.mark.gpu

ERR_RANGE, ERR_STATE = "status -4", "status -5"


def _eval_checked(c, shard=None, forms=0):
    with ec.engine_of(c, forms=forms, shard=shard) as eng:
        assert eng.restricted_count() == int(c.restricted.sum())
        out = eng.eval(c.cl.now_ns)
    b, e = shard or (0, c.N)
    assert out["mask"].shape[1] == (e - b + 63) // 64
    ec.check_planes(c.cfg, out, **c.planes(b, e))
    return out


def _changes_something(c, begin=0, end=None):
    """The class takes feasible nodes away from restricted pods (on the cached oracle planes)."""
    end = c.N if end is None else end
    return bool((c.free[0][c.restricted, begin:end] & ~c.matrix[0][c.restricted, begin:end]).any())


# ---- matrix mode ---------------------------------------------------------------------------------------------------
def test_matrix_mixed():
    c = ec.case("mixed")
    assert 0.25 <= c.restricted.mean() <= 0.75 and _changes_something(c)
    with ec.engine_of(c) as eng:
        assert eng.spill_count() == 0
    _eval_checked(c)


def test_matrix_mixed_shard():
    c = ec.case("mixed")
    assert _changes_something(c, *ec.SHARD)
    _eval_checked(c, shard=ec.SHARD)


@pytest.mark.parametrize("name", ["first", "last", "every"])
def test_matrix_restricted_pod_positions(name):
    c = ec.case(name)
    want = {"first": [0], "last": [c.P - 1], "every": list(range(c.P))}[name]
    assert c.P == 37 and np.flatnonzero(c.restricted).tolist() == want and _changes_something(c)
    out = _eval_checked(c)
    with ec.engine_of(c) as eng:
        keys = eng.eval(c.cl.now_ns, mask=False, scores=False)["top1"]   # the keys-only form of the kernels
    np.testing.assert_array_equal(keys, out["top1"])


def test_class_all_equals_unrestricted():
    c_all, c_zero = ec.case("all_vs_zero")
    assert c_all.restricted.all() and not c_zero.restricted.any()
    a = _eval_checked(c_all)
    z = _eval_checked(c_zero)
    for k in ("mask", "top1"):
        np.testing.assert_array_equal(a[k], z[k])
    np.testing.assert_array_equal(a["scores"][:, :c_all.N], z["scores"][:, :c_all.N])


def test_matrix_wide_and_restricted():
    """More than 8 resources: some pods are spill pods, some restricted, some both (k_eval_spill, then k_eval_elig)."""
    c = ec.case("wide")
    assert (c.spill & c.restricted).any() and (c.spill & ~c.restricted).any() and _changes_something(c)
    with ec.engine_of(c) as eng:
        assert eng.spill_count() == int(c.spill.sum())   # its meaning is unchanged: spill for width
    _eval_checked(c)


@pytest.mark.parametrize("name", ["numa_eq", "numa_distinct"])
def test_matrix_numa(name):
    """NodeNUMAResource: repeated rows (eq_on, the COMBINE form reads the repaired planes back; rows that differ only
    in class are distinct rows) and a batch of distinct rows with pairs differing only in class."""
    c = ec.case(name)
    rows = {r.tobytes() for r in c.pod_rows}
    if name == "numa_eq":
        assert c.P >= 64 and 4 * len(rows) <= 3 * c.P
        same_spec = c.idx[:6]
        assert len(set(same_spec.tolist())) == 1 and len(set(c.elig_class[:6].tolist())) >= 3
    else:
        assert (c.idx[0::2][:18] == c.idx[1::2]).all() and (c.elig_class[0::2][:18] != c.elig_class[1::2]).any()
    assert _changes_something(c)
    _eval_checked(c)


def test_matrix_reservation_quota():
    """Reservation + ElasticQuota: reservation nodes eligible and ineligible for a pod, a pod whose preferred
    reservation node is ineligible; rsv_scores and top1 against eval_matrix5 re-reduced over the eligible entries."""
    c = ec.rsv_case()
    (m, f, l, plane, top1), moved = ec.rsv_reference(c)
    assert moved >= 1
    with ec.engine_of(c) as eng:
        out = eng.eval(c.cl.now_ns)
    np.testing.assert_array_equal(engine.unpack_mask(out["mask"], c.N), m)
    np.testing.assert_array_equal(out["scores"][:, :c.N, 0], np.where(m, f, out["scores"][:, :c.N, 0]))
    np.testing.assert_array_equal(out["scores"][:, :c.N, 1], np.where(m, l, out["scores"][:, :c.N, 1]))
    np.testing.assert_array_equal(out["rsv_scores"][:, :c.N], plane)
    np.testing.assert_array_equal(out["top1"], top1)


@pytest.mark.parametrize("name", ["lax", "exact"])
def test_matrix_loadaware_extra_weights(name):
    """k_eval2's LAX form (then k_eval_elig and the KGD_XSLOW fix-up) and k_eval_exact."""
    c = ec.case(name)
    assert _changes_something(c)
    _eval_checked(c)


def test_matrix_slow_nodes():
    """Nodes outside the fp64 bounds (k_fix_slow), eligible and ineligible."""
    c = ec.case("slow")
    slow = np.array(ec.SLOW_NODES)
    r = np.flatnonzero(c.restricted)
    assert c.free[0][r][:, slow].any() and (c.free[0][r][:, slow] & ~c.matrix[0][r][:, slow]).any()
    _eval_checked(c)


def test_guarded_outputs():
    """The mixed batch into guarded device buffers (tests/guarded_out.py), prefilled 0x00 and 0xFF: guards intact,
    pad bits 0, the same answers."""
    import torch
    from guarded_out import GuardedOutputs, specified_cells
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    c = ec.case("mixed")
    request = ("mask", "scores", "top1")
    for shard in (None, ec.SHARD):
        b, e = shard or (0, c.N)
        runs = []
        with ec.engine_of(c, shard=shard) as eng:
            for prefill in (0x00, 0xFF):
                got = GuardedOutputs(c.P, e - b, prefill, dev).eval(eng, c.cl.now_ns, request)   # asserts the guards
                ec.check_planes(c.cfg, got, **c.planes(b, e))   # (and the mask's pad bits)
                runs.append(specified_cells(got, e - b))
        for k in request:
            np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


# ---- placement -----------------------------------------------------------------------------------------------------
def _check_replay(c, nodes, scores, after=None):
    ref_n, ref_s, ref_rows = c.replayed
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)
    if after is not None:
        np.testing.assert_array_equal(after, ref_rows)


@pytest.mark.parametrize("name,forms", [("place16", 0), ("place16", nat.FORM_PLACE_PIPELINE), ("place1", 0)],
                         ids=["chunk16", "chunk16_pipeline", "chunk1"])
def test_place(name, forms):
    c = ec.case(name)
    ref_n = c.replayed[0]
    r = np.flatnonzero(c.restricted & (ref_n >= 0))
    assert len(r) and all(c.masks[c.elig_class[p] - 1][ref_n[p]] for p in r)
    with ec.engine_of(c, forms=forms) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
        after = eng.download()
    _check_replay(c, nodes, scores, after)


def test_place_chunk_api_and_sharded():
    """kg_place_chunk_eval / kg_place_chunk_resolve_prev on their two streams (dist.place) and kg_place_sharded's own
    loop (one rank, loopback communicator), the table loaded through `eligibility=`."""
    import torch
    from koordinator_amd import dist as kdist
    c = ec.case("place16")
    nodes, scores = kdist.place(c.cfg, c.node_rows, c.pod_rows, c.cl.now_ns, torch.device("cuda", 0),
                                eligibility=c.masks)
    _check_replay(c, nodes, scores)
    eng = kdist.native_engine(c.cfg, c.node_rows, c.pod_rows, torch.device("cuda", 0), comm="loopback", rank=0,
                              world=1, shm_name=f"/kg_elig_{os.getpid()}", eligibility=c.masks)
    try:
        nodes, scores = eng.place_sharded(c.cl.now_ns)
        after = eng.download()
    finally:
        eng.close()
    _check_replay(c, nodes, scores, after)


def test_place_numa():
    c = ec.case("numa_place")
    assert not (c.pod_rows["flags"] & nat.POD_NUMA_CPU_BIND).any()
    with ec.engine_of(c) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
        after = eng.download()
    _check_replay(c, nodes, scores, after)


def test_place_twin_against_oracle_schedule():
    """The classes as unweighted named scalars (RES_EXT0 + k: 2^40 on the class's nodes, absent elsewhere, each
    restricted pod requesting 1): oracle.schedule on the twin equals the engine on the original view with classes."""
    from oracle import oracle
    c, view = ec.twin()
    ref_n, ref_s = oracle.schedule(c.cfg, view, c.idx, c.cl.now_ns)
    free_n, _ = oracle.schedule(c.cfg, c.cl, c.idx, c.cl.now_ns)
    assert (ref_n != free_n).any() and (ref_n[c.restricted] >= 0).any()
    with ec.engine_of(c) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)


def test_place_reservation_quota():
    """kg_place equals the sequence of one-pod kg_pods_set + kg_eval(top1) + kg_commit (whose matrix form is
    oracle-checked above); the reservation, quota and snapshot downloads are equal too."""
    c = ec.rsv_case()
    with ec.engine_of(c) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
        state = (eng.download(), eng.download_reservations(), eng.download_quotas())
    seq_n, seq_s = np.full(c.P, -1, np.int32), np.full(c.P, -1, np.int64)
    with ec.engine_of(c) as eng:
        for p in range(c.P):
            eng.set_pods(c.pod_rows[p:p + 1])
            n, s = engine.decode_top1(eng.eval(c.cl.now_ns, mask=False, scores=False, rsv_scores=False)["top1"])
            seq_n[p], seq_s[p] = int(n[0]), int(s[0])
            if n[0] >= 0:
                assert eng.commit(0, int(n[0]))
        seq_state = (eng.download(), eng.download_reservations(), eng.download_quotas())
    r = np.flatnonzero(c.restricted & (seq_n >= 0))
    assert len(r) and all(c.masks[c.elig_class[p] - 1][seq_n[p]] for p in r)
    assert np.isin(seq_n[r], np.unique(c.cl.rsv_arr["node"])).any()
    np.testing.assert_array_equal(nodes, seq_n)
    np.testing.assert_array_equal(scores, seq_s)
    for a, b in zip(state, seq_state):
        np.testing.assert_array_equal(a, b)


# ---- kg_cycle_one ----------------------------------------------------------------------------------------------------
def test_cycle_one_restricted_pod():
    c = ec.case("mixed")
    m, f, l = c.matrix
    want_n, want_t = ec.best_of(m, ec.totals(c.cfg, f, l))
    with ec.engine_of(c) as eng:
        for p in range(c.P):
            res = eng.cycle_one(c.pod_rows[p:p + 1], c.cl.now_ns, commit=False, planes=True)
            assert (res["node"], res["score"]) == (int(want_n[p]), int(want_t[p])), p
            key = 0 if want_n[p] < 0 else ((int(want_t[p]) + 1) << 32) | (0xFFFFFFFF - int(want_n[p]))
            assert res["key"] == key, p
            np.testing.assert_array_equal(engine.unpack_mask(res["mask"], c.N)[0], m[p])
            topk = eng.cycle_one(c.pod_rows[p:p + 1], c.cl.now_ns, commit=False)   # the top-1-only form
            assert (topk["key"], topk["node"], topk["score"]) == (key, res["node"], res["score"])
        np.testing.assert_array_equal(eng.download(), c.node_rows)


def test_cycle_one_committed_sequence():
    c = ec.case("place16")
    nodes, scores = [], []
    with ec.engine_of(c) as eng:
        for p in range(c.P):
            res = eng.cycle_one(c.pod_rows[p:p + 1], c.cl.now_ns, commit=True)
            assert res["committed"] == (res["node"] >= 0)
            nodes.append(res["node"])
            scores.append(res["score"])
        after = eng.download()
    _check_replay(c, np.array(nodes), np.array(scores), after)


# ---- the table's lifecycle ---------------------------------------------------------------------------------------------
def test_update_flips_the_best_node():
    c = ec.case("mixed")
    m, f, l = c.matrix
    t = ec.totals(c.cfg, f, l)
    p = int(np.flatnonzero(c.of_class("half") & (m.sum(axis=1) >= 2))[0])
    k = int(c.elig_class[p]) - 1
    best, _ = ec.best_of(m[p:p + 1], t[p:p + 1])
    m2 = m[p:p + 1].copy()
    m2[0, best[0]] = False
    second, second_t = ec.best_of(m2, t[p:p + 1])
    assert second[0] >= 0 and second[0] != best[0]
    with ec.engine_of(c) as eng:
        top = lambda: engine.decode_top1(eng.eval(c.cl.now_ns, mask=False, scores=False)["top1"])
        n0, t0 = top()
        assert n0[p] == best[0]
        eng.update_eligibility(k, [int(best[0])], False)
        n1, t1 = top()
        assert (n1[p], t1[p]) == (second[0], second_t[0])
        others = np.flatnonzero(c.elig_class != k + 1)
        np.testing.assert_array_equal(n1[others], n0[others])
        eng.update_eligibility(k, [int(best[0])], True)
        n2, t2 = top()
        np.testing.assert_array_equal(n2, n0)
        np.testing.assert_array_equal(t2, t0)


def test_update_keeps_the_tile_counts():
    """`pool`'s tile emptied node by node: the planes equal the oracle's at every checkpoint, the last with the tile's
    count at 0 (the skip path), then refilled."""
    c = ec.case("mixed")
    k = ec.CLS["pool"] - 1
    pods = np.flatnonzero(c.of_class("pool"))
    assert len(pods) and c.free[0][pods][:, 1024:2048].any()
    masks = np.array(c.masks)
    order = np.random.default_rng(9).permutation(np.arange(1024, 2048))
    with ec.engine_of(c) as eng:
        done = 0
        for upto in (1, 64, 1000, 1023, 1024):
            for j in order[done:upto]:
                eng.update_eligibility(k, [int(j)], False)
            masks[k, order[done:upto]] = False
            done = upto
            out = eng.eval(c.cl.now_ns)
            m = ec.restrict(c.free[0], masks, c.elig_class)
            ec.check_planes(c.cfg, out, m, c.free[1], c.free[2])
        assert not m[pods].any() and (engine.decode_top1(out["top1"])[0][pods] == -1).all()
        eng.update_eligibility(k, order, np.ones(1024, bool))   # one call, many nodes
        out = eng.eval(c.cl.now_ns)
    ec.check_planes(c.cfg, out, **c.planes())


def test_set_ignores_bits_past_the_snapshot_and_accepts_packed_words():
    c = ec.case("mixed")
    packed = engine.pack_eligibility(c.masks).copy()
    packed[:, -1] |= ~np.uint64((1 << (c.N % 64)) - 1)   # garbage in the pad bits
    with ec.engine_of(c, with_table=False) as eng:
        eng.set_eligibility(packed)
        out = eng.eval(c.cl.now_ns)
    ec.check_planes(c.cfg, out, **c.planes())


def test_reset_drops_the_table_and_upsert_keeps_it():
    c = ec.case("mixed")
    with ec.engine_of(c) as eng:
        eng.upsert(np.arange(c.N, dtype=np.int32), c.node_rows)   # kg_snapshot_upsert leaves the table alone
        ec.check_planes(c.cfg, eng.eval(c.cl.now_ns), **c.planes())
        eng.load_snapshot(c.node_rows)                             # kg_snapshot_reset drops it
        with pytest.raises(engine.EngineError, match=ERR_RANGE):
            eng.eval(c.cl.now_ns)
        eng.set_eligibility(c.masks)
        ec.check_planes(c.cfg, eng.eval(c.cl.now_ns), **c.planes())


def test_error_returns():
    c = ec.case("mixed")
    with engine.Engine(c.cfg) as eng:   # no snapshot
        with pytest.raises(engine.EngineError, match=ERR_STATE):
            eng.n_nodes = c.N
            eng.set_eligibility(c.masks)
    with ec.engine_of(c) as eng:
        want = eng.eval(c.cl.now_ns)
        # the table of another node count
        with pytest.raises(engine.EngineError, match=ERR_RANGE):
            engine._check(nat.lib().kg_elig_set(eng._h, nat.ptr(engine.pack_eligibility(c.masks[:, :c.N - 1])),
                                                len(c.masks), c.N - 1), eng, "kg_elig_set")
        # updates out of range change nothing
        for cls, node in ((len(c.masks), 0), (-1, 0), (0, c.N), (0, -1)):
            with pytest.raises(engine.EngineError, match=ERR_RANGE):
                eng.update_eligibility(cls, [5, node], False)
        got = eng.eval(c.cl.now_ns)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
        # a pod naming a class at or past the loaded count: every entry point refuses, nothing changes
        eng.set_eligibility(c.masks[:3])
        gen = eng.generation()
        import torch
        dev = torch.device("cuda", 0)
        part = torch.zeros((1, eng.num_tiles, eng.partial_slots), dtype=torch.int32, device=dev)
        node = torch.full((2,), -1, dtype=torch.int32, device=dev)
        score = torch.full((1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        ptrs = (part.data_ptr(), node.data_ptr(), score.data_ptr())
        calls = {
            "kg_eval": lambda: eng.eval(c.cl.now_ns),
            "kg_place": lambda: eng.place(c.cl.now_ns),
            "kg_place_chunk_eval": lambda: eng.chunk_eval(c.cl.now_ns, 0, 1, ptrs[0]),
            "kg_place_chunk_resolve": lambda: eng.chunk_resolve(c.cl.now_ns, 0, 1, *ptrs),
            "kg_place_chunk_resolve_prev": lambda: eng.chunk_resolve(c.cl.now_ns, 0, 1, *ptrs, node.data_ptr() + 4, 1),
            "kg_cycle_one": lambda: eng.cycle_one(c.pod_rows[np.flatnonzero(c.elig_class > 3)[:1]], c.cl.now_ns),
        }
        for name, call in calls.items():
            with pytest.raises(engine.EngineError, match=name + ".*" + ERR_RANGE + ".*elig_class"):
                call()
        torch.cuda.synchronize(dev)
        assert not part.any() and (node == -1).all() and (score == -1).all()   # nothing was launched
        bad = c.pod_rows[:1].copy()
        bad["elig_class"] = -2
        with pytest.raises(engine.EngineError, match=ERR_RANGE):
            eng.cycle_one(bad, c.cl.now_ns)
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), c.node_rows)
        # kg_place_sharded checks before its first collective
        eng.comm_init_loopback(0, 1, f"/kg_elig_err_{os.getpid()}")
        with pytest.raises(engine.EngineError, match="kg_place_sharded.*" + ERR_RANGE + ".*elig_class"):
            eng.place_sharded(c.cl.now_ns)
        # kg_commit does not check eligibility (nor the class range): the node is the caller's decision
        p = int(np.flatnonzero(c.of_class("pool"))[0])
        assert not c.masks[ec.CLS["pool"] - 1][0] and eng.commit(p, 0)
        # n_classes = 0 drops the table
        eng.set_eligibility(None)
        with pytest.raises(engine.EngineError, match=ERR_RANGE):
            eng.eval(c.cl.now_ns)
        eng.set_pods(ec.case("all_vs_zero")[1].pod_rows)   # unrestricted pods need no table
        eng.eval(c.cl.now_ns)
