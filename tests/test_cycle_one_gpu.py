"""kg_cycle_one (Engine.cycle_one): the fused one-pod scheduling cycle against matrix mode, the oracle and the host
replay.  The shared cluster has 1,100 nodes — four full 256-node blocks and a ragged one of 76, neither a multiple
of 64 nor of 256 — and nodes beyond the fp64 bounds, so both pair paths and every block's atomic take part."""
import numpy as np
import pytest

import cycle_cases as cc
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile
from numa_cases import make_numa_edge_cluster, numa_config
from oracle import oracle

pytestmark = pytest.mark.gpu


def _loaded(cfg, rows):
    eng = engine.Engine(cfg)
    eng.load_snapshot(rows)
    return eng


@pytest.mark.parametrize("profile", cc.PROFILES)
def test_select_equals_matrix_mode_and_oracle(profile):
    cfg, cl, rows, pods = cc.case(profile)
    m, f, l, tot = cc.oracle_matrix(profile)
    assert m[:, cc.BIG].any() and m.any(axis=1).all()
    with _loaded(cfg, rows) as eng, _loaded(cfg, rows) as twin:
        gen = eng.generation()
        for i in range(cc.N_PODS):
            res = eng.cycle_one(pods[i], cl.now_ns, commit=False, planes=True)
            twin.set_pods(pods[i:i + 1])
            want = int(twin.eval(cl.now_ns, mask=False, scores=False)["top1"][0])
            assert res["key"] == want == cc.key_of(tot[i]), i
            node, score = engine.decode_top1(np.array([want], np.uint64))
            assert (res["node"], res["score"], res["committed"]) == (int(node[0]), int(score[0]), False)
            cc.check_planes(res, cc.N_NODES, m[i], f[i], l[i])
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), rows)


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 255, 256, 257, 1_025])
def test_grid_edges(n_nodes):
    cfg, cl, rows, pods = cc.case("shipped")
    rows = rows[:n_nodes]
    with _loaded(cfg, rows) as eng:
        for i in range(8):
            res = eng.cycle_one(pods[i], cl.now_ns, commit=False, planes=True)
            m, f, l, tot = cc.rows_totals(cfg, rows, pods[i], cl.now_ns)
            assert res["key"] == cc.key_of(tot), i
            cc.check_planes(res, n_nodes, m, f, l)


def _sequential(cfg, cl, n_pods):
    """n_pods committing cycles in queue order: (nodes, scores, rows after, generations gained)."""
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(n_pods))
    nodes, scores = [], []
    with _loaded(cfg, rows) as eng:
        gen = eng.generation()
        for i in range(n_pods):
            res = eng.cycle_one(pods[i], cl.now_ns, commit=True)
            assert res["committed"] == (res["node"] >= 0)
            assert res["key"] == (0 if res["node"] < 0 else ((res["score"] + 1) << 32) | (0xFFFFFFFF - res["node"]))
            nodes.append(res["node"])
            scores.append(res["score"])
        after, gained = eng.download(), eng.generation() - gen
        placed = eng.counters()["placed"]
    nodes, scores = np.array(nodes), np.array(scores)
    assert gained == placed == (nodes >= 0).sum()
    for p, n in enumerate(nodes):   # the host replay
        if n >= 0:
            engine.row_commit(cfg, rows[n:n + 1], pods[p:p + 1])
    np.testing.assert_array_equal(after, rows)
    return nodes, scores


def test_sequential_cycle_equals_oracle():
    cfg, cl, _, _ = cc.case("shipped")
    ref_n, ref_s = oracle.schedule(cfg, cl, np.arange(cc.N_PODS), cl.now_ns)
    # every block's atomic, both pair paths and the commit of a slow node take part
    assert (ref_n >= 0).all() and set(ref_n // 256) == {0, 1, 2, 3, 4} and np.isin(ref_n, cc.BIG).sum() == 9
    nodes, scores = _sequential(cfg, cl, cc.N_PODS)
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)


def test_sequential_cycle_rereads_committed_rows():
    cl = synth.make_cluster(400, 150, seed=43)
    cfg = shipped_profile()
    ref_n, ref_s = oracle.schedule(cfg, cl, np.arange(150), cl.now_ns)
    assert (ref_n >= 0).all() and len(set(ref_n)) == 43   # many pods re-read a row an earlier call committed
    nodes, scores = _sequential(cfg, cl, 150)
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)


def test_numa_sequential_cycle_equals_oracle():
    cl = make_numa_edge_cluster(700, 200, seed=21)
    cfg = numa_config(weight_numa=2)
    prow = engine.build_pod_rows(cfg, cl, np.arange(200))
    before = engine.build_node_rows(cfg, cl)
    assert not (prow["flags"] & nat.POD_NUMA_CPU_BIND).any() and not before["node_cpu_bind"].any()
    ref_n, ref_s = oracle.schedule(cfg, cl, np.arange(200), cl.now_ns)
    # the unplaced pods run key = 0 between successful calls: the reset of key and ticket
    assert (ref_n >= 0).sum() == 187 and set(ref_n[ref_n >= 0] // 256) == {0, 1, 2}
    nodes, scores = _sequential(cfg, cl, 200)
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)
    after = before.copy()
    for p, n in enumerate(nodes):
        if n >= 0:
            engine.row_commit(cfg, after[n:n + 1], prow[p:p + 1])
    assert (after["zone_allocated"] != before["zone_allocated"]).any()   # (_sequential compared the rows)


def test_ties_and_shard():
    cfg, cl, rows, pods = cc.case("shipped")
    pick = None
    for j in range(cc.N_NODES):   # a (node row, pod) pair that is feasible
        m, _, _, _ = cc.rows_totals(cfg, rows[j:j + 1], pods[0], cl.now_ns)
        if m[0] and j not in cc.BIG:
            pick = j
            break
    assert pick is not None
    same = np.repeat(rows[pick:pick + 1], cc.N_NODES)
    with _loaded(cfg, same) as eng:
        assert eng.cycle_one(pods[0], cl.now_ns, commit=False)["node"] == 0
        eng.set_shard(1024, cc.N_NODES)
        assert eng.cycle_one(pods[0], cl.now_ns, commit=False)["node"] == 1024
        eng.set_shard(0, cc.N_NODES)
        first = eng.cycle_one(pods[0], cl.now_ns, commit=True)
        assert first["node"] == 0 and first["committed"]
        engine.row_commit(cfg, same[0:1], pods[0:1])
        nxt = eng.cycle_one(pods[1], cl.now_ns, commit=False)
        _, _, _, tot = cc.rows_totals(cfg, same, pods[1], cl.now_ns)
        assert nxt["key"] == cc.key_of(tot)
        np.testing.assert_array_equal(eng.download(), same)


def test_no_feasible_node():
    cfg, cl, rows, pods = cc.case("shipped")
    big = pods[0:1].copy()
    big["request"][0, nat.RES_CPU] = 10**9          # a million cores: larger than every node
    big["flags"] |= np.uint32(nat.POD_HAS_REQUEST)
    big["request_present"] |= np.uint32(1 << nat.RES_CPU)
    with _loaded(cfg, rows) as eng:
        gen = eng.generation()
        res = eng.cycle_one(big, cl.now_ns, commit=True, planes=True)
        assert (res["node"], res["key"], res["score"], res["committed"]) == (-1, 0, -1, False)
        assert not res["mask"].any()
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), rows)
        nxt = eng.cycle_one(pods[1], cl.now_ns, commit=False)
        assert nxt["key"] == cc.key_of(cc.oracle_matrix("shipped")[3][1]) != 0


def test_batch_untouched():
    cfg, cl, rows, pods = cc.case("shipped")
    ref_n, ref_s = oracle.schedule(cfg, cl, np.arange(8), cl.now_ns)
    ninth = pods[8]

    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)

    with _loaded(cfg, rows) as eng:
        eng.set_pods(pods[:8])
        first = eng.eval(cl.now_ns)
        assert eng.cycle_one(ninth, cl.now_ns, commit=False)["node"] >= 0
        same(eng.eval(cl.now_ns), first)
        n, s = eng.place(cl.now_ns)
        np.testing.assert_array_equal(n, ref_n)
        np.testing.assert_array_equal(s, ref_s)
    # with the commit, on a copy of the snapshot: the batch still answers, now for the snapshot the commit left
    with _loaded(cfg, rows) as eng:
        eng.set_pods(pods[:8])
        same(eng.eval(cl.now_ns), first)
        res = eng.cycle_one(ninth, cl.now_ns, commit=True)
        assert res["committed"]
        got = eng.eval(cl.now_ns)
        moved = rows.copy()
        engine.row_commit(cfg, moved[res["node"]:res["node"] + 1], pods[8:9])
        with _loaded(cfg, moved) as fresh:
            fresh.set_pods(pods[:8])
            same(got, fresh.eval(cl.now_ns))


def _refused(eng, pod, now_ns):
    gen, before = eng.generation(), eng.download()
    for commit in (False, True):
        with pytest.raises(engine.EngineError, match="status -3"):
            eng.cycle_one(pod, now_ns, commit=commit)
    assert eng.generation() == gen
    np.testing.assert_array_equal(eng.download(), before)


def _three_calls(eng, pod, now_ns):
    eng.set_pods(pod)
    node, _ = engine.decode_top1(eng.eval(now_ns, mask=False, scores=False)["top1"])
    assert node[0] >= 0 and eng.commit(0, int(node[0]))


def test_refuses_reservation_slots():
    cl = synth.make_rsv_cluster(300, 8, seed=7)
    cfg = shipped_profile(plugins=("NodeResourcesFit", "LoadAwareScheduling", "Reservation"))
    pods = engine.build_pod_rows(cfg, cl, np.arange(8))
    with _loaded(cfg, engine.build_node_rows(cfg, cl)) as eng:
        pod = pods[(pods["rsv_affinity_class"] < 0).argmax()][None]
        assert eng.cycle_one(pod, cl.now_ns, commit=False)["node"] >= 0   # no slots loaded yet: answered
        eng.set_reservations(cl.rsv_arr)
        assert len(cl.rsv_arr) > 0
        _refused(eng, pod, cl.now_ns)
        _three_calls(eng, pod, cl.now_ns)


def test_refuses_elastic_quota():
    cl = synth.make_rsv_cluster(300, 8, seed=7)
    cfg = shipped_profile(plugins=("NodeResourcesFit", "LoadAwareScheduling", "ElasticQuota"))
    pods = engine.build_pod_rows(cfg, cl, np.arange(8))
    with _loaded(cfg, engine.build_node_rows(cfg, cl)) as eng:
        eng.set_quotas(cl.quota_arr)
        _refused(eng, pods[0:1], cl.now_ns)
        eng.set_pods(pods[0:1])
        assert eng.eval(cl.now_ns, mask=False, scores=False)["top1"].shape == (1,)   # the three-call path answers


def test_refuses_cpuset_pod():
    cl = synth.make_numa_cluster(100, 4, seed=5)
    cfg = numa_config()
    pods = engine.build_pod_rows(cfg, cl, np.arange(4))
    with _loaded(cfg, engine.build_node_rows(cfg, cl)) as eng:
        assert eng.cycle_one(pods[1], cl.now_ns, commit=False)["key"] >= 0   # the plain pod: answered
        bind = pods[1:2].copy()
        bind["flags"] |= np.uint32(nat.POD_NUMA_CPU_BIND)
        bind["flags"] &= ~np.uint32(nat.POD_NUMA_SKIP)
        _refused(eng, bind, cl.now_ns)
