"""kg_unreserve on the device: after a batched rollback the snapshot rows equal the host model (engine.row_commit per
placement, engine.row_unreserve per release) byte for byte, and every derived plane equals a fresh twin engine loaded
from the model — a second batch's eval (mask, both score planes, top1) and its placement are the twin's, bit for bit.
N = 2100 nodes (two full tiles and a ragged third), batches of 64 to 256 pods."""
import numpy as np
import pytest

import churn_cases as ch
import unreserve_cases as uc
from koordinator_amd import _native as nat
from koordinator_amd import engine

pytestmark = pytest.mark.gpu

NOW = uc.NOW


def _twin_eval(cfg, rows, pods, rsv=None, quotas=None):
    with uc.make_engine(cfg, rows, rsv, quotas) as twin:
        twin.set_pods(pods)
        return twin.eval(NOW)


@pytest.mark.parametrize("extra", [False, True], ids=["shipped", "la_extra"])
def test_fit_loadaware_rollback_equals_model_and_twin(extra):
    r = uc.fit_la_rollback(extra)
    nodes, pick = r["nodes"], r["pick"]
    assert r["released"].all() and len(pick) > 40
    assert (nodes[pick] == r["busiest"]).sum() >= 2, "one node has repeated entries"
    assert r["rows"].tobytes() == r["model_rows"].tobytes()
    uc.same_eval(r["eval"], r["ref_eval"], "second batch after the rollback")
    np.testing.assert_array_equal(r["place"][0], r["ref_place"][0])
    np.testing.assert_array_equal(r["place"][1], r["ref_place"][1])
    assert r["generations"][1] == r["generations"][0] + 1
    assert (r["place"][0] >= 0).any()


def test_transition_rows_on_the_device():
    """A node that is PODS_FULL / over-cpu / outside the fp64 bounds only while the pod is on it: after the release
    the rows are the originals and the planes a fresh twin's (the KGD_SLOW node is back on the fast path)."""
    cfg, cases = uc.transition_rows()
    _, rows0, _, second = uc.fit_la_cluster()
    rows = rows0.copy()
    at = {"pods_full": 5, "over_cpu": 1024, "val_limit": N - 1}
    pod = cases["pods_full"][1]
    for name, j in at.items():
        rows[j] = cases[name][0]
    with uc.make_engine(cfg, rows) as eng:
        eng.set_pods(pod)
        for j in at.values():
            assert eng.commit(0, j)
        held = eng.download()
        for name, j in at.items():
            assert uc.TRANSITION_FLAG[name](cfg, held[j]) and not uc.TRANSITION_FLAG[name](cfg, rows[j])
        probe = np.concatenate([pod, second])
        eng.set_pods(probe)
        busy = eng.eval(NOW)
        g0 = eng.generation()
        rel = eng.unreserve(np.concatenate([pod] * 3), list(at.values()))
        assert rel.all() and eng.generation() == g0 + 1
        assert eng.download().tobytes() == rows.tobytes()
        got = eng.eval(NOW)
    ref = _twin_eval(cfg, rows, probe)
    uc.same_eval(got, ref, "after the release")
    m_busy, m_free = engine.unpack_mask(busy["mask"], N), engine.unpack_mask(got["mask"], N)
    assert not m_busy[:, at["pods_full"]].any() and not m_busy[:, at["over_cpu"]].any()
    assert m_free[0, at["pods_full"]], "the node takes the pod again"


N = ch.N


def test_numa_rollback_equals_model_and_twin():
    cfg, rows, first, second = uc.numa_cluster()
    model = uc.Model(cfg, rows)
    with uc.make_engine(cfg, rows) as eng:
        nodes, recs = uc.place_on_both(eng, model, first)
        assert eng.download().tobytes() == model.rows.tobytes()
        pick, _ = uc.release_choice(nodes)
        assert sum(recs[i][0].any() for i in pick) >= 5, "releases with a zone record"
        rel = uc.roll_back(eng, model, first, nodes, pick, recs)
        assert rel.all()
        assert eng.download().tobytes() == model.rows.tobytes()
        eng.set_pods(second)
        got = eng.eval(NOW)
    uc.same_eval(got, _twin_eval(cfg, model.rows, second), "NodeNUMAResource: second batch after the rollback")


def test_reservation_and_quota_rollback():
    r = uc.rsv_quota_rollback()
    nodes, pick, recs, model = r["nodes"], r["pick"], r["recs"], r["model"]
    assert r["released"].all()
    assert sum(recs[i][1] >= 0 for i in pick) >= 5, "releases that hand a slot back"
    # the model replays the engine's own Reserves (slots from row_eval_rsv): they agree before the rollback
    np.testing.assert_array_equal(r["placed_rsv"], r["mid"].rsv)
    np.testing.assert_array_equal(r["placed_quotas"], r["mid"].quotas)
    assert r["got"]["rows"].tobytes() == model.rows.tobytes()
    np.testing.assert_array_equal(r["got"]["rsv"], model.rsv)
    np.testing.assert_array_equal(r["got"]["quotas"], model.quotas)
    assert (r["got"]["quotas"]["used"]["v"] != r["placed_quotas"]["used"]["v"]).any()
    inner = np.flatnonzero(np.isin(np.arange(len(model.quotas)), model.quotas["parent"]))
    assert (r["got"]["quotas"]["used"]["v"][inner] != r["placed_quotas"]["used"]["v"][inner]).any(), "ancestors too"
    np.testing.assert_array_equal(r["place"][0], r["ref_place"][0])
    np.testing.assert_array_equal(r["place"][1], r["ref_place"][1])


def test_refused_entries_leave_their_nodes_alone():
    cfg, rows, first, second, rsv, quotas = uc.rsv_quota_cluster()
    model = uc.Model(cfg, rows, rsv, quotas)
    with uc.make_engine(cfg, rows, rsv, quotas) as eng:
        nodes, recs = uc.place_on_both(eng, model, first)
        placed = np.flatnonzero(nodes >= 0)
        with_slot = [i for i in placed if recs[i][1] >= 0]
        plain = [i for i in placed if recs[i][1] < 0]
        gone_i = plain[0]
        short_i = next(i for i in plain if nodes[i] != nodes[gone_i])
        wrong_i = next(i for i in with_slot if nodes[i] not in (nodes[gone_i], nodes[short_i]))
        used = {int(nodes[i]) for i in (gone_i, short_i, wrong_i)}
        good = [i for i in placed if int(nodes[i]) not in used][:40]
        # a removed node; a node asked for more pods than it holds; a slot that lives on another node
        eng.remove(int(nodes[gone_i]))
        model.rows[nodes[gone_i]] = np.zeros((), nat.NODE_ROW)
        short_node = int(nodes[short_i])
        row = model.rows[short_node:short_node + 1].copy()
        row["pod_count"] = 1
        eng.upsert([short_node], row)
        model.rows[short_node] = row[0]
        other = next(k for k in range(len(rsv)) if int(rsv["node"][k]) != int(nodes[wrong_i]))
        idx = [gone_i, short_i, short_i, wrong_i] + good
        slots = [-1, -1, -1, other] + [recs[i][1] for i in good]
        before = eng.download()
        rsv_before, q_before = eng.download_reservations(), eng.download_quotas()
        g0 = eng.generation()
        rel = eng.unreserve(first[idx], nodes[idx], rsv_slot=slots)
        np.testing.assert_array_equal(rel, [False] * 4 + [True] * len(good))
        for i in good:
            model.release(first[i:i + 1], nodes[i], None, recs[i][1])
        after = eng.download()
        for j in used:
            assert after[j].tobytes() == before[j].tobytes()
        # the refused entries touched no slot and no quota group either: the rest equals the model
        assert after.tobytes() == model.rows.tobytes()
        want_rsv, want_q = rsv_before.copy(), q_before.copy()
        for i in good:
            if recs[i][1] >= 0:
                uc.restate_rsv(want_rsv[recs[i][1]], first[i], -1)
            if int(first["quota"][i]) >= 0:
                uc.restate_quota(want_q, first[i], -1)
        np.testing.assert_array_equal(eng.download_reservations(), want_rsv)
        np.testing.assert_array_equal(eng.download_quotas(), want_q)
        assert eng.generation() == g0 + 1
        # nothing released: the generation stays
        rel = eng.unreserve(first[[gone_i]], nodes[[gone_i]])
        assert not rel.any() and eng.generation() == g0 + 1


def test_shard_is_ignored():
    cfg, rows, first, _ = uc.fit_la_cluster()
    model = uc.Model(cfg, rows)
    with uc.make_engine(cfg, rows) as eng:
        nodes, recs = uc.place_on_both(eng, model, first[:64])
        eng.set_shard(1024, 2048)
        outside = [i for i in np.flatnonzero(nodes >= 0) if not 1024 <= nodes[i] < 2048][:8]
        assert outside
        rel = eng.unreserve(first[outside], nodes[outside])
        for i in outside:
            model.release(first[i:i + 1], nodes[i])
        assert rel.all() and eng.download().tobytes() == model.rows.tobytes()


def _raises(status, fn, eng, rows):
    g = eng.generation()
    with pytest.raises(engine.EngineError, match=r"status %d\b" % status):
        fn()
    assert eng.generation() == g and eng.download().tobytes() == rows.tobytes()


def test_errors_change_nothing():
    INVALID, UNSUPPORTED, RANGE, STATE = -1, -3, -4, -5
    cfg, rows, first, _ = uc.fit_la_cluster()
    L = nat.lib()
    pod, node, out = first[:1].copy(), np.array([7], np.int32), np.zeros(1, np.uint8)
    zeros = np.zeros((1, nat.MAX_ZONES, 2), np.int64)
    with engine.Engine(cfg) as eng:
        with pytest.raises(engine.EngineError, match=r"status %d\b" % STATE):
            eng.unreserve(pod, node)                                             # no snapshot
        eng.load_snapshot(rows)
        held = eng.download()
        g = eng.generation()
        assert len(eng.unreserve(first[:0], [])) == 0 and eng.generation() == g                # n = 0: a no-op
        for args, status in (((nat.ptr(pod), nat.ptr(node), -1, 0, None, None, nat.ptr(out)), INVALID),
                             ((None, nat.ptr(node), 1, 0, None, None, nat.ptr(out)), INVALID),
                             ((nat.ptr(pod), None, 1, 0, None, None, nat.ptr(out)), INVALID),
                             ((nat.ptr(pod), nat.ptr(node), 1, 0, None, None, None), INVALID),
                             ((nat.ptr(pod), nat.ptr(node), 1, 1, None, None, nat.ptr(out)), INVALID)):
            assert L.kg_unreserve(eng._h, *args) == status
        assert eng.generation() == g and eng.download().tobytes() == held.tobytes()
        _raises(INVALID, lambda: eng.unreserve(pod, node, zone_release=zeros), eng, held)   # NodeNUMAResource disabled
        big = np.repeat(pod, nat.UNRESERVE_MAX + 1)
        _raises(RANGE, lambda: eng.unreserve(big, np.zeros(len(big), np.int32)), eng, held)
        _raises(RANGE, lambda: eng.unreserve(pod, [N]), eng, held)
        _raises(RANGE, lambda: eng.unreserve(pod, [-1]), eng, held)
        wide = pod.copy()
        wide["request"][0, 0] = ch.VAL_LIMIT
        _raises(RANGE, lambda: eng.unreserve(wide, node), eng, held)
        _raises(STATE, lambda: eng.unreserve(pod, node, rsv_slot=[0]), eng, held)           # no slots loaded
    cfg5, rows5, first5, _, rsv, quotas = uc.rsv_quota_cluster()
    one = quotas[:1].copy()
    one["parent"] = -1
    with uc.make_engine(cfg5, rows5, rsv, one) as eng:
        held = eng.download()
        p = first5[:1].copy()
        _raises(RANGE, lambda: eng.unreserve(p, node, rsv_slot=[len(rsv)]), eng, held)
        p["quota"] = 5
        _raises(STATE, lambda: eng.unreserve(p, node), eng, held)                           # a quota index without a group
    ncfg, nrows, nfirst, _ = uc.numa_cluster()
    with uc.make_engine(ncfg, nrows) as eng:
        held = eng.download()
        j = int(np.flatnonzero((nrows["n_zones"] >= 1) & (nrows["n_zones"] < nat.MAX_ZONES))[0])
        neg, past = zeros.copy(), zeros.copy()
        neg[0, 0, 0] = -5
        past[0, int(nrows["n_zones"][j]), 1] = 3
        _raises(INVALID, lambda: eng.unreserve(nfirst[:1], [j], zone_release=neg), eng, held)
        _raises(INVALID, lambda: eng.unreserve(nfirst[:1], [j], zone_release=past), eng, held)
        bind = nfirst[:1].copy()
        bind["flags"] |= nat.POD_NUMA_CPU_BIND
        bind["flags"] &= ~np.uint32(nat.POD_NUMA_SKIP)
        _raises(UNSUPPORTED, lambda: eng.unreserve(bind, [j]), eng, held)                   # a cpuset pod
        row = nrows[j:j + 1].copy()
        row["node_cpu_bind"] = nat.NODE_CPU_BIND_FULL_PCPUS_ONLY
        row["cpus_per_core"] = 2
        row["flags"] |= nat.NODE_NUMA_OPTIONS
        eng.upsert([j], row)
        held = eng.download()
        _raises(UNSUPPORTED, lambda: eng.unreserve(nfirst[:1], [j + 1]), eng, held)         # a node with a CPU bind policy


def test_max_batch_over_many_nodes():
    """n = KG_UNRESERVE_MAX tiny pods over 300 distinct nodes (more than 256 workgroups), 13 or 14 entries each."""
    cfg, rows0, first, second = uc.fit_la_cluster()
    n, k = nat.UNRESERVE_MAX, 300
    tiny = first[:1].copy()
    tiny["request"][:] = 0
    tiny["request"][0, uc.CPU], tiny["request"][0, uc.MEM] = 1, 1 << 20
    tiny["fit_score_request"][0, :] = tiny["request"][0, :]
    tiny["nonzero_request"][0] = (1, 1 << 20)
    tiny["la_estimate"][0] = (1, 1 << 20)
    valid = np.flatnonzero((rows0["flags"] & nat.NODE_VALID) != 0)
    where = valid[np.linspace(0, len(valid) - 1, k).astype(int)]
    nodes = where[np.arange(n) % k].astype(np.int32)
    base = rows0.copy()
    base["allowed_pods"][where] = 200
    base["pod_count"][where] = 40
    rows = base.copy()
    pods = np.repeat(tiny, n)
    for i in range(n):
        engine.row_commit(cfg, rows[nodes[i]:nodes[i] + 1], pods[i:i + 1])
    with uc.make_engine(cfg, rows) as eng:
        rel = eng.unreserve(pods, nodes)
        assert rel.all()
        assert eng.download().tobytes() == base.tobytes()
        eng.set_pods(second)
        got = eng.eval(NOW)
    uc.same_eval(got, _twin_eval(cfg, base, second), "after the largest batch")
