"""kg_preempt (Engine.preempt) and the bound-pod table against tests/preempt_ref.py on the cases of
tests/preempt_cases.py: the seeded 1,100-node cluster (a full tile and a ragged one, lists of 0..128 pods, four quota
groups) and the hand-written pick cases."""
import numpy as np
import pytest

import preempt_cases as pc
import preempt_ref as pr
import why_cases as wc
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import make_config

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_RANGE, ERR_STATE = -1, -3, -4, -5
BOUND_FIELDS = ("request", "request_present", "nonzero_request", "numa_request", "numa_request_present", "quota")


def raises(status, fn, *a, **kw):
    with pytest.raises(engine.EngineError) as ei:
        fn(*a, **kw)
    assert f"status {status}:" in str(ei.value), str(ei.value)


def check(res, ref, lo=0, hi=None):
    """A preempt() result against per-preemptor reference results over the nodes [lo, hi)."""
    pick, cells, _ = pc.ref_arrays(ref, lo, hi)
    np.testing.assert_array_equal(res["pick"], pick)
    np.testing.assert_array_equal(res["node"], pick[:, 0])
    np.testing.assert_array_equal(res["n_candidates"], pick[:, 7])
    if "plane" in res:
        np.testing.assert_array_equal(res["plane"][:, :cells.shape[1]], cells)
        np.testing.assert_array_equal(res["status"][:, :cells.shape[1]], cells & 0xFF)
        np.testing.assert_array_equal(res["n_potential"][:, :cells.shape[1]], cells >> 16)
    for i in range(len(ref)):
        want = [] if pick[i, 0] < 0 else sorted(v.pos for v in ref[i][int(pick[i, 0])].victims)
        assert np.flatnonzero(res["victims"][i]).tolist() == want


def same_bound(got, rows, prio, start):
    g_rows, g_prio, g_start = got
    assert len(g_rows) == len(rows)
    for f in BOUND_FIELDS:
        np.testing.assert_array_equal(g_rows[f], rows[f], err_msg=f)
    np.testing.assert_array_equal(g_rows["flags"], rows["flags"] & nat.POD_NON_PREEMPTIBLE)
    np.testing.assert_array_equal(g_prio, prio)
    np.testing.assert_array_equal(g_start, start)


def test_parity_seeded():
    c = pc.seeded()
    ref = pc.reference("seeded")
    with pc.engine_of(c) as eng:
        got = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        check(got, ref)
        check(eng.preempt(c.pods, c.pod_prio, c.now_ns), ref)   # picks alone: the form without the plane
        again = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)   # identical from run to run
        np.testing.assert_array_equal(again["pick"], got["pick"])
        np.testing.assert_array_equal(again["plane"][:, :len(c.rows)], got["plane"][:, :len(c.rows)])


@pytest.mark.parametrize("name", [h.name for h in pc.hand_cases()])
def test_parity_hand(name):
    c = next(h for h in pc.hand_cases() if h.name == name)
    with pc.engine_of(c) as eng:
        got = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        check(got, pc.reference(name))
        assert int(got["node"][0]) == c.want_node


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 1_023, 1_024, 1_025])
def test_grid_edges_nodes(n_nodes):
    c = pc.seeded()
    ref = pc.reference("seeded")[:9]
    with pc.engine_of(c, n_nodes) as eng:
        check(eng.preempt(c.pods[:9], c.pod_prio[:9], c.now_ns, plane=True), ref, 0, n_nodes)


@pytest.mark.parametrize("n_pods", [1, 9, 64])
def test_grid_edges_pods(n_pods):
    c = pc.seeded()
    idx = np.arange(n_pods) % len(c.pods)
    full = pc.reference("seeded")
    with pc.engine_of(c) as eng:
        check(eng.preempt(c.pods[idx], c.pod_prio[idx], c.now_ns, plane=True), [full[i] for i in idx])


def test_eligibility():
    c = pc.seeded()
    pods = pc.elig_pods(c)
    ref = pc.reference("seeded", elig=True)
    plain = pc.ref_arrays(pc.reference("seeded"))[1]
    assert (pc.ref_arrays(ref)[1] != plain).any()   # the classes change verdicts
    with pc.engine_of(c) as eng:
        raises(ERR_RANGE, eng.preempt, pods, c.pod_prio, c.now_ns)   # no class loaded yet
        eng.set_eligibility(wc.elig_classes(len(c.rows)))
        check(eng.preempt(pods, c.pod_prio, c.now_ns, plane=True), ref)


def test_shards():
    c = pc.seeded()
    n = len(c.rows)
    ref = pc.reference("seeded")
    with pc.engine_of(c) as eng:
        whole = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        parts = []
        for lo, hi in ((0, 1_024), (1_024, n)):
            eng.set_shard(lo, hi)
            part = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
            check(part, ref, lo, hi)
            np.testing.assert_array_equal(part["plane"][:, :hi - lo], whole["plane"][:, lo:hi])
            parts.append(part)
        np.testing.assert_array_equal(engine.merge_preempt(parts)["pick"], whole["pick"])
        np.testing.assert_array_equal(engine.merge_preempt(parts[::-1])["pick"], whole["pick"])
        eng.set_shard(1_024, 1_024)   # an empty shard: no candidate, no plane column
        before = eng.counters()
        empty = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        assert (empty["node"] == -1).all() and not empty["pick"][:, 1:].any() and empty["plane"].shape == (len(c.pods), 0)
        after = eng.counters()
        assert (after["eval_calls"], after["evals"]) == (before["eval_calls"] + 1, before["evals"])
        np.testing.assert_array_equal(engine.merge_preempt(parts + [empty])["pick"], whole["pick"])


def test_bound_update_and_download():
    c = pc.seeded()
    first = c.first
    grow, shrink, clear = 11, 16, 1031   # 1 -> 70 pods, 128 -> 3, 128 -> none
    donor = slice(int(first[1099]), int(first[1099]) + 70)
    new = {grow: (c.b_rows[donor], c.b_prio[donor], c.b_start[donor]),
           shrink: tuple(a[int(first[shrink]) + 60:int(first[shrink]) + 63] for a in (c.b_rows, c.b_prio, c.b_start)),
           clear: tuple(a[:0] for a in (c.b_rows, c.b_prio, c.b_start))}
    lists = [tuple(a[int(first[j]):int(first[j + 1])] for a in (c.b_rows, c.b_prio, c.b_start)) for j in range(len(c.rows))]
    for j, l in new.items():
        lists[j] = l
    f2 = np.zeros_like(first)
    f2[1:] = np.cumsum([len(l[0]) for l in lists])
    final = with_table(c, f2, *(np.concatenate([l[k] for l in lists]) for k in range(3)))
    pods, prio = c.pods[:12], c.pod_prio[:12]
    with pc.engine_of(c) as eng, pc.engine_of(final) as fresh:
        for j in (0, 12, 13, 14, 16, 1099):   # the round trip, in the caller's order
            same_bound(eng.download_bound_pods(j), *lists_of(c, j))
        gen, ctr = eng.generation(), eng.counters()
        for j, l in new.items():
            eng.update_bound_pods(j, *l)
        assert eng.generation() == gen and eng.counters()["h2d_bytes"] > ctr["h2d_bytes"]
        for j in new:
            same_bound(eng.download_bound_pods(j), *lists[j])
        same_bound(eng.download_bound_pods(12), *lists_of(c, 12))   # a neighbour is untouched
        got, want = eng.preempt(pods, prio, c.now_ns, plane=True), fresh.preempt(pods, prio, c.now_ns, plane=True)
        np.testing.assert_array_equal(got["pick"], want["pick"])
        np.testing.assert_array_equal(got["plane"][:, :len(c.rows)], want["plane"][:, :len(c.rows)])
        # and both equal the reference on the final table
        ref = [pr.dry_run(final.cfg, final.ref_rows, final.first, final.b_rows, final.b_prio, final.b_start, pods[i], int(prio[i]),
                          final.quotas, final.now_ns) for i in range(4)]
        assert any(ref[i][j].status != pc.reference("seeded")[i][j].status for i in range(4) for j in new)
        check({k: v[:4] for k, v in got.items()}, ref)
        # errors change nothing
        raises(ERR_RANGE, eng.update_bound_pods, len(c.rows), *new[shrink])
        raises(ERR_RANGE, eng.update_bound_pods, -1, *new[shrink])
        raises(ERR_RANGE, eng.download_bound_pods, len(c.rows))
        same_bound(eng.download_bound_pods(shrink), *lists[shrink])
    with pc.engine_of(c, table=False) as eng:
        raises(ERR_STATE, eng.update_bound_pods, 0, *new[shrink])
        raises(ERR_STATE, eng.download_bound_pods, 0)
        small = (np.array([0] + [2] * len(c.rows), np.int32), c.b_rows[:2], c.b_prio[:2], c.b_start[:2])
        raises(ERR_RANGE, eng.set_bound_pods, *small, 1)      # a list longer than max_per_node
        raises(ERR_RANGE, eng.set_bound_pods, *small, 129)
        bad = small[0].copy()
        bad[3] = 1
        raises(ERR_RANGE, eng.set_bound_pods, bad, *small[1:], 4)   # offsets that do not rise
        raises(ERR_STATE, eng.preempt, c.pods[:1], c.pod_prio[:1], c.now_ns)   # still no table
        eng.set_bound_pods(*small, 2)
        raises(ERR_RANGE, eng.update_bound_pods, 0, c.b_rows[:3], c.b_prio[:3], c.b_start[:3])   # above the stride kept
        eng.load_snapshot(c.rows)   # kg_snapshot_reset drops the table
        raises(ERR_STATE, eng.download_bound_pods, 0)
    with engine.Engine(c.cfg) as eng:   # no snapshot
        raises(ERR_STATE, eng.set_bound_pods, np.zeros(1, np.int32), c.b_rows[:0], c.b_prio[:0], c.b_start[:0], 4)


def lists_of(c, j):
    lo, hi = int(c.first[j]), int(c.first[j + 1])
    return c.b_rows[lo:hi], c.b_prio[lo:hi], c.b_start[lo:hi]


def with_table(c, first, b_rows, b_prio, b_start):
    """The case with another bound-pod table."""
    from types import SimpleNamespace
    d = dict(vars(c))
    d.update(first=first, b_rows=b_rows, b_prio=b_prio, b_start=b_start)
    return SimpleNamespace(**d)


def test_purity():
    c = pc.seeded()
    with pc.engine_of(c) as eng:
        eng.set_pods(c.pods[:16])
        out0 = eng.eval(c.now_ns)
        gen, rows0, q0, ctr0 = eng.generation(), eng.download(), eng.download_quotas(), eng.counters()
        tab0 = [eng.download_bound_pods(j) for j in (0, 13, 16, 1031)]
        res = eng.preempt(c.pods[20:30], c.pod_prio[20:30], c.now_ns, plane=True)
        ctr1 = eng.counters()
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), rows0)
        np.testing.assert_array_equal(eng.download_quotas(), q0)
        for j, t in zip((0, 13, 16, 1031), tab0):
            same_bound(eng.download_bound_pods(j), *t)
        assert (ctr1["placed"], ctr1["resolved"]) == (ctr0["placed"], ctr0["resolved"])
        assert ctr1["eval_calls"] == ctr0["eval_calls"] + 1
        assert ctr1["evals"] == ctr0["evals"] + 10 * len(c.rows)
        assert ctr1["out_bytes"] == ctr0["out_bytes"] + res["pick"].nbytes + res["plane"].nbytes
        assert ctr1["h2d_bytes"] > ctr0["h2d_bytes"]
        out1 = eng.eval(c.now_ns)   # the uploaded batch is still the first 16 pods
        assert out0.keys() == out1.keys()
        for k in out0:
            np.testing.assert_array_equal(out0[k], out1[k], err_msg=k)
        check(res, pc.reference("seeded")[20:30])


def test_quota_state_is_read_from_the_device():
    """The re-check reads the group's `used` as the engine holds it: after kg_quota_set with another state the verdicts
    follow it."""
    c = pc.seeded()
    q = c.quotas.copy()
    q[pc.GROUP_OVER]["used"]["v"][nat.RES_CPU] = 0   # the group is under its limit now
    pods, prio = c.pods[:10], c.pod_prio[:10]
    ref = [pr.dry_run(c.cfg, c.ref_rows, c.first, c.b_rows, c.b_prio, c.b_start, pods[i], int(prio[i]), q, c.now_ns)
           for i in range(len(pods))]
    assert (pc.ref_arrays(ref)[1] != pc.ref_arrays(pc.reference("seeded")[:10])[1]).any()
    with pc.engine_of(c) as eng:
        eng.set_quotas(q)
        check(eng.preempt(pods, prio, c.now_ns, plane=True), ref)


def test_argument_errors_launch_nothing():
    c = pc.seeded()
    L = nat.lib()
    with pc.engine_of(c) as eng:
        before = eng.counters()
        idx = np.arange(65) % len(c.pods)
        raises(ERR_RANGE, eng.preempt, c.pods[idx], c.pod_prio[idx], c.now_ns)
        bad = c.pods[:2].copy()
        bad["elig_class"][1] = 1
        raises(ERR_RANGE, eng.preempt, bad, c.pod_prio[:2], c.now_ns)
        bad = c.pods[:2].copy()
        bad["request"][0, nat.RES_CPU] = -1
        raises(ERR_RANGE, eng.preempt, bad, c.pod_prio[:2], c.now_ns)
        bad = c.pods[:2].copy()
        bad["quota"][1] = len(c.quotas)   # a quota index without its group
        raises(ERR_STATE, eng.preempt, bad, c.pod_prio[:2], c.now_ns)
        pick = np.zeros((1, 8), np.int64)
        prio = np.ascontiguousarray(c.pod_prio[:1])
        pod = np.ascontiguousarray(c.pods[:1])
        args = (nat.ptr(pod), nat.ptr(prio), 1, int(c.now_ns))
        assert L.kg_preempt(eng._h, *args, 0x1, nat.ptr(pick), None, 0) == ERR_INVALID_ARG
        assert L.kg_preempt(eng._h, *args, 0, None, None, 0) == ERR_INVALID_ARG
        assert L.kg_preempt(eng._h, None, nat.ptr(prio), 1, int(c.now_ns), 0, nat.ptr(pick), None, 0) == ERR_INVALID_ARG
        assert L.kg_preempt(eng._h, nat.ptr(pod), None, 1, int(c.now_ns), 0, nat.ptr(pick), None, 0) == ERR_INVALID_ARG
        assert L.kg_preempt(eng._h, nat.ptr(pod), nat.ptr(prio), -1, int(c.now_ns), 0, nat.ptr(pick), None, 0) == ERR_INVALID_ARG
        assert eng.counters() == before
        assert L.kg_preempt(eng._h, None, None, 0, int(c.now_ns), 0, None, None, 0) == 0   # n = 0: a no-op
        assert eng.counters() == before
    with engine.Engine(c.cfg) as eng:   # no snapshot
        raises(ERR_STATE, eng.preempt, c.pods[:1], c.pod_prio[:1], c.now_ns)


def test_refusals_launch_nothing():
    import cycle_cases as cc
    cl = cc.cluster()
    # reservation slots loaded
    cfg = make_config(plugins=("NodeResourcesFit", "LoadAwareScheduling", "Reservation"))
    rows, pods = engine.build_node_rows(cfg, cl), engine.build_pod_rows(cfg, cl, np.arange(4))
    prio = np.full(4, 100, np.int32)
    first = np.zeros(len(rows) + 1, np.int32)
    first[1:] = 1
    bound = (first, np.array([pc.bound_row(100, 1 << 20)]), np.zeros(1, np.int32), np.zeros(1, np.int64))
    rsv = np.zeros(1, dtype=nat.RESERVATION)
    rsv["node"], rsv["flags"], rsv["owner_classes"] = 0, nat.RSV_AVAILABLE, 1
    rsv["allocatable"]["v"][0, nat.RES_CPU], rsv["allocatable"]["present"] = 1000, 1 << nat.RES_CPU
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(rows)
        eng.set_bound_pods(*bound, 4)
        got = eng.preempt(pods, prio, cl.now_ns)   # Reservation enabled, no slots: answered
        assert (got["n_candidates"] <= 1).all()
        eng.set_reservations(rsv)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.preempt, pods, prio, cl.now_ns)
        assert eng.counters() == before
    # NodeNUMAResource enabled
    c = wc.case("numa")
    with wc.engine_of(c) as eng:
        f = np.zeros(len(c.rows) + 1, np.int32)
        eng.set_bound_pods(f, bound[1][:0], bound[2][:0], bound[3][:0], 4)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.preempt, c.pods[:3], np.zeros(3, np.int32), c.now_ns)
        assert eng.counters() == before
