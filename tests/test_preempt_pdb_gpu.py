"""kg_preempt with a PDB threshold plane loaded (kg_bound_pdb_set / _update / _download) against
tests/preempt_pdb_ref.py on the cases of tests/preempt_pdb_cases.py: the seeded 1,100-node cluster under 6 PDBs, the
hand-written 2-node cases and the 1,100-node wide cases in which n_violating decides the pick across waves, tiles and
shards.  The thresholds the engine is given come from kg_pdb_thresholds; the reference works from PDB ids
and budgets."""
import numpy as np
import pytest

import preempt_cases as pc
import preempt_pdb_cases as ppc
from koordinator_amd import _native as nat
from koordinator_amd import engine

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_RANGE, ERR_STATE = -1, -4, -5
INT32_MAX = np.iinfo(np.int32).max


def raises(status, fn, *a, **kw):
    with pytest.raises(engine.EngineError) as ei:
        fn(*a, **kw)
    assert f"status {status}:" in str(ei.value), str(ei.value)


def check(res, ref, lo=0, hi=None):
    """A preempt() result against per-preemptor reference results over the nodes [lo, hi)."""
    pick, cells, _ = ppc.ref_arrays(ref, lo, hi)
    np.testing.assert_array_equal(res["pick"], pick)
    np.testing.assert_array_equal(res["node"], pick[:, 0])
    np.testing.assert_array_equal(res["n_victims"], pick[:, 1] & 0xFFFFFFFF)
    np.testing.assert_array_equal(res["n_violating"], pick[:, 1] >> 32)
    np.testing.assert_array_equal(res["n_candidates"], pick[:, 7])
    if "plane" in res:
        w = cells.shape[1]
        np.testing.assert_array_equal(res["plane"][:, :w], cells)
        np.testing.assert_array_equal(res["status"][:, :w], cells & 0xFF)
        np.testing.assert_array_equal(res["n_victims_plane"][:, :w], (cells >> 8) & 0xFF)
        np.testing.assert_array_equal(res["n_potential"][:, :w], (cells >> 16) & 0xFF)
        np.testing.assert_array_equal(res["n_violating_plane"][:, :w], cells >> 24)
    for i in range(len(ref)):
        want = [] if pick[i, 0] < 0 else sorted(v.pos for v in ref[i][int(pick[i, 0])].victims)
        assert np.flatnonzero(res["victims"][i]).tolist() == want


@pytest.fixture(scope="module")
def seeded_engine():
    with ppc.engine_of(ppc.seeded()) as eng:
        yield eng


def test_parity_seeded(seeded_engine):
    c, eng = ppc.seeded(), seeded_engine
    ref = ppc.reference("seeded")
    got = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
    check(got, ref)
    assert (got["n_violating_plane"][:, :len(c.rows)] > 0).any()
    check(eng.preempt(c.pods, c.pod_prio, c.now_ns), ref)   # picks alone: the form without the plane
    again = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)   # identical from run to run
    np.testing.assert_array_equal(again["pick"], got["pick"])
    np.testing.assert_array_equal(again["plane"][:, :len(c.rows)], got["plane"][:, :len(c.rows)])


@pytest.mark.parametrize("name", [h.name for h in ppc.hand_cases()])
def test_parity_hand(name):
    c = ppc.case(name)
    with ppc.engine_of(c) as eng:
        got = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        check(got, ppc.reference(name))
        assert (int(got["node"][0]), int(got["n_violating"][0])) == (c.want["node"], c.want["n_violating"])
        if "hi_prio" in c.want:
            assert int(got["hi_prio"][0]) == c.want["hi_prio"]
        eng.set_bound_pdb(None, None)
        plain = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        assert not plain["n_violating"].any() and not plain["n_violating_plane"].any()
        if name in ("violating_decides", "budget_zero"):
            assert int(plain["node"][0]) == 0   # the pick the n_violating step overturns


@pytest.mark.parametrize("name", [w.name for w in ppc.wide_cases()])
def test_violating_step_across_waves_tiles_and_shards(name):
    """The 1,100-node wide cases: n_violating alone decides the pick between candidates in different waves and in
    different tiles (k_preempt's wave butterfly and LDS reduction, k_preempt_pick over two tiles), and between the
    picks of the shards [0, 1024) and [1024, 1100) (kg_preempt_merge); without the plane the pick is the other node."""
    c = ppc.case(name)
    ref = ppc.reference(name)
    n = len(c.rows)
    with ppc.engine_of(c) as eng:
        whole = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        check(whole, ref)
        check(eng.preempt(c.pods, c.pod_prio, c.now_ns), ref)
        assert (int(whole["node"][0]), int(whole["n_violating"][0])) == (c.want["node"], 0)
        assert (whole["n_violating_plane"][0, :n] > 0).sum() >= 2   # candidates the step sets aside
        parts = []
        for lo, hi in ((0, 1_024), (1_024, n)):
            eng.set_shard(lo, hi)
            part = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
            check(part, ref, lo, hi)
            parts.append(part)
        assert int(parts[0]["n_violating"][0]) != int(parts[1]["n_violating"][0])   # the merge turns on the step
        for order in (parts, parts[::-1]):
            np.testing.assert_array_equal(engine.merge_preempt(order)["pick"], whole["pick"])
        eng.set_shard(0, n)
        eng.set_bound_pdb(None, None)
        assert int(eng.preempt(c.pods, c.pod_prio, c.now_ns)["node"][0]) == c.want["plain_node"]


def test_shards(seeded_engine):
    c, eng = ppc.seeded(), seeded_engine
    n = len(c.rows)
    ref = ppc.reference("seeded")
    whole = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
    parts = []
    try:
        for lo, hi in ((0, 1_024), (1_024, n)):
            eng.set_shard(lo, hi)
            part = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
            check(part, ref, lo, hi)
            np.testing.assert_array_equal(part["plane"][:, :hi - lo], whole["plane"][:, lo:hi])
            parts.append(part)
    finally:
        eng.set_shard(0, n)
    for order in (parts, parts[::-1]):
        np.testing.assert_array_equal(engine.merge_preempt(order)["pick"], whole["pick"])


def test_plane_update_download_and_drop():
    c = ppc.seeded()
    th = ppc.thresholds("seeded")
    ref = ppc.reference("seeded")
    n = len(c.rows)
    span = lambda j: slice(int(c.first[j]), int(c.first[j + 1]))
    # a node whose thresholds matter to some preemptor, and the longest list
    busy = next(j for j in range(n) if any(res[j].status == nat.PRE_CANDIDATE and res[j].n_violating for res in ref))
    with ppc.engine_of(c) as eng:
        for j in (0, 10, 12, 13, 14, 16, busy, 1099):   # the round trip, in the caller's order
            np.testing.assert_array_equal(eng.download_bound_pdb(j), th[span(j)])
        want = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        check(want, ref)
        ctr = eng.counters()
        for j in (busy, 16):
            lst = tuple(a[span(j)] for a in (c.b_rows, c.b_prio, c.b_start))
            eng.update_bound_pods(j, *lst)   # the same list again: its thresholds are reset
            assert (eng.download_bound_pdb(j) == INT32_MAX).all() and len(eng.download_bound_pdb(j)) == len(lst[0])
        np.testing.assert_array_equal(eng.download_bound_pdb(busy + 1), th[span(busy + 1)])   # a neighbour is untouched
        reset = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        assert not reset["n_violating_plane"][:, busy].any()
        assert (reset["plane"][:, busy] != want["plane"][:, busy]).any()
        others = np.setdiff1d(np.arange(n), [busy, 16])
        np.testing.assert_array_equal(reset["plane"][:, others], want["plane"][:, others])
        for j in (busy, 16):
            eng.update_bound_pdb(j, th[span(j)])
            np.testing.assert_array_equal(eng.download_bound_pdb(j), th[span(j)])
        assert eng.counters()["h2d_bytes"] > ctr["h2d_bytes"]
        back = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        np.testing.assert_array_equal(back["pick"], want["pick"])
        np.testing.assert_array_equal(back["plane"][:, :n], want["plane"][:, :n])
        # errors change nothing
        raises(ERR_RANGE, eng.update_bound_pdb, busy, th[span(busy)][:-1])       # n must equal the node's count
        raises(ERR_RANGE, eng.update_bound_pdb, n, th[span(busy)])
        raises(ERR_RANGE, eng.download_bound_pdb, -1)
        short = c.first.copy()
        short[-1] -= 1
        raises(ERR_RANGE, eng.set_bound_pdb, short, th[:-1])                      # a node's length differs from the table's
        np.testing.assert_array_equal(eng.download_bound_pdb(busy), th[span(busy)])
        # all-INT32_MAX thresholds and no plane at all: exactly the no-PDB answers
        plain_pick, plain_cells, _ = pc.ref_arrays(pc.reference("seeded")[:ppc.N_PRE])
        eng.set_bound_pdb(c.first, np.full(len(th), INT32_MAX, np.int32))
        none = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        np.testing.assert_array_equal(none["pick"], plain_pick)
        np.testing.assert_array_equal(none["plane"][:, :n], plain_cells)
        eng.set_bound_pdb(c.first, th)
        eng.set_bound_pdb(None, None)   # dropped
        raises(ERR_STATE, eng.download_bound_pdb, 0)
        raises(ERR_STATE, eng.update_bound_pdb, 0, th[span(0)])
        for with_plane in (True, False):
            got = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=with_plane)
            np.testing.assert_array_equal(got["pick"], plain_pick)
            if with_plane:
                np.testing.assert_array_equal(got["plane"][:, :n], plain_cells)
        # kg_bound_set and kg_snapshot_reset drop the plane too
        eng.set_bound_pdb(c.first, th)
        eng.set_bound_pods(c.first, c.b_rows, c.b_prio, c.b_start, c.max_per_node)
        raises(ERR_STATE, eng.download_bound_pdb, 0)
        np.testing.assert_array_equal(eng.preempt(c.pods, c.pod_prio, c.now_ns)["pick"], plain_pick)
        eng.set_bound_pdb(c.first, th)
        eng.load_snapshot(c.rows)
        raises(ERR_STATE, eng.set_bound_pdb, c.first, th)   # no table
    with pc.engine_of(c, table=False) as eng:
        raises(ERR_STATE, eng.set_bound_pdb, c.first, th)
        raises(ERR_STATE, eng.set_bound_pdb, None, None)


def test_purity(seeded_engine):
    c, eng = ppc.seeded(), seeded_engine
    gen, rows0, q0 = eng.generation(), eng.download(), eng.download_quotas()
    tab0 = [eng.download_bound_pods(j) for j in (0, 13, 16, 1031)]
    th0 = [eng.download_bound_pdb(j) for j in (0, 13, 16, 1031)]
    ctr0 = eng.counters()
    eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
    ctr1 = eng.counters()
    assert eng.generation() == gen
    assert (ctr1["placed"], ctr1["resolved"]) == (ctr0["placed"], ctr0["resolved"])
    assert ctr1["eval_calls"] == ctr0["eval_calls"] + 1
    np.testing.assert_array_equal(eng.download(), rows0)
    np.testing.assert_array_equal(eng.download_quotas(), q0)
    for j, t0, p0 in zip((0, 13, 16, 1031), tab0, th0):
        t1 = eng.download_bound_pods(j)
        for a, b in zip(t0, t1):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(eng.download_bound_pdb(j), p0)
