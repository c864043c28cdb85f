"""kg_candidates (Engine.candidates): the k best feasible nodes per pod with the engine plugins' scores, against
tests/cand_ref.py on the oracle's matrices (the four profiles of tests/cycle_cases.py: 1,100 nodes, a full tile and a
ragged one of 76, the nodes BIG on the exact pair path) and on a twin engine's kg_eval planes (the cases of
tests/why_cases.py, eligibility classes, ElasticQuota, shards, grid edges)."""
import functools

import numpy as np
import pytest

import cand_ref as cr
import cycle_cases as cc
import why_cases as wc
import why_ref
from guarded_out import GuardedPlane
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_RANGE, ERR_STATE = -1, -3, -4, -5
KS = (1, 16, 64)


@pytest.fixture(scope="module")
def dev():
    import torch   # torch's HIP context first: it does not initialise beside a live engine
    d = torch.device("cuda", 0)
    torch.zeros(1, device=d)
    torch.cuda.synchronize(d)
    return d


def raises(status, fn, *a, **kw):
    with pytest.raises(engine.EngineError) as ei:
        fn(*a, **kw)
    assert f"status {status}:" in str(ei.value), str(ei.value)


def check(res, ref, what=""):
    """A candidates() result against cand_ref's (keys, scores, n_feasible), and the contract's own invariants."""
    keys, scores, nf = ref
    np.testing.assert_array_equal(res["keys"], keys, err_msg=what)
    np.testing.assert_array_equal(res["n_feasible"], nf, err_msg=what)
    if "scores" in res:
        np.testing.assert_array_equal(res["scores"], scores, err_msg=what)
        assert not res["scores"][..., 3].any() and not res["scores"][res["keys"] == 0].any()
    k = keys.shape[1]
    got = res["keys"]
    assert ((got[:, 1:] < got[:, :-1]) | (got[:, 1:] == 0)).all()            # strictly descending, then zeros
    np.testing.assert_array_equal((got != 0).sum(axis=1), np.minimum(nf, k))   # exactly min(n_feasible, k) entries
    if "nodes" in res:
        node, total = engine.decode_top1(got)
        np.testing.assert_array_equal(res["nodes"], node)
        np.testing.assert_array_equal(res["totals"], total)


def planes_of(c_cfg, eng, pods, now_ns, width):
    """(totals, fit, la, numa, top1) of `pods` from the engine's kg_eval planes over its shard (planes mode)."""
    eng.set_pods(pods)
    out = eng.eval(now_ns)
    return (*cr.from_planes(c_cfg, out, width), out["top1"].copy())


@functools.lru_cache(maxsize=None)
def twin_planes(name):
    """The why_cases case on a twin engine through kg_pods_set + kg_eval: computed once, read-only."""
    c = wc.case(name)
    with wc.engine_of(c) as twin:
        out = planes_of(c.cfg, twin, c.pods, c.now_ns, len(c.rows))
    for a in out:
        a.setflags(write=False)
    return out


def ref_of(planes, k, lo=0, hi=None, rows=None):
    tot, fit, la, numa, _ = planes
    rows = slice(None) if rows is None else rows
    return cr.cand_ref(tot[rows, lo:hi], k, fit[rows, lo:hi], la[rows, lo:hi], numa[rows, lo:hi], node0=lo)


@pytest.mark.parametrize("profile", cc.PROFILES)
def test_oracle_parity(profile):
    """Every profile at k = 1, 16, 64.  Checked in the reference before the engine runs: a tie in total straddles the
    cut at k = 16 and at k = 64 (at k = 1 only the profiles `most` and `la_extra` have one, so that is asserted over
    the profiles together in tests/test_candidates_cpu.py), and a BIG node is listed at k = 64."""
    cfg, cl, rows, pods = cc.case(profile)
    _, fit, la, tot = cc.oracle_matrix(profile)
    assert cr.tie_at_cut(tot, 16) and cr.tie_at_cut(tot, 64)
    keys64 = cr.cand_ref(tot, 64, fit, la)[0]
    listed = engine.decode_top1(keys64)[0]
    assert np.isin(listed[keys64 != 0], cc.BIG).any()
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(rows)
        for k in KS:
            ref = cr.cand_ref(tot, k, fit, la)
            got = eng.candidates(pods, cl.now_ns, k)
            check(got, ref, f"k={k}")
            again = eng.candidates(pods, cl.now_ns, k)     # identical from run to run
            for name in got:
                np.testing.assert_array_equal(again[name], got[name], err_msg=name)
            bare = eng.candidates(pods, cl.now_ns, k, scores=False)
            assert "scores" not in bare
            check(bare, ref, f"k={k} without scores")


@pytest.mark.parametrize("name", wc.NAMES)
def test_cases_against_the_twin(name):
    c = wc.case(name)
    planes = twin_planes(name)
    tot, _, _, numa, top1 = planes
    assert (tot >= 0).any() and (tot < 0).any()
    if name == "edited":
        assert not (tot[0] >= 0).any() and not (tot[:, c.removed] >= 0).any()
        assert (tot[wc.DAEMON_POD] >= 0).any() and (tot[wc.EMPTY_POD] >= 0).any()
    if name == "numa":
        assert numa.any() and int(c.cfg["weight_numa"]) > 0
    with wc.engine_of(c) as eng:
        for k in KS:
            got = eng.candidates(c.pods, c.now_ns, k)
            check(got, ref_of(planes, k), f"{name} k={k}")
            np.testing.assert_array_equal(got["keys"][:, 0], top1)
        if name == "numa":
            assert got["scores"][..., 2].any()


def test_eligibility():
    c = wc.case("edited")
    n, k = len(c.rows), 16
    few = np.zeros(n, bool)
    few[[4, 130, 700, 1030, 1090]] = True      # a third class with exactly 5 eligible nodes
    classes = np.concatenate([wc.elig_classes(n), few[None]])
    pods = c.pods.copy()
    pods["elig_class"] = np.arange(len(pods)) % 4
    with wc.engine_of(c) as eng, wc.engine_of(c) as twin:
        raises(ERR_RANGE, eng.candidates, pods, c.now_ns, k)   # no class loaded yet
        eng.set_eligibility(classes)
        twin.set_eligibility(classes)
        planes = planes_of(c.cfg, twin, pods, c.now_ns, n)
        nf = (planes[0] >= 0).sum(axis=1)
        assert ((nf > 0) & (nf < k)).any() and (nf == 0).any() and (nf > k).any()
        assert ((nf[3::4] > 0) & (nf[3::4] <= 5)).any()
        got = eng.candidates(pods, c.now_ns, k)
        check(got, ref_of(planes, k))
        np.testing.assert_array_equal(got["keys"][:, 0], planes[4])
        bad = pods[:4].copy()
        bad["elig_class"][2] = 4               # one past the loaded classes
        raises(ERR_RANGE, eng.candidates, bad, c.now_ns, k)


@functools.lru_cache(maxsize=None)
def wide_case():
    """2,049 nodes (two full tiles and one node), 8 pods, every 97th node beyond the fp64 bounds."""
    cfg = shipped_profile()
    cl = synth.make_cluster(2_049, 8, seed=53)
    cl.nodes["allocatable"]["v"][3::97, 1] = (1 << 43) + 99
    cl = cl.with_nodes(cl.nodes)
    rows, pods = engine.build_node_rows(cfg, cl), engine.build_pod_rows(cfg, cl, np.arange(8))
    rows.setflags(write=False)
    pods.setflags(write=False)
    return cfg, cl.now_ns, rows, pods


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 1_023, 1_024, 1_025, 2_049])
def test_grid_edges_nodes(n_nodes):
    cfg, now_ns, rows, pods = wide_case()
    with engine.Engine(cfg) as eng, engine.Engine(cfg) as twin:
        eng.load_snapshot(rows[:n_nodes])
        twin.load_snapshot(rows[:n_nodes])
        planes = planes_of(cfg, twin, pods, now_ns, n_nodes)
        got = eng.candidates(pods, now_ns, 64)     # k > n_nodes at the small sizes
        check(got, ref_of(planes, 64), f"n_nodes={n_nodes}")
        np.testing.assert_array_equal(got["keys"][:, 0], planes[4])


@pytest.mark.parametrize("n_pods", [1, 9, 256])
def test_grid_edges_pods(n_pods):
    c = wc.case("edited")
    idx = np.arange(n_pods) % len(c.pods)
    with wc.engine_of(c) as eng:
        check(eng.candidates(c.pods[idx], c.now_ns, 16), ref_of(twin_planes("edited"), 16, rows=idx))


def test_shards():
    c = wc.case("edited")
    n = len(c.rows)
    planes = twin_planes("edited")
    with wc.engine_of(c) as eng:
        for k in KS:
            eng.set_shard(0, n)
            whole = eng.candidates(c.pods, c.now_ns, k)
            check(whole, ref_of(planes, k))
            parts = []
            for lo, hi in ((0, 1_024), (1_024, n)):
                eng.set_shard(lo, hi)
                parts.append(eng.candidates(c.pods, c.now_ns, k))
                check(parts[-1], ref_of(planes, k, lo, hi), f"shard [{lo}, {hi}) k={k}")
            merged = engine.merge_candidates(parts)
            assert merged.keys() == whole.keys()
            for name in whole:
                np.testing.assert_array_equal(merged[name], whole[name], err_msg=f"{name} k={k}")
        eng.set_shard(1_024, 1_024)   # an empty shard: all-zero outputs
        empty = eng.candidates(c.pods, c.now_ns, 16)
        assert not empty["keys"].any() and not empty["scores"].any() and not empty["n_feasible"].any()
        assert (empty["nodes"] == -1).all() and (empty["totals"] == -1).all()


def test_elastic_quota_gate():
    cfg, now_ns, rows, pods, quotas = wc.quota_case()
    gated = why_ref.pod_why_ref(cfg, pods, quotas) != 0
    assert gated[7] and gated[3] and gated[4] and not (gated[11] or gated[8] or gated[0] or gated[2])
    with engine.Engine(cfg) as eng, engine.Engine(cfg) as twin:
        eng.load_snapshot(rows)
        twin.load_snapshot(rows)
        raises(ERR_STATE, eng.candidates, pods, now_ns, 16)   # quota indices without their groups
        eng.set_quotas(quotas)
        twin.set_quotas(quotas)
        planes = planes_of(cfg, twin, pods, now_ns, len(rows))
        np.testing.assert_array_equal((planes[0] >= 0).any(axis=1), ~gated)   # kg_eval folds the gate into the mask
        for k in (1, 16):
            got = eng.candidates(pods, now_ns, k)
            check(got, ref_of(planes, k))
            assert not got["keys"][gated].any() and not got["n_feasible"][gated].any() and got["keys"][~gated, 0].all()
            np.testing.assert_array_equal(got["keys"][:, 0], planes[4])
        np.testing.assert_array_equal(eng.download_quotas(), quotas)


def test_required_reservation_with_none_loaded():
    """The node-independent gate of kg_pod_why / kg_cycle_one: a pod that requires a reservation while no slot is
    loaded has no candidate.  (kg_eval folds this gate into its mask only in the launches that apply a gate at all -
    quotas or slots loaded - so the reference here is the twin's planes with that pod's row closed, and the keys are
    compared with kg_cycle_one's, which closes the pod the same way.)"""
    cfg = make_config(plugins=("NodeResourcesFit", "LoadAwareScheduling", "Reservation"))
    cl = cc.cluster()
    rows, pods = engine.build_node_rows(cfg, cl), engine.build_pod_rows(cfg, cl, np.arange(4))
    req = pods.copy()
    req["rsv_affinity_class"][1] = 0   # a required reservation, and no slots
    with engine.Engine(cfg) as eng, engine.Engine(cfg) as twin:
        eng.load_snapshot(rows)
        twin.load_snapshot(rows)
        tot, fit, la, numa, _ = planes_of(cfg, twin, req, cl.now_ns, len(rows))
        tot = tot.copy()
        tot[1] = -1
        assert (tot[[0, 2, 3]] >= 0).any(axis=1).all()
        got = eng.candidates(req, cl.now_ns, 16)
        check(got, cr.cand_ref(tot, 16, fit, la, numa))
        assert not got["keys"][1].any() and not got["scores"][1].any() and got["n_feasible"][1] == 0
        one = [eng.cycle_one(req[i:i + 1], cl.now_ns, commit=False)["key"] for i in range(4)]
        assert one[1] == 0
        np.testing.assert_array_equal(got["keys"][:, 0], np.array(one, np.uint64))


def test_purity_and_counters():
    c = wc.case("edited")
    with wc.engine_of(c) as eng:
        eng.set_pods(c.pods[:32])
        out0 = eng.eval(c.now_ns)
        gen, rows0, ctr0 = eng.generation(), eng.download(), eng.counters()
        res = eng.candidates(c.pods[40:60], c.now_ns, 16)
        ctr1 = eng.counters()
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), rows0)
        assert (ctr1["placed"], ctr1["resolved"]) == (ctr0["placed"], ctr0["resolved"])
        assert ctr1["eval_calls"] == ctr0["eval_calls"] + 1
        assert ctr1["evals"] == ctr0["evals"] + 20 * len(c.rows)
        assert ctr1["out_bytes"] == ctr0["out_bytes"] + sum(res[k].nbytes for k in ("keys", "scores", "n_feasible"))
        assert ctr1["h2d_bytes"] > ctr0["h2d_bytes"]
        bare = eng.candidates(c.pods[40:60], c.now_ns, 16, scores=False)
        ctr2 = eng.counters()
        assert ctr2["out_bytes"] == ctr1["out_bytes"] + bare["keys"].nbytes + bare["n_feasible"].nbytes
        assert eng.candidates(c.pods[:0], c.now_ns, 16)["keys"].shape == (0, 16)   # n = 0: a no-op
        assert eng.counters() == ctr2
        out1 = eng.eval(c.now_ns)   # the uploaded batch is still the first 32 pods
        assert out0.keys() == out1.keys()
        for k in out0:
            np.testing.assert_array_equal(out0[k], out1[k], err_msg=k)


def test_argument_errors():
    c = wc.case("edited")
    with wc.engine_of(c) as eng:
        before = eng.counters()
        raises(ERR_RANGE, eng.candidates, c.pods[np.arange(257) % len(c.pods)], c.now_ns, 16)
        raises(ERR_RANGE, eng.candidates, c.pods[:2], c.now_ns, 0)
        raises(ERR_RANGE, eng.candidates, c.pods[:2], c.now_ns, 65)
        bad = c.pods[:2].copy()
        bad["elig_class"][1] = 1
        raises(ERR_RANGE, eng.candidates, bad, c.now_ns, 16)
        L = nat.lib()
        keys = np.zeros((1, 16), np.uint64)
        assert L.kg_candidates(eng._h, nat.ptr(c.pods[:1]), 1, int(c.now_ns), 16, 0x1, nat.ptr(keys), None, None, 0) == ERR_INVALID_ARG
        assert L.kg_candidates(eng._h, nat.ptr(c.pods[:1]), 1, int(c.now_ns), 16, 0, None, None, None, 0) == ERR_INVALID_ARG
        assert L.kg_candidates(eng._h, None, 1, int(c.now_ns), 16, 0, nat.ptr(keys), None, None, 0) == ERR_INVALID_ARG
        assert L.kg_candidates(eng._h, nat.ptr(c.pods[:1]), -1, int(c.now_ns), 16, 0, nat.ptr(keys), None, None, 0) == ERR_INVALID_ARG
        assert eng.counters() == before and not keys.any()
    with engine.Engine(c.cfg) as eng:   # no snapshot
        raises(ERR_STATE, eng.candidates, c.pods[:1], c.now_ns, 16)


def test_refusals_launch_nothing():
    # reservation slots loaded
    cfg = make_config(plugins=("NodeResourcesFit", "LoadAwareScheduling", "Reservation"))
    cl = cc.cluster()
    rows, pods = engine.build_node_rows(cfg, cl), engine.build_pod_rows(cfg, cl, np.arange(4))
    rsv = np.zeros(1, dtype=nat.RESERVATION)
    rsv["node"], rsv["flags"], rsv["owner_classes"] = 0, nat.RSV_AVAILABLE, 1
    rsv["allocatable"]["v"][0, nat.RES_CPU], rsv["allocatable"]["present"] = 1000, 1 << nat.RES_CPU
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(rows)
        eng.candidates(pods, cl.now_ns, 16)
        eng.set_reservations(rsv)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.candidates, pods, cl.now_ns, 16)
        assert eng.counters() == before
    # cpuset binding: a pod that binds, a node with a CPU bind policy
    c = wc.case("numa")
    with wc.engine_of(c) as eng:
        bind = c.pods[:3].copy()
        bind["flags"][2] = (bind["flags"][2] | nat.POD_NUMA_CPU_BIND) & ~np.uint32(nat.POD_NUMA_SKIP)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.candidates, bind, c.now_ns, 16)
        assert eng.counters() == before
        eng.candidates(c.pods[:3], c.now_ns, 16)
        j = int(np.flatnonzero((c.rows["flags"] & nat.NODE_NUMA_OPTIONS) != 0)[0])
        row = c.rows[j:j + 1].copy()
        row["node_cpu_bind"] = nat.NODE_CPU_BIND_FULL_PCPUS_ONLY
        row["cpus_per_core"] = 2   # (a bind policy needs CPU detail on a valid topology: kg_snapshot_upsert)
        eng.upsert([j], row)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.candidates, c.pods[:3], c.now_ns, 16)
        assert eng.counters() == before


@pytest.mark.parametrize("prefill", [0x00, 0xFF])
def test_containment(dev, prefill):
    """Device outputs in guarded buffers over the two shapes of test_why_gpu.test_containment (the first 1,025 nodes:
    two tiles; the shard [1024, 1087): 63 nodes that start at the second tile), the keys pointer in the middle of a
    guarded allocation: guards intact, every cell written whatever the buffers held, a NULL plane not needed."""
    import torch
    c = wc.case("edited")
    pods = c.pods[:9]
    rows = np.arange(9)
    planes = twin_planes("edited")
    k = 16
    for n_nodes, (lo, hi) in ((1_025, (0, 1_025)), (len(c.rows), (1_024, 1_087))):
        ref = ref_of(planes, k, lo, hi, rows=rows)
        key_b, sc_b, nf_b = len(pods) * k * 8, len(pods) * k * 4, len(pods) * 4
        with wc.engine_of(c, n_nodes) as eng:
            eng.set_shard(lo, hi)
            # keys 4 KiB into a guarded payload of 3 × their size: the bytes before and after them are guards too
            kp = GuardedPlane(4096 + 3 * key_b, prefill, dev)
            sp = GuardedPlane(sc_b, prefill, dev)
            fp = GuardedPlane(nf_b, prefill, dev)
            torch.cuda.synchronize(dev)
            eng.candidates_device(pods, c.now_ns, k, kp.ptr + 4096 + key_b, scores_ptr=sp.ptr, n_feasible_ptr=fp.ptr)
            for g in (kp, sp, fp):
                assert g.stray().size == 0
            payload = kp.read()[1]
            inner = payload[4096 + key_b:4096 + 2 * key_b]
            outer = np.concatenate([payload[:4096 + key_b], payload[4096 + 2 * key_b:]])
            assert (outer == prefill).all()
            got = {"keys": inner.view(np.uint64).reshape(len(pods), k), "scores": sp.read()[1].reshape(len(pods), k, 4),
                   "n_feasible": fp.read()[1].view(np.uint32)}
            check(got, ref, f"shard [{lo}, {hi})")
            # scores = NULL and n_feasible = NULL, each alone
            for with_scores in (False, True):
                kp2 = GuardedPlane(key_b, prefill, dev)
                other = GuardedPlane(sc_b if with_scores else nf_b, prefill, dev)
                torch.cuda.synchronize(dev)
                eng.candidates_device(pods, c.now_ns, k, kp2.ptr, scores_ptr=other.ptr if with_scores else 0,
                                      n_feasible_ptr=0 if with_scores else other.ptr)
                assert kp2.stray().size == 0 and other.stray().size == 0
                np.testing.assert_array_equal(kp2.read()[1].view(np.uint64).reshape(len(pods), k), got["keys"])
                if with_scores:
                    np.testing.assert_array_equal(other.read()[1].reshape(len(pods), k, 4), got["scores"])
                else:
                    np.testing.assert_array_equal(other.read()[1].view(np.uint32), got["n_feasible"])
