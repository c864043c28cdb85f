"""kg_diagnose (Engine.diagnose): per-node rejection reasons and their counts against tests/why_ref.py and against
matrix mode, on the three cases of tests/why_cases.py — the edited la_extra cluster (1,100 nodes: a full tile and a
ragged one of 76, nodes beyond the fp64 bounds on the canonical-row path, removed nodes), the later named slots and
NodeNUMAResource."""
import numpy as np
import pytest

import why_cases as wc
import why_ref
from guarded_out import GuardedPlane
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import make_config

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_RANGE, ERR_STATE = -1, -3, -4, -5


@pytest.fixture(scope="module")
def dev():
    import torch   # torch's HIP context first: it does not initialise beside a live engine
    d = torch.device("cuda", 0)
    torch.zeros(1, device=d)
    torch.cuda.synchronize(d)
    return d


def check(res, ref, n_nodes, pod_why=None):
    """counts, plane (columns < n_nodes) and pod-level words of a diagnose() result against reference words [P][N]."""
    np.testing.assert_array_equal(res["counts"], why_ref.counts_ref(ref))
    if "why" in res:
        np.testing.assert_array_equal(res["why"][:, :n_nodes], ref)
    np.testing.assert_array_equal(res["pod_why"], np.zeros(len(ref), np.uint32) if pod_why is None else pod_why)
    c = res["counts"].astype(np.int64)
    assert (c[:, 0] + c[:, nat.WHY_SLOT_REJECTED] + c[:, nat.WHY_SLOT_FEASIBLE] == n_nodes).all()
    assert not c[:, 28:30].any()


def raises(status, fn, *a, **kw):
    with pytest.raises(engine.EngineError) as ei:
        fn(*a, **kw)
    assert f"status {status}:" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("name", wc.NAMES)
def test_parity(name):
    c = wc.case(name)
    n = len(c.rows)
    full, first = wc.reference(name), wc.reference(name, True)
    assert (full != 0).any() and (full == 0).any()
    with wc.engine_of(c) as eng, wc.engine_of(c) as twin:
        twin.set_pods(c.pods)
        mask = engine.unpack_mask(twin.eval(c.now_ns, scores=False, top1=False, numa_scores=False)["mask"], n)
        got = eng.diagnose(c.pods, c.now_ns, why=True)
        check(got, full, n)
        np.testing.assert_array_equal(got["why"][:, :n] == 0, mask)
        np.testing.assert_array_equal(got["counts"][:, nat.WHY_SLOT_FEASIBLE], mask.sum(axis=1))
        check(eng.diagnose(c.pods, c.now_ns), full, n)   # counts alone: the form without the plane
        ff = eng.diagnose(c.pods, c.now_ns, first_fail=True, why=True)
        check(ff, first, n)
        w = ff["why"][:, :n]
        np.testing.assert_array_equal(w != 0, got["why"][:, :n] != 0)
        groups = [(w & g) != 0 for g in (nat.WHY_ABSENT, nat.WHY_ELIG, nat.WHY_FIT_MASK, nat.WHY_LOADAWARE, nat.WHY_NUMA)]
        assert (np.sum(groups, axis=0) <= 1).all()
        # identical from run to run
        np.testing.assert_array_equal(eng.diagnose(c.pods, c.now_ns)["counts"], got["counts"])


@pytest.mark.parametrize("first_fail", [False, True])
def test_eligibility(first_fail):
    c = wc.case("edited")
    n = len(c.rows)
    classes = wc.elig_classes(n)
    pods = c.pods.copy()
    pods["elig_class"] = np.arange(len(pods)) % 3
    ref = why_ref.why_ref(c.cfg, c.ref_rows, pods, c.now_ns, first_fail=first_fail, elig=classes)
    elig_bit = (ref & nat.WHY_ELIG) != 0
    assert elig_bit[1::3].any() and elig_bit[2::3, :1024].any() and not elig_bit[0::3].any()
    with wc.engine_of(c) as eng:
        raises(ERR_RANGE, eng.diagnose, pods, c.now_ns)   # no class loaded yet
        eng.set_eligibility(classes)
        check(eng.diagnose(pods, c.now_ns, first_fail=first_fail, why=True), ref, n)


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 1_023, 1_024, 1_025])
def test_grid_edges_nodes(n_nodes):
    c = wc.case("edited")
    pods = c.pods[:8]
    ref = wc.reference("edited")[:8, :n_nodes]
    with wc.engine_of(c, n_nodes) as eng:
        check(eng.diagnose(pods, c.now_ns, why=True), ref, n_nodes)


@pytest.mark.parametrize("n_pods", [1, 9, 256])
def test_grid_edges_pods(n_pods):
    c = wc.case("edited")
    n = len(c.rows)
    idx = np.arange(n_pods) % len(c.pods)
    pods = c.pods[idx]
    with wc.engine_of(c) as eng:
        check(eng.diagnose(pods, c.now_ns, why=True), wc.reference("edited")[idx], n)


def test_argument_errors():
    c = wc.case("edited")
    with wc.engine_of(c) as eng:
        before = eng.counters()
        raises(ERR_RANGE, eng.diagnose, c.pods[np.arange(257) % len(c.pods)], c.now_ns)
        bad = c.pods[:2].copy()
        bad["elig_class"][1] = 1
        raises(ERR_RANGE, eng.diagnose, bad, c.now_ns)
        L = nat.lib()
        counts = np.zeros((1, nat.WHY_SLOTS), np.uint32)
        assert L.kg_diagnose(eng._h, nat.ptr(c.pods[:1]), 1, int(c.now_ns), 0x2, nat.ptr(counts), None, None, 0) == ERR_INVALID_ARG
        assert L.kg_diagnose(eng._h, nat.ptr(c.pods[:1]), 1, int(c.now_ns), 0, None, None, None, 0) == ERR_INVALID_ARG
        assert eng.counters() == before
    with engine.Engine(c.cfg) as eng:   # no snapshot
        raises(ERR_STATE, eng.diagnose, c.pods[:1], c.now_ns)


def test_shards():
    c = wc.case("edited")
    n = len(c.rows)
    ref = wc.reference("edited")
    with wc.engine_of(c) as eng:
        whole = eng.diagnose(c.pods, c.now_ns, why=True)
        check(whole, ref, n)
        total = np.zeros_like(whole["counts"])
        for lo, hi in ((0, 1_024), (1_024, n)):
            eng.set_shard(lo, hi)
            part = eng.diagnose(c.pods, c.now_ns, why=True)
            check(part, ref[:, lo:hi], hi - lo)
            np.testing.assert_array_equal(part["why"][:, :hi - lo], whole["why"][:, lo:hi])
            total += part["counts"]
        np.testing.assert_array_equal(total, whole["counts"])
        eng.set_shard(1_024, 1_024)   # an empty shard: all-zero counts
        empty = eng.diagnose(c.pods, c.now_ns, why=True)
        assert not empty["counts"].any() and empty["why"].shape == (len(c.pods), 0)


def test_purity():
    c = wc.case("edited")
    with wc.engine_of(c) as eng:
        eng.set_pods(c.pods[:32])
        out0 = eng.eval(c.now_ns)
        gen, rows0, ctr0 = eng.generation(), eng.download(), eng.counters()
        res = eng.diagnose(c.pods[40:60], c.now_ns, why=True)
        ctr1 = eng.counters()
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), rows0)
        assert (ctr1["placed"], ctr1["resolved"]) == (ctr0["placed"], ctr0["resolved"])
        assert ctr1["eval_calls"] == ctr0["eval_calls"] + 1
        assert ctr1["evals"] == ctr0["evals"] + 20 * len(c.rows)
        assert ctr1["out_bytes"] == ctr0["out_bytes"] + sum(v.nbytes for v in res.values())
        assert ctr1["h2d_bytes"] > ctr0["h2d_bytes"]
        out1 = eng.eval(c.now_ns)   # the uploaded batch is still the first 32 pods
        assert out0.keys() == out1.keys()
        for k in out0:
            np.testing.assert_array_equal(out0[k], out1[k], err_msg=k)


def test_elastic_quota_pod_words():
    cfg, now_ns, rows, pods, quotas = wc.quota_case()
    want = why_ref.pod_why_ref(cfg, pods, quotas)
    # over the cpu limit, through the parent, the min gate of a non-preemptible pod; not: the same group's preemptible
    # pod, a group with room, no quota, a batch pod whose resources the tight group does not name
    assert want[7] and want[3] and want[4] and not (want[11] or want[8] or want[0] or want[2])
    cfg_flat = cfg.copy()
    cfg_flat["eq_check_parent_quota"] = 0
    want_flat = why_ref.pod_why_ref(cfg_flat, pods, quotas)
    assert want[3] and not want_flat[3]
    ref = why_ref.why_ref(cfg, rows, pods, now_ns)
    for conf, w in ((cfg, want), (cfg_flat, want_flat)):
        with engine.Engine(conf) as eng:
            eng.load_snapshot(rows)
            raises(ERR_STATE, eng.diagnose, pods, now_ns)   # quota indices without their groups
            eng.set_quotas(quotas)
            check(eng.diagnose(pods, now_ns, why=True), ref, len(rows), pod_why=w)   # the node words ignore the gate
            np.testing.assert_array_equal(eng.download_quotas(), quotas)


def test_refusals_launch_nothing():
    import cycle_cases as cc
    # reservation slots loaded
    cfg = make_config(plugins=("NodeResourcesFit", "LoadAwareScheduling", "Reservation"))
    cl = cc.cluster()
    rows, pods = engine.build_node_rows(cfg, cl), engine.build_pod_rows(cfg, cl, np.arange(4))
    rsv = np.zeros(1, dtype=nat.RESERVATION)
    rsv["node"], rsv["flags"], rsv["owner_classes"] = 0, nat.RSV_AVAILABLE, 1
    rsv["allocatable"]["v"][0, nat.RES_CPU], rsv["allocatable"]["present"] = 1000, 1 << nat.RES_CPU
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(rows)
        req = pods.copy()
        req["rsv_affinity_class"][1] = 0   # a required reservation, and no slots: the pod-level word
        got = eng.diagnose(req, cl.now_ns)
        np.testing.assert_array_equal(got["pod_why"], [0, nat.WHY_POD_RSV_REQUIRED, 0, 0])
        np.testing.assert_array_equal(got["counts"], why_ref.counts_ref(why_ref.why_ref(cfg, rows, req, cl.now_ns)))
        eng.set_reservations(rsv)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.diagnose, pods, cl.now_ns)
        assert eng.counters() == before
    # cpuset binding: a pod that binds, a node with a CPU bind policy
    c = wc.case("numa")
    with wc.engine_of(c) as eng:
        bind = c.pods[:3].copy()
        bind["flags"][2] = (bind["flags"][2] | nat.POD_NUMA_CPU_BIND) & ~np.uint32(nat.POD_NUMA_SKIP)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.diagnose, bind, c.now_ns)
        assert eng.counters() == before
        eng.diagnose(c.pods[:3], c.now_ns)
        j = int(np.flatnonzero((c.rows["flags"] & nat.NODE_NUMA_OPTIONS) != 0)[0])
        row = c.rows[j:j + 1].copy()
        row["node_cpu_bind"] = nat.NODE_CPU_BIND_FULL_PCPUS_ONLY
        row["cpus_per_core"] = 2   # (a bind policy needs CPU detail on a valid topology: kg_snapshot_upsert)
        eng.upsert([j], row)
        before = eng.counters()
        raises(ERR_UNSUPPORTED, eng.diagnose, c.pods[:3], c.now_ns)
        assert eng.counters() == before


@pytest.mark.parametrize("prefill", [0x00, 0xFF])
def test_containment(dev, prefill):
    """Device outputs in guarded buffers over odd W (the first 1,025 nodes: W = 17, two tiles; the shard [1024, 1087):
    W = 1, a 63-node range that starts at the second tile), the counts pointer in the middle of a guarded allocation:
    guards intact, every in-range cell written whatever the buffers held."""
    import torch
    c = wc.case("edited")
    pods = c.pods[:9]
    ref = wc.reference("edited")[:9]
    for n_nodes, (lo, hi) in ((1_025, (0, 1_025)), (len(c.rows), (1_024, 1_087))):
        width = hi - lo
        words = (width + 63) // 64
        stride = words * 64
        with wc.engine_of(c, n_nodes) as eng:
            eng.set_shard(lo, hi)
            why = GuardedPlane(len(pods) * stride * 4, prefill, dev)
            # counts 4 KiB into a guarded payload of 3 × their size: the bytes before and after them are guards too
            cnt_b = len(pods) * nat.WHY_SLOTS * 4
            cnt = GuardedPlane(4096 + 3 * cnt_b, prefill, dev)
            pw = GuardedPlane(len(pods) * 4, prefill, dev)
            torch.cuda.synchronize(dev)
            eng.diagnose_device(pods, c.now_ns, cnt.ptr + 4096 + cnt_b, pod_why_ptr=pw.ptr, why_ptr=why.ptr)
            for g in (why, cnt, pw):
                assert g.stray().size == 0
            payload = cnt.read()[1]
            inner = payload[4096 + cnt_b:4096 + 2 * cnt_b]
            outer = np.concatenate([payload[:4096 + cnt_b], payload[4096 + 2 * cnt_b:]])
            assert (outer == prefill).all()
            got = {"counts": inner.view(np.uint32).reshape(len(pods), nat.WHY_SLOTS),
                   "why": why.read()[1].view(np.uint32).reshape(len(pods), stride),
                   "pod_why": pw.read()[1].view(np.uint32)}
            check(got, ref[:, lo:hi], width)
            # counts alone (the form without the plane)
            cnt2 = GuardedPlane(cnt_b, prefill, dev)
            torch.cuda.synchronize(dev)
            eng.diagnose_device(pods, c.now_ns, cnt2.ptr)
            assert cnt2.stray().size == 0
            np.testing.assert_array_equal(cnt2.read()[1].view(np.uint32).reshape(len(pods), nat.WHY_SLOTS), got["counts"])
