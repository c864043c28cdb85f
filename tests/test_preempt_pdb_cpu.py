"""The PDB form of the preemption dry run on the host: kg_pdb_thresholds against the literal budget walk,
kg_row_preempt_pdb against tests/preempt_pdb_ref.py on every pair, the plain form under NULL / INT32_MAX thresholds,
ingest.bound_pdb, kg_preempt_merge's order with n_violating, the error returns, and the conditions the cases of
tests/preempt_pdb_cases.py must meet.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import preempt_cases as pc
import preempt_pdb_cases as ppc
import preempt_pdb_ref as ppr
import preempt_ref as pr
from koordinator_amd import _native as nat
from koordinator_amd import engine, ingest

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "koord_gpu.h")
NEW_FUNCTIONS = ("kg_pdb_thresholds", "kg_bound_pdb_set", "kg_bound_pdb_update", "kg_bound_pdb_download", "kg_row_preempt_pdb")
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_RANGE = -1, -3, -4
INT32_MAX = np.iinfo(np.int32).max


def test_header_native_and_library_agree():
    L = nat.lib()
    text = open(HEADER).read()
    for fn in NEW_FUNCTIONS:
        assert fn in nat.EXPORTED and getattr(L, fn) is not None
        assert re.search(rf"\b{fn}\s*\(", text), fn
    assert nat.PDB_PRIO_NONE == INT32_MAX
    assert L.kg_abi_version() == 13 and nat.ABI_VERSION == 13   # new symbols only


def _plain_reference(c):
    """The no-PDB reference (tests/preempt_ref.py) of a case of preempt_pdb_cases."""
    if c.base is not None:
        return pc.reference(c.base)[:len(c.pods)]
    return tuple(pr.dry_run(c.cfg, c.ref_rows, c.first, c.b_rows, c.b_prio, c.b_start, c.pods[i], int(c.pod_prio[i]), c.quotas,
                            c.now_ns) for i in range(len(c.pods)))


def test_case_conditions():
    """What the cases must exercise, from the references alone.  The victim conditions hold on the seeded case; the
    two pick conditions (a pick that differs from the no-PDB pick, a pick the n_violating step decides) hold on each
    1,100-node wide case by itself: see tests/preempt_pdb_cases.py on why no PDB assignment reaches them with the
    seeded preemptors.  The last lines run the wide cases' shard picks through kg_preempt_merge, so this test too fails
    without the feature."""
    c = ppc.seeded()
    assert len(c.pods) == ppc.N_PRE and len(c.ref_rows) == 1_100
    both = differs = late = quota_only = errors = moved = 0
    steps = []
    for c in ppc.cases():
        ref, plain = ppc.reference(c.name), _plain_reference(c)
        assert len(ref) == len(c.pods) and all(len(res) == len(c.ref_rows) for res in ref)   # no pair is left out
        for res, res0 in zip(ref, plain):
            for r, r0 in zip(res, res0):
                assert r.status == r0.status or nat.PRE_ERROR in (r.status, r0.status)   # the order can move an error only
                if r.status != nat.PRE_CANDIDATE:
                    errors += r.status == nat.PRE_ERROR
                    continue
                if c.name != "seeded":
                    continue
                vio = {id(e) for e in r.violating}
                kinds = {id(v) in vio for v in r.victims}
                both += kinds == {True, False}
                late += any(id(v) in vio and v.pos >= 64 for v in r.victims)
                quota_only += r.quota_only_first_pass
                if r0.status == nat.PRE_CANDIDATE:
                    differs += {v.pos for v in r.victims} != {v.pos for v in r0.victims}
        pick, _, st = ppc.ref_arrays(ref)
        moved += int((pick[:, 0] != pc.ref_arrays(plain)[0][:, 0]).sum())
        steps += st.tolist()
    c = ppc.seeded()
    print("seeded: both kinds", both, "victim sets that differ", differs, "violating victims at position >= 64", late,
          "quota-only first-pass victims", quota_only, "exempt pairs", c.n_exempt, "| all cases: errors", errors,
          "picks moved", moved, "steps", steps)
    assert both >= 1 and differs >= 1 and late >= 1 and quota_only >= 1 and errors >= 1
    assert moved >= 1 and ppr.STEP_VIOLATING in steps
    for w in ppc.wide_cases():   # each by itself: the pick moves, n_violating decides it, and it decides across the shards
        ref, plain = ppc.reference(w.name), _plain_reference(w)
        pick, _, st = ppc.ref_arrays(ref)
        assert len(w.ref_rows) == 1_100 and int(st[0]) == ppr.STEP_VIOLATING, w.name
        assert (int(pick[0, 0]), int(pc.ref_arrays(plain)[0][0, 0])) == (w.want["node"], w.want["plain_node"]), w.name
        parts = [ppc.ref_arrays(ref, lo, hi)[0] for lo, hi in ((0, 1_024), (1_024, 1_100))]
        assert parts[0][0, 0] >= 0 and parts[1][0, 0] >= 0 and parts[0][0, 1] >> 32 != parts[1][0, 1] >> 32, w.name
        np.testing.assert_array_equal(engine.merge_preempt([{"pick": x} for x in parts])["pick"], pick)
    assert c.n_exempt >= 1 and {0, 1, 2} <= {len(x) for x in c.pdb_ids} and {0, 1, 1000} <= set(c.allowed.tolist())
    # the hand cases decide what they are named for
    for h in ppc.hand_cases() + ppc.wide_cases():
        res = ppc.reference(h.name)[0]
        words, step = ppr.pick_words(res)
        assert (words[0], step) == (h.want["node"], h.want["step"]), h.name
        assert words[1] >> 32 == h.want["n_violating"], h.name
        if "n_victims" in h.want:
            assert words[1] & 0xFFFFFFFF == h.want["n_victims"], h.name
    r = ppc.reference("violating_decides")[0]
    plain_pick = pr.pick_one([(j, *pr.stats_of(x)[:4]) for j, x in enumerate(r)])
    assert plain_pick == (0, 2) and r[0].n_violating == 1   # without the step node 0 wins at the next criterion (hi_prio)
    q = ppc.reference("quota_only_uncounted")[0][0]
    assert q.quota_only_first_pass == 1 and len(q.victims) == 1 and q.n_violating == 0 and len(q.violating) == 1
    z = ppc.reference("budget_zero")[0][0]
    assert z.n_violating == 2 and len(z.violating) == 2
    d = ppc.reference("hi_prio_divergence")[0][0]
    h = ppc.case("hi_prio_divergence")
    assert d.victims[0].prio == h.want["first_victim_prio"] and pr.stats_of(d)[1] == h.want["hi_prio"]
    e = ppc.reference("error_first_pass")[0]
    assert e[0].status == nat.PRE_ERROR and e[1].status == nat.PRE_ERROR


def _literal_check(prio, start, quota, non_pre, ids, allowed, got):
    """got[b] < P  <=>  the budget walk calls pod b violating, for every preemptor priority that can tell two pods
    apart and every group of the list."""
    levels = sorted({int(p) for p in prio} | {int(p) + 1 for p in prio})
    seen = 0
    for g in sorted({int(x) for x in quota}):
        for pp in levels:
            want = ppr.literal_thresholds(prio, start, quota, non_pre, ids, allowed, pp, g)
            mine = (got < pp) & (np.asarray(quota) == g)
            np.testing.assert_array_equal(mine, want, err_msg=f"priority {pp} group {g}")
            seen += int(want.sum())
    return seen


def test_thresholds_match_the_budget_walk_seeded():
    c = ppc.seeded()
    th = ppc.thresholds("seeded")
    non_pre = (c.b_rows["flags"] & nat.POD_NON_PREEMPTIBLE) != 0
    assert (th[non_pre] == INT32_MAX).all()
    seen = 0
    for j in range(len(c.rows)):
        lo, hi = int(c.first[j]), int(c.first[j + 1])
        if hi > lo:
            seen += _literal_check(c.b_prio[lo:hi], c.b_start[lo:hi], c.b_rows["quota"][lo:hi], non_pre[lo:hi], c.pdb_ids[lo:hi],
                                   c.allowed, th[lo:hi])
    assert seen > 1_000


def test_thresholds_match_the_budget_walk_random():
    """Small random lists: negative and zero budgets, pods under up to three PDBs, ties in priority and start."""
    rng = np.random.default_rng(20_240)
    seen = 0
    for _ in range(400):
        n = int(rng.integers(0, 13))
        prio = rng.choice([-5, 0, 0, 10, 10, 99, INT32_MAX - 1], n).astype(np.int32)
        start = rng.integers(0, 3, n).astype(np.int64)
        quota = rng.integers(-1, 2, n).astype(np.int32)
        non_pre = rng.random(n) < 0.15
        allowed = rng.integers(-2, 4, 3).astype(np.int32)
        ids = [sorted(rng.choice(3, int(rng.integers(0, 4)), replace=False).tolist()) for _ in range(n)]
        first = np.zeros(n + 1, np.int32)
        first[1:] = np.cumsum([len(x) for x in ids])
        got = engine.pdb_thresholds(prio, start, quota, non_pre, first, [i for x in ids for i in x], allowed)
        assert (got[non_pre] == INT32_MAX).all()
        seen += _literal_check(prio, start, quota, non_pre, ids, allowed, got)
    assert seen > 500


def row_preempt_pdb_all(c, th):
    """kg_row_preempt_pdb over every pair of a case -> (status [P][N], mask [P][N][2] u64, stats [P][N][5] i64);
    th None: NULL thresholds."""
    L = nat.lib()
    P, N = len(c.pods), len(c.ref_rows)
    rows, pods = np.ascontiguousarray(c.ref_rows), np.ascontiguousarray(c.pods)
    b_rows, b_prio, b_start = (np.ascontiguousarray(a) for a in (c.b_rows, c.b_prio, c.b_start))
    th = None if th is None else np.ascontiguousarray(th, dtype=np.int32)
    status = np.zeros((P, N), np.int32)
    mask = np.zeros((P, N, 2), np.uint64)
    stats = np.zeros((P, N, 5), np.int64)
    st = ctypes.c_int32(0)
    q = None if c.quotas is None else np.ascontiguousarray(c.quotas)
    qp, nq = (nat.ptr(q), len(q)) if q is not None else (None, 0)
    cfg_p = nat.ptr(c.cfg)
    for i in range(P):
        for j in range(N):
            lo, n = int(c.first[j]), int(c.first[j + 1] - c.first[j])
            rc = L.kg_row_preempt_pdb(cfg_p, rows.ctypes.data + j * rows.itemsize, b_rows.ctypes.data + lo * b_rows.itemsize,
                                      b_prio.ctypes.data + 4 * lo, b_start.ctypes.data + 8 * lo,
                                      None if th is None else th.ctypes.data + 4 * lo, n,
                                      pods.ctypes.data + i * pods.itemsize, int(c.pod_prio[i]), qp, nq, int(c.now_ns),
                                      ctypes.byref(st), mask[i, j].ctypes.data, stats[i, j].ctypes.data)
            assert rc == 0, (i, j, rc)
            status[i, j] = st.value
    return status, mask, stats


@pytest.mark.parametrize("name", [c.name for c in ppc.cases()])
def test_row_preempt_pdb_matches_reference(name):
    c = ppc.case(name)
    ref = ppc.reference(name)
    status, mask, stats = row_preempt_pdb_all(c, ppc.thresholds(name))
    assert status.shape == (len(c.pods), len(c.ref_rows))   # every pair
    want_status = np.array([[r.status for r in res] for res in ref], np.int32)
    want = np.array([[pr.stats_of(r) + (ppr.n_violating_of(r),) for r in res] for res in ref], dtype=object)
    np.testing.assert_array_equal(status, want_status)
    np.testing.assert_array_equal(stats[:, :, :4], want[:, :, :4].astype(np.int64))
    np.testing.assert_array_equal(stats[:, :, 4], want[:, :, 6].astype(np.int64))
    np.testing.assert_array_equal(mask.astype(object), want[:, :, 4:6])


def test_without_thresholds_it_is_the_plain_form():
    """NULL thresholds and all-INT32_MAX thresholds both equal kg_row_preempt (the no-PDB reference), n_violating 0."""
    c = ppc.seeded()
    plain = pc.reference("seeded")[:ppc.N_PRE]
    want_status = np.array([[r.status for r in res] for res in plain], np.int32)
    want = np.array([[pr.stats_of(r) for r in res] for res in plain], dtype=object)
    for th in (None, np.full(len(c.b_rows), INT32_MAX, np.int32)):
        status, mask, stats = row_preempt_pdb_all(c, th)
        np.testing.assert_array_equal(status, want_status)
        np.testing.assert_array_equal(stats[:, :, :4], want[:, :, :4].astype(np.int64))
        assert not stats[:, :, 4].any()
        np.testing.assert_array_equal(mask.astype(object), want[:, :, 4:])
    j, i = 16, 7
    lo, hi = int(c.first[j]), int(c.first[j + 1])
    a = engine.row_preempt(c.cfg, c.ref_rows[j:j + 1], c.b_rows[lo:hi], c.b_prio[lo:hi], c.b_start[lo:hi], c.pods[i:i + 1],
                           int(c.pod_prio[i]), c.now_ns, quotas=c.quotas)
    b = engine.row_preempt_pdb(c.cfg, c.ref_rows[j:j + 1], c.b_rows[lo:hi], c.b_prio[lo:hi], c.b_start[lo:hi], None,
                               c.pods[i:i + 1], int(c.pod_prio[i]), c.now_ns, quotas=c.quotas)
    assert b.pop("n_violating") == 0
    assert a["status"] == b["status"] and (a["victims"] == b["victims"]).all()
    assert all(a[k] == b[k] for k in ("n_victims", "hi_prio", "prio_sum", "earliest_ns"))


def test_wrapper_on_a_node_with_both_kinds():
    c = ppc.seeded()
    ref = ppc.reference("seeded")
    th = ppc.thresholds("seeded")
    i, j = next((i, j) for i, res in enumerate(ref) for j, r in enumerate(res)
                if r.status == nat.PRE_CANDIDATE and 0 < r.n_violating < len(r.victims))
    lo, hi = int(c.first[j]), int(c.first[j + 1])
    got = engine.row_preempt_pdb(c.cfg, c.ref_rows[j:j + 1], c.b_rows[lo:hi], c.b_prio[lo:hi], c.b_start[lo:hi], th[lo:hi],
                                 c.pods[i:i + 1], int(c.pod_prio[i]), c.now_ns, quotas=c.quotas)
    assert got["n_violating"] == ref[i][j].n_violating and got["n_victims"] == len(ref[i][j].victims)
    # the reference's victim list from the mask - the violating victims in importance order, the others
    pos = np.flatnonzero(got["victims"])
    key = lambda b: (-int(c.b_prio[lo + b]), int(c.b_start[lo + b]), b)
    pp = int(c.pod_prio[i])
    rebuilt = sorted((b for b in pos if th[lo + b] < pp), key=key) + sorted((b for b in pos if th[lo + b] >= pp), key=key)
    assert rebuilt == [v.pos for v in ref[i][j].victims]


def test_argument_errors():
    L = nat.lib()
    prio, start = np.array([5, 3], np.int32), np.array([1, 2], np.int64)
    quota, non_pre = np.array([0, 0], np.int32), np.zeros(2, np.uint8)
    first, ids, allowed = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([0, 0], np.int32)
    out = np.zeros(2, np.int32)

    def call(prio=prio, start=start, quota=quota, non_pre=non_pre, n=2, first=first, ids=ids, allowed=allowed, n_pdbs=2, out=out):
        return L.kg_pdb_thresholds(nat.ptr(prio), nat.ptr(start), nat.ptr(quota), nat.ptr(non_pre), n, nat.ptr(first),
                                   nat.ptr(ids), nat.ptr(allowed), n_pdbs, nat.ptr(out))

    assert call() == 0 and out.tolist() == [5, 3]
    for k in ("prio", "start", "quota", "non_pre", "first", "ids", "allowed", "out"):
        assert call(**{k: None}) == ERR_INVALID_ARG, k
    assert call(n=-1) == ERR_RANGE and call(n=129) == ERR_RANGE and call(n_pdbs=-1) == ERR_RANGE
    assert call(first=np.array([0, 2, 1], np.int32)) == ERR_RANGE and call(first=np.array([1, 1, 2], np.int32)) == ERR_RANGE
    assert call(ids=np.array([0, 2], np.int32)) == ERR_RANGE and call(ids=np.array([-1, 0], np.int32)) == ERR_RANGE
    assert call(n_pdbs=1) == ERR_RANGE
    assert call(n=0, prio=None, start=None, quota=None, non_pre=None, out=None, first=np.zeros(1, np.int32), ids=None) == 0
    # kg_row_preempt_pdb: kg_row_preempt's checks
    c = ppc.seeded()
    j, i = 16, 7
    lo, hi = int(c.first[j]), int(c.first[j + 1])
    st, mask, stats = ctypes.c_int32(0), np.zeros(2, np.uint64), np.zeros(5, np.int64)
    node, pod = np.ascontiguousarray(c.ref_rows[j:j + 1]), np.ascontiguousarray(c.pods[i:i + 1])
    b = [np.ascontiguousarray(x[lo:hi]) for x in (c.b_rows, c.b_prio, c.b_start, ppc.thresholds("seeded"))]
    q = np.ascontiguousarray(c.quotas)

    def row(cfg=c.cfg, node=node, n=hi - lo, stats=stats, nq=len(q), rows=b[0]):
        return L.kg_row_preempt_pdb(nat.ptr(cfg), nat.ptr(node), nat.ptr(rows), nat.ptr(b[1]), nat.ptr(b[2]), nat.ptr(b[3]), n,
                                    nat.ptr(pod), 1_000, nat.ptr(q), nq, int(c.now_ns), ctypes.byref(st), nat.ptr(mask),
                                    nat.ptr(stats))

    assert row() == 0
    assert row(node=None) == ERR_INVALID_ARG and row(stats=None) == ERR_INVALID_ARG and row(rows=None) == ERR_INVALID_ARG
    assert row(n=-1) == ERR_RANGE and row(n=129) == ERR_RANGE and row(nq=int(pod["quota"][0])) == ERR_RANGE
    numa = c.cfg.copy()
    numa["enabled_plugins"] |= nat.PLUGIN_NUMA
    assert row(cfg=numa) == ERR_UNSUPPORTED


def test_merge_with_the_new_order():
    """kg_preempt_merge over the reference's picks of node ranges equals the pick over the whole (the n_violating step
    included), and on hand-made words the step sits after "no victim" and before hi_prio."""
    for c in ppc.cases():
        ref = ppc.reference(c.name)
        N = len(c.ref_rows)
        whole = ppc.ref_arrays(ref)[0]
        cuts = [0, 1_024, N] if N > 1_024 else [0, 1, N]
        parts = [{"pick": ppc.ref_arrays(ref, lo, hi)[0]} for lo, hi in zip(cuts[:-1], cuts[1:])]
        for order in (parts, parts[::-1]):
            got = engine.merge_preempt(order)
            np.testing.assert_array_equal(got["pick"], whole)
            np.testing.assert_array_equal(got["n_violating"], whole[:, 1] >> 32)
            np.testing.assert_array_equal(got["n_victims"], whole[:, 1] & 0xFFFFFFFF)
    w = lambda node, nv, nvio, hi: np.array([[[node, nv | nvio << 32, hi, nv * (hi + (1 << 31)), 5, 1 << node, 0, 1]]], np.int64)
    m = lambda *lists: engine.merge_preempt([{"pick": x[0]} for x in lists])
    assert m(w(3, 1, 1, 10), w(7, 2, 0, 900))["node"][0] == 7       # fewer violating beats hi_prio, sum and count
    assert m(w(3, 0, 0, 0), w(7, 2, 0, 900))["node"][0] == 3        # no victim first
    assert m(w(3, 2, 2, 10), w(7, 0, 0, 0))["node"][0] == 7
    assert m(w(3, 1, 1, 10), w(7, 1, 1, 9))["node"][0] == 7         # equal n_violating: the old order
    got = m(w(9, 3, 2, 10), w(4, 3, 2, 10))
    assert (got["node"][0], got["n_violating"][0], got["n_victims"][0], got["n_candidates"][0]) == (4, 2, 3, 2)


def _pod_obj(name, ns, node, priority, labels, start="2024-01-01T00:00:05Z"):
    return {"metadata": {"namespace": ns, "name": name, "uid": f"{ns}-{name}", "labels": labels},
            "spec": {"priority": priority, "nodeName": node,
                     "containers": [{"resources": {"requests": {"cpu": "1", "memory": "1Gi"}}}]},
            "status": {"phase": "Running", "startTime": start}}


def _pdb(ns, selector, allowed, disrupted=()):
    return {"metadata": {"namespace": ns, "name": "pdb"}, "spec": {"selector": selector},
            "status": {"disruptionsAllowed": allowed, "disruptedPods": {n: "2024-01-01T00:00:00Z" for n in disrupted}}}


def test_ingest_bound_pdb():
    from koordinator_amd.config import make_config
    nodes = [{"metadata": {"name": n}, "status": {"allocatable": {"cpu": "8", "memory": "32Gi", "pods": "110"}}}
             for n in ("n0", "n1")]
    web = {"app": "web"}
    pods = [_pod_obj("a", "default", "n0", 10, web), _pod_obj("b", "default", "n0", 5, web),
            _pod_obj("other-ns", "prod", "n0", 5, web), _pod_obj("bare", "default", "n0", 5, {}),
            _pod_obj("gone", "default", "n0", 5, web), _pod_obj("db", "default", "n1", 7, {"app": "db", "tier": "x"}),
            _pod_obj("db2", "default", "n1", 6, {"app": "db"})]
    cfg = make_config(plugins=("NodeResourcesFit", "ElasticQuota"))
    cl = ingest.cluster_from_objects(nodes, pods)
    first, rows, prio, start = ingest.bound_pods(cfg, cl)
    np.testing.assert_array_equal(first, [0, 5, 7])
    none = [INT32_MAX] * 7
    pdbs = [_pdb("default", {"matchLabels": web}, 0, disrupted=("gone",))]
    # budget 0: a and b violate from their own priority on; the other namespace, the label-less pod and the disrupted
    # pod are not covered
    np.testing.assert_array_equal(ingest.bound_pdb(cfg, cl, pdbs), [10, 5] + none[2:])
    # budget 1: b goes negative once a (priority 10) is a potential victim too
    np.testing.assert_array_equal(ingest.bound_pdb(cfg, cl, [_pdb("default", {"matchLabels": web}, 1)]),
                                  [INT32_MAX, 10, INT32_MAX, INT32_MAX, 5, INT32_MAX, INT32_MAX])
    # nil and empty selectors match nothing; one that does not convert is skipped
    for sel in (None, {}, {"matchLabels": {}, "matchExpressions": []},
                {"matchExpressions": [{"key": "app", "operator": "In", "values": []}]},
                {"matchExpressions": [{"key": "app", "operator": "Near", "values": ["web"]}]}):
        np.testing.assert_array_equal(ingest.bound_pdb(cfg, cl, [_pdb("default", sel, 0)]), none)
    expr = lambda op, values=None: {"matchExpressions": [{"key": "tier", "operator": op, **({"values": values} if values else {})}]}
    by_op = {"Exists": [7, INT32_MAX], "DoesNotExist": [INT32_MAX, 6]}
    for op, want in by_op.items():
        got = ingest.bound_pdb(cfg, cl, [_pdb("default", {"matchLabels": {"app": "db"}, **expr(op)}, 0)])
        np.testing.assert_array_equal(got, none[:5] + want)
    got = ingest.bound_pdb(cfg, cl, [_pdb("default", {"matchExpressions": [{"key": "app", "operator": "In", "values": ["db", "x"]}]}, 0)])
    np.testing.assert_array_equal(got, none[:5] + [7, 6])
    got = ingest.bound_pdb(cfg, cl, [_pdb("default", {"matchExpressions": [{"key": "app", "operator": "NotIn", "values": ["web"]}]}, 0)])
    np.testing.assert_array_equal(got, none[:5] + [7, 6])   # (the label-less pod is never covered)
    assert len(ingest.bound_pdb(cfg, cl, [])) == 7 and (ingest.bound_pdb(cfg, cl, []) == INT32_MAX).all()
