"""kg_row_preempt (the host entry of the preemption dry run) and kg_preempt_merge against tests/preempt_ref.py, the
conditions the cases of tests/preempt_cases.py must meet, ingest.bound_pods, and the unchanged ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import preempt_cases as pc
import preempt_ref as pr
from koordinator_amd import _native as nat
from koordinator_amd import engine, ingest

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "koord_gpu.h")
# kg_struct_size of every kg_struct_id at ABI 13 (tests/test_why_cpu.py): the preemption entries add functions and macros
STRUCT_SIZES_ABI13 = [104, 1120, 208, 184, 632, 120, 16, 840, 160, 432, 992, 48, 1776, 240, 424, 320, 24, 64, 24]
NEW_FUNCTIONS = ("kg_bound_set", "kg_bound_update", "kg_bound_download", "kg_row_preempt", "kg_preempt", "kg_preempt_merge")
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_RANGE = -1, -3, -4


def test_header_native_and_library_agree():
    L = nat.lib()
    text = open(HEADER).read()
    for fn in NEW_FUNCTIONS:
        assert fn in nat.EXPORTED and getattr(L, fn) is not None
        assert re.search(rf"\b{fn}\s*\(", text), fn
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (KG_\w+) (\d+)\b", text)}
    assert (consts["KG_PRE_CANDIDATE"], consts["KG_PRE_ABSENT"], consts["KG_PRE_NO_VICTIMS"], consts["KG_PRE_UNFIT"],
            consts["KG_PRE_ERROR"]) == (nat.PRE_CANDIDATE, nat.PRE_ABSENT, nat.PRE_NO_VICTIMS, nat.PRE_UNFIT, nat.PRE_ERROR)
    assert consts["KG_BOUND_MAX_PER_NODE"] == nat.BOUND_MAX_PER_NODE == 128
    assert consts["KG_PREEMPT_MAX_PODS"] == nat.PREEMPT_MAX_PODS == 64
    assert consts["KG_PREEMPT_PICK_WORDS"] == nat.PREEMPT_PICK_WORDS == 8
    assert nat.START_NS_NONE == np.iinfo(np.int64).max


def test_abi_is_unchanged():
    L = nat.lib()
    assert L.kg_abi_version() == 13 and nat.ABI_VERSION == 13
    assert len(nat.STRUCT_IDS) == len(STRUCT_SIZES_ABI13)   # KG_SID_COUNT: no new ABI struct
    assert [L.kg_struct_size(sid) for sid in range(len(STRUCT_SIZES_ABI13) + 1)] == STRUCT_SIZES_ABI13 + [-1]


def test_case_conditions():
    """What the cases must exercise, from the reference alone."""
    seen_status, steps = set(), set()
    quota_victims = reprieved_first = errors = 0
    none = zero = False
    for c in pc.cases():
        ref = pc.reference(c.name)
        pick, cells, st = pc.ref_arrays(ref)
        seen_status |= set(np.unique(cells & 0xFF).tolist())
        steps |= set(st.tolist())
        for res in ref:
            quota_victims += sum(r.quota_victims for r in res)
            reprieved_first += sum(r.reprieved_before_victim for r in res)
            errors += sum(r.status == nat.PRE_ERROR for r in res)
        none = none or bool((pick[:, 0] < 0).any())
        zero = zero or bool(((pick[:, 0] >= 0) & (pick[:, 1] == 0)).any())
    print("statuses", seen_status, "steps", steps, "quota victims", quota_victims, "reprieved before a victim",
          reprieved_first, "errors", errors)
    assert seen_status == {nat.PRE_CANDIDATE, nat.PRE_ABSENT, nat.PRE_NO_VICTIMS, nat.PRE_UNFIT, nat.PRE_ERROR}
    assert errors >= 1 and quota_victims >= 1 and reprieved_first >= 1
    assert {1, 2, 3, 4, 5, 6} <= steps
    assert none and zero
    # the seeded table: the mask-word edges, victims past bit 63, the clamps
    s = pc.seeded()
    lengths = np.diff(s.first)
    assert {0, 1, 63, 64, 65, 127, 128} <= set(lengths.tolist()) and 5 < lengths.mean() < 8
    assert any(v.pos >= 64 for res in pc.reference("seeded") for r in res for v in r.victims)
    sums = np.add.reduceat(s.b_rows["request"][:, nat.RES_CPU], s.first[:-1][lengths > 0])
    assert (sums > s.rows["requested"][lengths > 0, nat.RES_CPU]).any()
    assert ((s.b_rows["flags"] & nat.POD_NON_PREEMPTIBLE) != 0).any() and (s.b_start == nat.START_NS_NONE).any()
    for h in pc.hand_cases():
        p, _, st = pc.ref_arrays(pc.reference(h.name))
        assert (int(p[0, 0]), int(st[0])) == (h.want_node, h.want_step), h.name


def row_preempt_all(c):
    """kg_row_preempt over every pair of a case -> (status [P][N], mask [P][N][2] u64, stats [P][N][4] i64)."""
    L = nat.lib()
    P, N = len(c.pods), len(c.ref_rows)
    rows, pods = np.ascontiguousarray(c.ref_rows), np.ascontiguousarray(c.pods)
    b_rows, b_prio, b_start = (np.ascontiguousarray(a) for a in (c.b_rows, c.b_prio, c.b_start))
    status = np.zeros((P, N), np.int32)
    mask = np.zeros((P, N, 2), np.uint64)
    stats = np.zeros((P, N, 4), np.int64)
    st = ctypes.c_int32(0)
    q = None if c.quotas is None else np.ascontiguousarray(c.quotas)
    qp, nq = (nat.ptr(q), len(q)) if q is not None else (None, 0)
    cfg_p = nat.ptr(c.cfg)
    for i in range(P):
        for j in range(N):
            lo, n = int(c.first[j]), int(c.first[j + 1] - c.first[j])
            rc = L.kg_row_preempt(cfg_p, rows.ctypes.data + j * rows.itemsize, b_rows.ctypes.data + lo * b_rows.itemsize,
                                  b_prio.ctypes.data + 4 * lo, b_start.ctypes.data + 8 * lo, n,
                                  pods.ctypes.data + i * pods.itemsize, int(c.pod_prio[i]), qp, nq, int(c.now_ns),
                                  ctypes.byref(st), mask[i, j].ctypes.data, stats[i, j].ctypes.data)
            assert rc == 0, (i, j, rc)
            status[i, j] = st.value
    return status, mask, stats


@pytest.mark.parametrize("name", [c.name for c in pc.cases()])
def test_row_preempt_matches_reference(name):
    c = next(x for x in pc.cases() if x.name == name)
    ref = pc.reference(name)
    status, mask, stats = row_preempt_all(c)
    want_status = np.array([[r.status for r in res] for res in ref], np.int32)
    want = np.array([[pr.stats_of(r) for r in res] for res in ref], dtype=object)
    np.testing.assert_array_equal(status, want_status)
    np.testing.assert_array_equal(stats, want[:, :, :4].astype(np.int64))
    np.testing.assert_array_equal(mask.astype(object), want[:, :, 4:])


def test_row_preempt_wrapper_and_argument_errors():
    c = pc.seeded()
    j = 16   # the 128-pod list
    lo, hi = int(c.first[j]), int(c.first[j + 1])
    ref = pc.reference("seeded")
    i = 7
    got = engine.row_preempt(c.cfg, c.ref_rows[j:j + 1], c.b_rows[lo:hi], c.b_prio[lo:hi], c.b_start[lo:hi], c.pods[i:i + 1],
                             int(c.pod_prio[i]), c.now_ns, quotas=c.quotas)
    nv, hp, ps, es, m0, m1 = pr.stats_of(ref[i][j])
    assert (got["status"], got["n_victims"], got["hi_prio"], got["prio_sum"], got["earliest_ns"]) == (ref[i][j].status, nv, hp, ps, es)
    assert sorted(np.flatnonzero(got["victims"]).tolist()) == sorted(v.pos for v in ref[i][j].victims)
    L = nat.lib()
    st, mask, stats = ctypes.c_int32(0), np.zeros(2, np.uint64), np.zeros(4, np.int64)
    node, pod = np.ascontiguousarray(c.ref_rows[j:j + 1]), np.ascontiguousarray(c.pods[i:i + 1])
    b = (np.ascontiguousarray(c.b_rows[lo:hi]), np.ascontiguousarray(c.b_prio[lo:hi]), np.ascontiguousarray(c.b_start[lo:hi]))
    q = np.ascontiguousarray(c.quotas)

    def call(cfg=c.cfg, node=node, rows=b[0], prio=b[1], start=b[2], n=hi - lo, pod=pod, quotas=q, nq=len(q), status=st,
             mask=mask, stats=stats):
        return L.kg_row_preempt(nat.ptr(cfg), nat.ptr(node), nat.ptr(rows), nat.ptr(prio), nat.ptr(start), n, nat.ptr(pod), 1_000,
                                nat.ptr(quotas), nq, int(c.now_ns), ctypes.byref(status) if status is not None else None,
                                nat.ptr(mask), nat.ptr(stats))

    assert call() == 0
    assert call(node=None) == ERR_INVALID_ARG and call(pod=None) == ERR_INVALID_ARG and call(status=None) == ERR_INVALID_ARG
    assert call(mask=None) == ERR_INVALID_ARG and call(stats=None) == ERR_INVALID_ARG and call(rows=None) == ERR_INVALID_ARG
    assert call(quotas=None) == ERR_INVALID_ARG   # n_quotas > 0 without the groups
    assert call(n=-1) == ERR_RANGE and call(n=129) == ERR_RANGE
    assert call(nq=int(pod["quota"][0])) == ERR_RANGE   # the pod's group is past the list
    assert call(n=0, rows=None, prio=None, start=None) == 0 and st.value == nat.PRE_NO_VICTIMS
    numa = c.cfg.copy()
    numa["enabled_plugins"] |= nat.PLUGIN_NUMA
    assert call(cfg=numa) == ERR_UNSUPPORTED


def test_merge_on_shard_splits():
    """kg_preempt_merge over the reference's picks of node ranges equals the pick over the whole; overlapping ranges
    (the same node in two lists: a full tie) change nothing but the summed candidate count."""
    for c in pc.cases():
        ref = pc.reference(c.name)
        N = len(c.ref_rows)
        whole = {"pick": pc.ref_arrays(ref)[0]}
        cuts = [0, 1_024, N] if N > 1_024 else [0, 1, N]
        parts = [{"pick": pc.ref_arrays(ref, lo, hi)[0]} for lo, hi in zip(cuts[:-1], cuts[1:])]
        for order in (parts, parts[::-1]):
            np.testing.assert_array_equal(engine.merge_preempt(order)["pick"], whole["pick"])
        three = [{"pick": pc.ref_arrays(ref, lo, hi)[0]} for lo, hi in ((0, N // 3), (N // 3, N // 2), (N // 2, N))]
        np.testing.assert_array_equal(engine.merge_preempt(three)["pick"], whole["pick"])
        over = engine.merge_preempt([whole, parts[-1], whole])["pick"]
        np.testing.assert_array_equal(over[:, :7], whole["pick"][:, :7])
        has = whole["pick"][:, 0] >= 0
        np.testing.assert_array_equal(over[has, 7], 2 * whole["pick"][has, 7] + parts[-1]["pick"][has, 7])
        got = engine.merge_preempt([whole])
        np.testing.assert_array_equal(got["node"], whole["pick"][:, 0])
        np.testing.assert_array_equal(got["n_candidates"], whole["pick"][:, 7])
    L = nat.lib()
    one = np.zeros((1, 1, 8), np.int64)
    out = np.zeros((1, 8), np.int64)
    assert L.kg_preempt_merge(nat.ptr(one), 0, 1, nat.ptr(out)) == ERR_INVALID_ARG
    assert L.kg_preempt_merge(nat.ptr(one), 1, -1, nat.ptr(out)) == ERR_INVALID_ARG
    assert L.kg_preempt_merge(None, 1, 1, nat.ptr(out)) == ERR_INVALID_ARG
    assert L.kg_preempt_merge(nat.ptr(one), 1, 1, None) == ERR_INVALID_ARG


def _pod_obj(name, node, cpu, priority=None, start=None, phase="Running"):
    status = {"phase": phase}
    if start:
        status["startTime"] = start
    return {"metadata": {"namespace": "default", "name": name, "uid": name},
            "spec": {"priority": priority, "nodeName": node,
                     "containers": [{"resources": {"requests": {"cpu": cpu, "memory": "1Gi"}}}]},
            "status": status}


def test_ingest_bound_pods():
    from koordinator_amd.config import make_config
    nodes = [{"metadata": {"name": n}, "status": {"allocatable": {"cpu": "8", "memory": "32Gi", "pods": "110"}}}
             for n in ("n0", "n1", "n2")]
    pods = [_pod_obj("a", "n1", "500m", 100, "2024-01-01T00:00:10Z"), _pod_obj("b", "n0", "1", None, "2024-01-01T00:00:05Z"),
            _pod_obj("c", "n1", "2", 7), _pod_obj("done", "n1", "1", 5, "2024-01-01T00:00:01Z", phase="Succeeded"),
            _pod_obj("pending", "", "1", 5)]
    cfg = make_config(plugins=("NodeResourcesFit", "ElasticQuota"))
    cl = ingest.cluster_from_objects(nodes, pods)
    first, rows, prio, start = ingest.bound_pods(cfg, cl)
    np.testing.assert_array_equal(first, [0, 1, 3, 3])   # n0: b; n1: a, c (the terminated pod is left out); n2: none
    np.testing.assert_array_equal(rows["request"][:, nat.RES_CPU], [1000, 500, 2000])
    np.testing.assert_array_equal(rows["numa_request"][:, nat.RES_CPU], [1000, 500, 2000])
    np.testing.assert_array_equal(prio, [0, 100, 7])
    t = ingest.parse_time_ns("2024-01-01T00:00:00Z")
    np.testing.assert_array_equal(start, [t + 5 * 10**9, t + 10 * 10**9, nat.START_NS_NONE])
    # the rows are what the dry run reads: a 7-core preemptor of priority 50 on n1 evicts c (priority 7), not a
    node_rows = engine.build_node_rows(cfg, cl.view())
    pre = ingest.pod_from_object(_pod_obj("p", "", "7", 50))
    view = cl.view([pre])
    pod_row = engine.build_pod_rows(cfg, view, [view.pod_index(pre)])
    got = engine.row_preempt(cfg, node_rows[1:2], rows[1:3], prio[1:3], start[1:3], pod_row, 50, cl.now_ns)
    assert got["status"] == nat.PRE_CANDIDATE and np.flatnonzero(got["victims"]).tolist() == [1]
    assert (got["hi_prio"], got["prio_sum"], got["earliest_ns"]) == (7, 7 + (1 << 31), nat.START_NS_NONE)


class _TableStub:
    """What SnapshotFeeder.flush needs of an engine, keeping the bound-pod lists it is sent."""

    def __init__(self, first, rows, prio, start):
        self.bound_max = nat.BOUND_MAX_PER_NODE
        self.lists = {j: (rows[first[j]:first[j + 1]], prio[first[j]:first[j + 1]], start[first[j]:first[j + 1]])
                      for j in range(len(first) - 1)}

    def upsert(self, idx, rows):
        pass

    def set_cpus(self, view, view_index, snap_index):
        pass

    def remove(self, i):
        pass

    def update_bound_pods(self, node, rows, prio, start):
        self.lists[node] = (np.array(rows), np.asarray(prio, np.int32), np.asarray(start, np.int64))


def test_feeder_keeps_the_table_in_step():
    """Event stream -> kg_bound_update calls equals the table of a fresh feeder that saw only the final objects."""
    from koordinator_amd import feeders
    from koordinator_amd.config import make_config
    cfg = make_config(plugins=("NodeResourcesFit", "ElasticQuota"))
    nodes = [{"metadata": {"name": n}, "status": {"allocatable": {"cpu": "8", "memory": "32Gi", "pods": "110"}}}
             for n in ("n0", "n1", "n2")]
    a, b, c2, d = (_pod_obj("a", "n0", "1", 10, "2024-01-01T00:00:10Z"), _pod_obj("b", "n0", "2", 5, "2024-01-01T00:00:05Z"),
                   _pod_obj("c", "n1", "1", None), _pod_obj("d", "n2", "500m", 7, "2024-01-01T00:00:07Z"))
    f = feeders.SnapshotFeeder(cfg, now_fn=lambda: 1_700_000_000 * 10**9)
    for n in nodes:
        f.on_node_add(n)
    for p in (a, b, c2):
        f.on_pod_add(p)
    stub = _TableStub(*f.bound_pods())
    f.flush(stub)
    np.testing.assert_array_equal(stub.lists[0][1], [10, 5])
    # a bind, a delete, a termination and a node that goes away
    f.on_pod_add(d)
    f.on_pod_delete(b)
    done = _pod_obj("c", "n1", "1", None, phase="Succeeded")
    f.on_pod_update(c2, done)
    e = _pod_obj("e", "n0", "250m", 3)
    f.on_pod_add(e)
    f.flush(stub)
    fresh = feeders.SnapshotFeeder(cfg, now_fn=lambda: 1_700_000_000 * 10**9)
    for n in nodes:
        fresh.on_node_add(n)
    for p in (a, done, d, e):
        fresh.on_pod_add(p)
    first, rows, prio, start = fresh.bound_pods()
    np.testing.assert_array_equal(first, [0, 2, 2, 3])
    for j in range(3):
        g_rows, g_prio, g_start = stub.lists[j]
        lo, hi = int(first[j]), int(first[j + 1])
        np.testing.assert_array_equal(g_rows, rows[lo:hi])
        np.testing.assert_array_equal(g_prio, prio[lo:hi])
        np.testing.assert_array_equal(g_start, start[lo:hi])
    np.testing.assert_array_equal(stub.lists[0][1], [10, 3])
    f.on_node_delete("n2")
    f.flush(stub)
    assert len(stub.lists[2][0]) == 0
