"""Input sets and references of the kg_row_why / kg_diagnose tests (tests/test_why_*.py).

TEST INFRASTRUCTURE: every case is built once per process; rows and references are handed out read-only.

  edited  cycle_cases.case("la_extra") (1,100 nodes, 96 pods, the nodes BIG beyond the fp64 bounds) on row copies:
          node j % 11 == 0 pod-full, j % 13 == 1 cpu over-requested by 500, j % 17 == 2 one byte of memory left,
          j % 19 == 3 removed; pod 0 asks 10,000 cores, one pod is a daemonset, one has no request at all
  scalar  synth.make_scalar_cluster(1_100, 64, seed=72) under shipped_profile(extended_resources=SCALAR_NAMES): the
          later named slots (resources 8..10), which take the canonical row
  numa    numa_cases.make_numa_edge_cluster(600, 24, seed=7) under numa_config(): NodeNUMAResource's bit, from the oracle
"""
import functools
from types import SimpleNamespace

import numpy as np

import cycle_cases as cc
import why_ref
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile

DAEMON_POD, EMPTY_POD = 5, 7     # the edited case's daemonset pod and its pod without a request
NAMES = ("edited", "scalar", "numa")


def _frozen(a):
    a.setflags(write=False)
    return a


def edit_nodes(rows):
    """The node edits of the `edited` case on a copy; returns (rows, removed node indices)."""
    rows = rows.copy()
    j = np.arange(len(rows))
    full = j % 11 == 0
    rows["pod_count"][full] = rows["allowed_pods"][full]
    over = j % 13 == 1
    rows["requested"][over, nat.RES_CPU] = rows["alloc"][over, nat.RES_CPU] + 500
    tight = j % 17 == 2
    rows["requested"][tight, nat.RES_MEMORY] = rows["alloc"][tight, nat.RES_MEMORY] - 1
    removed = np.flatnonzero(j % 19 == 3)
    return rows, removed


@functools.lru_cache(maxsize=None)
def base(name):
    """(cfg, cluster, node rows, pod rows) before any edit: what the oracle sees at object level."""
    if name == "edited":
        return cc.case("la_extra")
    if name == "scalar":
        cfg = shipped_profile(extended_resources=synth.SCALAR_NAMES)
        cl = synth.make_scalar_cluster(1_100, 64, seed=72)
        n_pods = 64
    else:
        from numa_cases import make_numa_edge_cluster, numa_config
        cfg = numa_config()
        cl = make_numa_edge_cluster(600, 24, seed=7)
        n_pods = 24
    return cfg, cl, _frozen(engine.build_node_rows(cfg, cl)), _frozen(engine.build_pod_rows(cfg, cl, np.arange(n_pods)))


@functools.lru_cache(maxsize=None)
def numa_bad():
    """bool [24][600]: the oracle's NodeNUMAResource Filter rejects the pair (numa case)."""
    from oracle import oracle
    cfg, cl, rows, pods = base("numa")
    out = np.zeros((len(pods), len(rows)), bool)
    for i in range(len(pods)):
        for j in range(len(rows)):
            out[i, j] = not oracle.numa_eval(cfg, cl, i, j)[0]
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def case(name):
    """cfg, now_ns, rows (what the engine loads), removed (nodes the engine removes after the load), ref_rows (the
    reference's rows: the removed nodes with KG_NODE_VALID cleared), pods, numa_bad (None without the plugin)."""
    cfg, cl, rows, pods = base(name)
    removed = np.zeros(0, np.int64)
    pods = pods.copy()
    if name == "edited":
        rows, removed = edit_nodes(rows)
        pods["request"][0, nat.RES_CPU] = 10_000_000
        pods["flags"][DAEMON_POD] |= nat.POD_DAEMONSET
        pods["request"][EMPTY_POD] = 0
        pods["request_present"][EMPTY_POD] = 0
        pods["flags"][EMPTY_POD] &= ~np.uint32(nat.POD_HAS_REQUEST)
    ref_rows = rows.copy()
    ref_rows["flags"][removed] &= ~np.uint32(nat.NODE_VALID)
    return SimpleNamespace(name=name, cfg=cfg, now_ns=cl.now_ns, rows=_frozen(rows.copy()), removed=removed,
                           ref_rows=_frozen(ref_rows), pods=_frozen(pods), numa_bad=numa_bad() if name == "numa" else None)


@functools.lru_cache(maxsize=None)
def reference(name, first_fail=False):
    """[P][N] reason words of the case from why_ref (no eligibility classes)."""
    c = case(name)
    return _frozen(why_ref.why_ref(c.cfg, c.ref_rows, c.pods, c.now_ns, first_fail=first_fail, numa_bad=c.numa_bad))


def engine_of(c, n_nodes=None):
    """An engine holding the case's snapshot (its first n_nodes nodes), the removed nodes removed."""
    eng = engine.Engine(c.cfg)
    n = len(c.rows) if n_nodes is None else n_nodes
    eng.load_snapshot(c.rows[:n])
    for j in c.removed:
        if j < n:
            eng.remove(int(j))
    return eng


def bit_totals(why):
    """{bit: pairs whose word has it} of a word matrix, zero entries left out."""
    why = np.asarray(why, np.uint32)
    return {b: int(((why >> np.uint32(b)) & np.uint32(1)).sum()) for b in range(32) if ((why >> np.uint32(b)) & np.uint32(1)).any()}


def elig_classes(n_nodes):
    """bool [2][n_nodes]: a sparse class (every 7th node) and one that empties whole tiles (nodes 1024.. only)."""
    j = np.arange(n_nodes)
    return np.stack([j % 7 == 0, j >= 1024])


def quota_case():
    """A small ElasticQuota case on the shipped cluster: (cfg, now_ns, rows, pods, quotas).  Group 0 has room, group 1
    is over its cpu limit for any request, group 2 passes on its own and fails through its parent (group 3), group 4
    fails the min gate of non-preemptible pods only."""
    from quota_cases import _rl
    cfg = make_config(plugins=("NodeResourcesFit", "ElasticQuota"), eq_check_parent_quota=1)
    cl = cc.cluster()
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(16))
    big = {"cpu": 1 << 40, "memory": 1 << 50}
    q = np.zeros(5, dtype=nat.QUOTA)
    for g in range(5):
        q[g]["used_limit"] = _rl(big)
        q[g]["min"] = _rl(big)
    q["parent"] = -1
    q[1]["used_limit"] = _rl({"cpu": 1000, "memory": 1 << 50})
    q[1]["used"] = _rl({"cpu": 1000})
    q[2]["parent"] = 3
    q[3]["used_limit"] = _rl({"cpu": 1 << 40, "memory": 4096})
    q[3]["used"] = _rl({"memory": 4096})
    q[4]["min"] = _rl({"cpu": 10, "memory": 1 << 50})
    q[4]["non_preemptible_used"] = _rl({"cpu": 10})
    pods["quota"] = np.array([-1, 0, 1, 2, 4, 4, 3, 1, 0, 2, -1, 4, 0, 1, 2, 3], np.int32)
    pods["flags"][4] |= nat.POD_NON_PREEMPTIBLE
    pods["flags"][11] &= ~np.uint32(nat.POD_NON_PREEMPTIBLE)   # the same group, preemptible: passes
    return cfg, cl.now_ns, rows, pods, q
