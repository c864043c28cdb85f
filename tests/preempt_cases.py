"""Input sets and references of the kg_row_preempt / kg_preempt tests (tests/test_preempt_*.py).

TEST INFRASTRUCTURE: every case is built once per process; arrays and references are handed out read-only.

  seeded  why_cases.case("edited") (1,100 nodes: a full 1,024-node tile and a ragged one; removed, pod-full,
          over-requested and LoadAware-rejected nodes) with ElasticQuota enabled, plus a seeded bound-pod table: about 6
          pods per node, the lengths 0, 1, 63, 64, 65, 127 and 128 planted in both tiles (the mask-word edges), 4 quota
          groups (loose, tight, over its limit, `used` below its victims' sum) and pods without a group, some
          non-preemptible pods, equal priorities with different starts, fully tied entries, pods without a start time,
          nodes whose `requested` is smaller than their list's sum; 32 preemptors over 4 priorities with mixed groups
  hand    2-4-node clusters in which each pick criterion in turn decides, one full tie resolved by the node index,
          and one preemptor without a candidate
"""
import functools
from types import SimpleNamespace

import numpy as np

import preempt_ref as pr
import why_cases as wc
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import make_config

N_PRE = 32
PLANTED = {10: 0, 11: 1, 12: 63, 13: 64, 14: 65, 15: 127, 16: 128, 1030: 64, 1031: 128, 1032: 65, 1033: 1, 1099: 127}
BOUND_PRIOS = (0, 100, 1_000, 5_000)
PRE_PRIOS = (100, 1_000, 5_000, 9_000)
T0 = 1_700_000_000 * 10**9
GROUP_LOOSE, GROUP_TIGHT, GROUP_OVER, GROUP_CLAMP = range(4)


def _frozen(a):
    a.setflags(write=False)
    return a


def _rl(values):
    out = np.zeros((), dtype=nat.RESOURCE_LIST)
    for r, v in values.items():
        out["v"][r] = v
        out["present"] |= 1 << r
    return out


def bound_row(cpu, mem, quota=-1, non_preemptible=False):
    """A bound pod's row: a cpu / memory request (NodeInfo deltas and quota deltas alike)."""
    row = np.zeros((), dtype=nat.POD_ROW)
    row["request"][nat.RES_CPU], row["request"][nat.RES_MEMORY] = cpu, mem
    row["nonzero_request"] = (cpu or 100, mem or 200 * 1024 * 1024)
    row["numa_request"][nat.RES_CPU], row["numa_request"][nat.RES_MEMORY] = cpu, mem
    row["numa_request_present"] = 0b11
    row["flags"] = nat.POD_HAS_REQUEST | nat.POD_VALID | (nat.POD_NON_PREEMPTIBLE if non_preemptible else 0)
    row["quota"] = quota
    return row


def set_request(row, cpu, mem):
    """Overwrite a preemptor's Fit request and quota request with cpu / memory alone."""
    row["request"] = 0
    row["request"][..., nat.RES_CPU], row["request"][..., nat.RES_MEMORY] = cpu, mem
    row["request_present"] = 0
    row["numa_request"] = 0
    row["numa_request"][..., nat.RES_CPU], row["numa_request"][..., nat.RES_MEMORY] = cpu, mem
    row["numa_request_present"] = 0b11
    row["flags"] |= nat.POD_HAS_REQUEST


@functools.lru_cache(maxsize=None)
def seeded():
    c = wc.case("edited")
    cfg = c.cfg.copy()
    cfg["enabled_plugins"] |= nat.PLUGIN_ELASTICQUOTA
    rng = np.random.default_rng(4242)
    N = len(c.rows)
    lengths = np.minimum(rng.poisson(6, N), 20).astype(np.int64)
    lengths[rng.random(N) < 0.04] = 0
    for j, L in PLANTED.items():
        lengths[j] = L
    first = np.zeros(N + 1, np.int32)
    first[1:] = np.cumsum(lengths)
    total = int(first[-1])
    rows = np.zeros(total, dtype=nat.POD_ROW)
    prio = np.zeros(total, np.int32)
    start = np.zeros(total, np.int64)
    req_cpu, req_mem = c.rows["requested"][:, nat.RES_CPU], c.rows["requested"][:, nat.RES_MEMORY]
    for j in range(N):
        L = int(lengths[j])
        if not L:
            continue
        lo = int(first[j])
        # the list carries about 90 % of the row's requested amounts; every 97th node three times as much (the
        # removals then drive `requested` below zero: no clamp on the row, plain int64)
        scale = 2.7 if j % 97 == 5 else 0.9
        w = rng.random(L) + 0.2
        w /= w.sum()
        group_of_node = rng.integers(-1, 4) if rng.random() < 0.5 else None   # half the nodes hold one group only
        for i in range(L):
            g = int(group_of_node) if group_of_node is not None else int(rng.integers(-1, 4))
            rows[lo + i] = bound_row(int(max(req_cpu[j], 0) * scale * w[i]), int(max(req_mem[j], 0) * scale * w[i]), g,
                                     non_preemptible=rng.random() < 0.08)
        prio[lo:lo + L] = rng.choice(BOUND_PRIOS, L)
        # few distinct starts: equal priorities with different starts, and entries tied in both
        start[lo:lo + L] = T0 + rng.integers(0, 4, L) * 10**9
        start[lo:lo + L][rng.random(L) < 0.05] = nat.START_NS_NONE
    # preemptors: the case's own pod rows (their LoadAware variants, daemonset and no-request pods and the 10,000-core
    # pod 0 kept), most with a cpu / memory request sized between the nodes' free amounts and what their lists hold
    pods = c.pods[:N_PRE].copy()
    free_cpu = np.sort((c.rows["alloc"] - c.rows["requested"])[:, nat.RES_CPU])
    alloc_mem = np.median(c.rows["alloc"][:, nat.RES_MEMORY])
    keep = {0, wc.DAEMON_POD, wc.EMPTY_POD}
    for i in range(N_PRE):
        if i not in keep:
            q = (0.35, 0.6, 0.8, 0.93)[i % 4]
            set_request(pods[i:i + 1], int(free_cpu[int(q * (N - 1))]) + 250 * (i % 3), int(alloc_mem * 0.02 * (1 + i % 5)))
        pods["quota"][i] = (i % 5) - 1
        pods["elig_class"][i] = 0
    pods["flags"][3] |= nat.POD_NON_PREEMPTIBLE   # (a preemptor's own flag plays no part in the dry run)
    pod_prio = np.array([PRE_PRIOS[(i // 5) % 4] for i in range(N_PRE)], np.int32)
    pod_prio[wc.EMPTY_POD] = 9_000
    # quota groups: what each one's re-check does to a typical preemptor (cpu of a few cores)
    typ = int(np.median(pods["request"][:, nat.RES_CPU]))
    big = {nat.RES_CPU: 1 << 40, nat.RES_MEMORY: 1 << 50}
    quotas = np.zeros(4, dtype=nat.QUOTA)
    quotas["parent"] = -1
    for g in range(4):
        quotas[g]["used_limit"] = _rl(big)
        quotas[g]["min"] = _rl(big)
    quotas[GROUP_LOOSE]["used"] = _rl({nat.RES_CPU: 50_000, nat.RES_MEMORY: 1 << 36})
    # tight: `used` sits at the limit, so the preemptor is admitted only while victims of its own size stay out
    quotas[GROUP_TIGHT]["used_limit"] = _rl({nat.RES_CPU: 400_000, nat.RES_MEMORY: 1 << 50})
    quotas[GROUP_TIGHT]["used"] = _rl({nat.RES_CPU: 400_000 + typ // 4, nat.RES_MEMORY: 1 << 30})
    # over: no removal on one node brings the group back under its limit
    quotas[GROUP_OVER]["used_limit"] = _rl({nat.RES_CPU: 100_000, nat.RES_MEMORY: 1 << 50})
    quotas[GROUP_OVER]["used"] = _rl({nat.RES_CPU: 1 << 38, nat.RES_MEMORY: 1 << 30})
    # clamp: `used` is smaller than a node's victims, the subtraction stops at zero and the add-backs climb from there
    quotas[GROUP_CLAMP]["used_limit"] = _rl({nat.RES_CPU: 3 * typ, nat.RES_MEMORY: 1 << 50})
    quotas[GROUP_CLAMP]["used"] = _rl({nat.RES_CPU: 10})
    return SimpleNamespace(name="seeded", cfg=cfg, now_ns=c.now_ns, rows=c.rows, removed=c.removed, ref_rows=c.ref_rows,
                           first=_frozen(first), b_rows=_frozen(rows), b_prio=_frozen(prio), b_start=_frozen(start),
                           pods=_frozen(pods), pod_prio=_frozen(pod_prio), quotas=_frozen(quotas), max_per_node=128)


def _node_row(alloc_cpu, bound_cpu, allowed=110):
    row = np.zeros((), dtype=nat.NODE_ROW)
    row["alloc"][nat.RES_CPU], row["alloc"][nat.RES_MEMORY] = alloc_cpu, 1 << 40
    row["requested"][nat.RES_CPU] = sum(bound_cpu)
    row["nonzero_requested"][0] = sum(bound_cpu)
    row["pod_count"], row["allowed_pods"] = len(bound_cpu), allowed
    row["flags"] = nat.NODE_VALID
    return row


def _hand(name, nodes, pod_cpu, pod_prio, want_node, want_step):
    """nodes: [(alloc cpu, [(cpu, priority, start)...])]; one preemptor of `pod_cpu` milli-cores and `pod_prio`."""
    cfg = make_config(plugins=("NodeResourcesFit", "ElasticQuota"))
    rows = np.array([_node_row(a, [b[0] for b in bl]) for a, bl in nodes], dtype=nat.NODE_ROW)
    first = np.zeros(len(nodes) + 1, np.int32)
    first[1:] = np.cumsum([len(bl) for _, bl in nodes])
    flat = [b for _, bl in nodes for b in bl]
    b_rows = np.array([bound_row(b[0], 0) for b in flat], dtype=nat.POD_ROW).reshape(-1)
    b_prio = np.array([b[1] for b in flat], np.int32)
    b_start = np.array([b[2] for b in flat], np.int64)
    pod = np.zeros(1, dtype=nat.POD_ROW)
    set_request(pod[0:1], pod_cpu, 0)
    pod["flags"] |= nat.POD_VALID
    pod["quota"] = -1
    return SimpleNamespace(name=name, cfg=cfg, now_ns=T0, rows=_frozen(rows), removed=np.zeros(0, np.int64), ref_rows=rows,
                           first=_frozen(first), b_rows=_frozen(b_rows), b_prio=_frozen(b_prio), b_start=_frozen(b_start),
                           pods=_frozen(pod), pod_prio=_frozen(np.array([pod_prio], np.int32)), quotas=None, max_per_node=4,
                           want_node=want_node, want_step=want_step)


LOW = -(1 << 31)   # priority + 2^31 = 0: the sums tie whatever the victim counts


@functools.lru_cache(maxsize=None)
def hand_cases():
    return (
        # 1: the pod fits on node 1 all along (its only pod is reprieved); node 0 needs a victim
        _hand("zero_victims", [(4000, [(3000, 0, 5)]), (4000, [(1000, 0, 5)])], 2000, 10, 1, 1),
        # 2: the lowest highest-victim priority
        _hand("hi_prio", [(4000, [(3000, 100, 5)]), (4000, [(3000, 50, 5)]), (4000, [(3000, 70, 5)])], 2000, 500, 1, 2),
        # 3: equal highest priority, the smaller sum (node 0 loses two pods of priority 100, node 1 one)
        _hand("prio_sum", [(4000, [(2000, 100, 5), (2000, 100, 6)]), (4000, [(3500, 100, 5)])], 3000, 500, 1, 3),
        # 4: equal highest priority and equal sums (every term is zero), the fewer victims
        _hand("n_victims", [(4000, [(2000, LOW, 5), (2000, LOW, 6)]), (4000, [(3500, LOW, 5)])], 3000, 500, 1, 4),
        # 5: the latest earliest start among the highest-priority victims
        _hand("earliest", [(4000, [(3000, 100, 10)]), (4000, [(3000, 100, 20)]), (4000, [(3000, 100, 15)])], 2000, 500, 1, 5),
        # 6: a full tie between nodes 1 and 2 (node 0 holds nothing to preempt): the lower index
        _hand("node_index", [(1000, []), (4000, [(3000, 100, 10)]), (4000, [(3000, 100, 10)]), (4000, [(3000, 100, 10), (500, 900, 1)])],
              2000, 500, 1, 6),
        # no candidate: every bound pod outranks the preemptor, or the node is too small whatever leaves
        _hand("none", [(4000, [(3000, 900, 5)]), (1000, [(500, 0, 5)])], 2000, 500, -1, 0),
    )


def cases():
    return (seeded(),) + hand_cases()


@functools.lru_cache(maxsize=None)
def reference(name, elig=False):
    """Per preemptor the per-node results (preempt_ref.dry_run) of a case; `elig`: the seeded pods take eligibility
    classes i % 3 of why_cases.elig_classes."""
    c = next(x for x in cases() if x.name == name)
    pods = elig_pods(c) if elig else c.pods
    classes = wc.elig_classes(len(c.rows)) if elig else None
    return tuple(pr.dry_run(c.cfg, c.ref_rows, c.first, c.b_rows, c.b_prio, c.b_start, pods[i], int(c.pod_prio[i]), c.quotas,
                            c.now_ns, elig=classes) for i in range(len(pods)))


def elig_pods(c):
    pods = c.pods.copy()
    pods["elig_class"] = np.arange(len(pods)) % 3
    return pods


def ref_arrays(results, lo=0, hi=None):
    """(pick [n][8] int64, cells [n][hi - lo] uint32, deciding steps [n]) of per-preemptor results over nodes [lo, hi)."""
    hi = len(results[0]) if hi is None else hi
    pick = np.zeros((len(results), nat.PREEMPT_PICK_WORDS), np.int64)
    cells = np.zeros((len(results), hi - lo), np.uint32)
    steps = np.zeros(len(results), np.int32)
    for i, res in enumerate(results):
        words, steps[i] = pr.pick_words(res, lo, hi)
        pick[i] = words
        cells[i] = [pr.cell_of(r) for r in res[lo:hi]]
    return pick, cells, steps


def engine_of(c, n_nodes=None, table=True):
    """An engine holding the case's snapshot (its first n_nodes nodes), quota groups and bound-pod table."""
    eng = engine.Engine(c.cfg)
    n = len(c.rows) if n_nodes is None else n_nodes
    eng.load_snapshot(c.rows[:n])
    for j in c.removed:
        if j < n:
            eng.remove(int(j))
    if c.quotas is not None:
        eng.set_quotas(c.quotas)
    if table:
        e = int(c.first[n])
        eng.set_bound_pods(c.first[:n + 1], c.b_rows[:e], c.b_prio[:e], c.b_start[:e], c.max_per_node)
    return eng
