"""The preemption dry run from engine rows alone: a literal Python restatement of ElasticQuota's SelectVictimsOnNode
(pkg/scheduler/plugins/elasticquota/preempt.go:111-215, canPreempt :283-294, the AddPod / RemovePod PreFilter
extensions plugin.go:263-299) without PodDisruptionBudgets, and of upstream pickOneNodeForPreemption's order with the
project's tie rule (the lowest node index).

TEST INFRASTRUCTURE: the reference of kg_row_preempt / kg_preempt (tests/test_preempt_*.py); the product path never
uses it and it calls none of the preemption entry points.  Filter is why_ref.why_ref(...) == 0 on the modified row
(oracle-pinned by tests/test_why_cpu.py).  NodeInfo.Pods is a list, removePod raises when the pod is not there (the
KG_PRE_ERROR path), `used` is a dict with the quotav1 semantics.  Every node runs the restatement as a generator that
yields the NodeInfo it wants filtered, so one why_ref call answers a round of all nodes at once.
"""
from types import SimpleNamespace

import numpy as np

import why_ref
from koordinator_amd import _native as nat


# ---- quotav1 on {resource id: value} dicts --------------------------------------------------------
def q_add(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def q_subtract_nonneg(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = max(0, out.get(k, 0) - v)
    return out


def q_mask(a, names):
    return {k: a[k] for k in names if k in a}


def q_leq(a, b):
    return all(not (k in a and a[k] > v) for k, v in b.items())


def rl_dict(values, present):
    return {r: int(values[r]) for r in range(nat.NUM_RES) if (int(present) >> r) & 1}


# ---- NodeInfo ------------------------------------------------------------------------------------
class NodeInfo:
    def __init__(self, row, bound):
        self.requested = row["requested"].astype(np.int64).copy()
        self.nonzero = row["nonzero_requested"].astype(np.int64).copy()
        self.pod_count = int(row["pod_count"])
        self.pods = list(bound)

    def remove_pod(self, e):
        if not any(x is e for x in self.pods):
            raise KeyError("no corresponding pod in pods of node")   # NodeInfo.RemovePod's error
        self.pods = [x for x in self.pods if x is not e]
        self.requested -= e.row["request"]
        self.nonzero -= e.row["nonzero_request"]
        self.pod_count -= 1

    def add_pod(self, e):
        self.pods.append(e)
        self.requested += e.row["request"]
        self.nonzero += e.row["nonzero_request"]
        self.pod_count += 1


class Entry:
    """One pod of NodeInfo.Pods (compared by identity): the row, PodPriority, StartTime, the caller position."""

    def __init__(self, row, prio, start, pos):
        self.row, self.prio, self.start, self.pos = row, int(prio), int(start), pos


def bound_entries(rows, priority, start_ns):
    return [Entry(rows[i], priority[i], start_ns[i], i) for i in range(len(rows))]


def select_victims(cfg, row, bound, pod, pp, quotas):
    """SelectVictimsOnNode as a generator: yields the NodeInfo to filter, is sent `fits`, returns the result."""
    res = SimpleNamespace(status=nat.PRE_ABSENT, victims=[], n_potential=0, quota_victims=0, reprieved_before_victim=False)
    if not int(row["flags"]) & nat.NODE_VALID:
        return res
    ni = NodeInfo(row, bound)
    g = int(pod["quota"])
    skip = not (int(cfg["enabled_plugins"]) & nat.PLUGIN_ELASTICQUOTA) or g < 0
    st = SimpleNamespace(used={} if skip else rl_dict(quotas[g]["used"]["v"], quotas[g]["used"]["present"]),
                         used_limit={} if skip else rl_dict(quotas[g]["used_limit"]["v"], quotas[g]["used_limit"]["present"]))
    pod_req = rl_dict(pod["numa_request"], pod["numa_request_present"])

    def can_preempt(v):
        if int(v.row["flags"]) & nat.POD_NON_PREEMPTIBLE:
            return False
        return pp > v.prio and g == int(v.row["quota"])

    def remove_pod(e):
        ni.remove_pod(e)
        if not skip:
            st.used = q_subtract_nonneg(st.used, rl_dict(e.row["numa_request"], e.row["numa_request_present"]))

    def add_pod(e):
        ni.add_pod(e)
        if not skip:
            st.used = q_add(st.used, rl_dict(e.row["numa_request"], e.row["numa_request_present"]))

    potential = []
    for e in list(ni.pods):
        if can_preempt(e):
            potential.append(e)
            remove_pod(e)
    res.n_potential = len(potential)
    if not potential:
        res.status = nat.PRE_NO_VICTIMS
        return res
    if not (yield ni):
        res.status = nat.PRE_UNFIT
        return res
    # util.MoreImportantPod: higher priority, then the earlier start; ties (sort.Slice leaves them open) keep the list order
    potential.sort(key=lambda e: (-e.prio, e.start, e.pos))
    victims = []
    reprieved = False
    try:
        for e in potential:   # no PDBs: every potential victim is non-violating
            add_pod(e)
            fits = yield ni
            was_victim = False
            if not fits:
                remove_pod(e)
                victims.append(e)
                was_victim = True
            new_used = q_mask(q_add(st.used, pod_req), pod_req.keys())
            if not skip and not q_leq(new_used, st.used_limit):
                remove_pod(e)
                victims.append(e)
                res.quota_victims += 1
                was_victim = True
            if was_victim and reprieved:
                res.reprieved_before_victim = True
            if not was_victim:
                reprieved = True
    except KeyError:
        res.status = nat.PRE_ERROR
        res.quota_victims = 0
        res.reprieved_before_victim = False
        return res
    res.status = nat.PRE_CANDIDATE
    res.victims = victims
    return res


def dry_run(cfg, rows, first, b_rows, b_prio, b_start, pod, pp, quotas, now_ns, elig=None):
    """One preemptor against every node: the list of per-node results.  `rows`: the reference's node rows (removed
    nodes with KG_NODE_VALID cleared); `elig`: bool [K][N] or None (the class is then ignored, as kg_row_preempt)."""
    N = len(rows)
    pods1 = np.array([pod], dtype=nat.POD_ROW)
    gens, out, waiting = {}, [None] * N, {}
    for j in range(N):
        lo, hi = int(first[j]), int(first[j + 1])
        gen = select_victims(cfg, rows[j], bound_entries(b_rows[lo:hi], b_prio[lo:hi], b_start[lo:hi]), pod, pp, quotas)
        try:
            waiting[j] = next(gen)
            gens[j] = gen
        except StopIteration as s:
            out[j] = s.value
    while waiting:
        idx = np.fromiter(waiting.keys(), dtype=np.int64)
        mod = rows[idx].copy()
        for k, j in enumerate(idx):
            ni = waiting[int(j)]
            mod["requested"][k] = ni.requested
            mod["nonzero_requested"][k] = ni.nonzero
            mod["pod_count"][k] = ni.pod_count
        why = why_ref.why_ref(cfg, mod, pods1, now_ns, elig=None if elig is None else np.asarray(elig)[:, idx])[0]
        nxt = {}
        for k, j in enumerate(idx):
            j = int(j)
            try:
                nxt[j] = gens[j].send(bool(why[k] == 0))
            except StopIteration as s:
                out[j] = s.value
        waiting = nxt
    return out


def stats_of(res):
    """(n_victims, hi_prio, prio_sum, earliest_ns, mask word 0, mask word 1) of a result; zeros unless a candidate."""
    if res.status != nat.PRE_CANDIDATE or not res.victims:
        return 0, 0, 0, 0, 0, 0
    hi = max(v.prio for v in res.victims)
    early = min(v.start for v in res.victims if v.prio == hi)
    mask = 0
    for v in res.victims:
        mask |= 1 << v.pos
    return (len(res.victims), hi, sum(v.prio + (1 << 31) for v in res.victims), early, mask & ((1 << 64) - 1), mask >> 64)


def cell_of(res):
    """The plane cell of a result: status | n_victims << 8 | n_potential << 16."""
    nv = len(res.victims) if res.status == nat.PRE_CANDIDATE else 0
    return res.status | nv << 8 | res.n_potential << 16


def pick_one(cands):
    """pickOneNodeForPreemption over [(node, n_victims, hi_prio, prio_sum, earliest_ns)] without PDBs, the last tie
    resolved by the lowest node index.  Returns (node, the step 1..6 that decided); (-1, 0) without candidates; a lone
    candidate is decided at step 0 (upstream returns it before any comparison)."""
    if not cands:
        return -1, 0
    if len(cands) == 1:
        return cands[0][0], 0
    zero = [c for c in cands if c[1] == 0]
    if zero:
        return min(c[0] for c in zero), 1
    left = list(cands)
    for step, key in ((2, lambda c: c[2]), (3, lambda c: c[3]), (4, lambda c: c[1]), (5, lambda c: -c[4])):
        best = min(key(c) for c in left)
        left = [c for c in left if key(c) == best]
        if len(left) == 1:
            return left[0][0], step
    return min(c[0] for c in left), 6


def pick_words(results, lo=0, hi=None):
    """kg_preempt's pick words of one preemptor from its per-node results over nodes [lo, hi), and the deciding step."""
    hi = len(results) if hi is None else hi
    cands = []
    for j in range(lo, hi):
        if results[j].status == nat.PRE_CANDIDATE:
            nv, hp, ps, es, _, _ = stats_of(results[j])
            cands.append((j, nv, hp, ps, es))
    node, step = pick_one(cands)
    if node < 0:
        return [-1, 0, 0, 0, 0, 0, 0, 0], step
    nv, hp, ps, es, m0, m1 = stats_of(results[node])
    to_i64 = lambda x: x - (1 << 64) if x >= 1 << 63 else x
    return [node, nv, hp, ps, es, to_i64(m0), to_i64(m1), len(cands)], step
