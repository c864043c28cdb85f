"""Gang-aware placement (kg_place_gangs): the rules of include/koord_gpu.h restated in Python over two interchangeable
drivers, and the clusters / batches the CPU and GPU tests share.

The model (run_model) walks the queue once.  For pod p with gang g and group G:

    1. g strict and rejected[G]: the pod is skipped (node = score = -1), the driver is not called.
    2. otherwise the driver runs one scheduling cycle on its current state and reserves the winner.
    3. no node and g strict: rejected[G] is set, every earlier placed pod of a gang of G is released through the
       driver (queue order) and gets node = score = -1 -- before pod p + 1's cycle.
    4. no node and g not strict: nothing else.
    5. after the last pod a gang is satisfied iff its placed pods number at least gang_min[g]; the verdict of a
       group is REJECTED / ALLOWED (every gang satisfied) / WAITING; release_waiting releases the WAITING groups.

Drivers (cycle(p) -> (node, score), release(p, node)):

    HostDriver   host rows: engine.row_eval over every row, the lowest index among the best totals, the ElasticQuota
                 gate restated from the header (used + request <= used_limit on the pod's keys, non-preemptible usage
                 against min, the ancestors below it with EnableCheckParentQuota), engine.row_commit /
                 engine.row_unreserve and unreserve_cases.restate_quota.
    TwinDriver   a second engine through merged entry points only, one pod at a time: cycle_one(commit=True), or
                 set_pods + eval(top1) + commit under ElasticQuota, and unreserve for the releases.

TEST INFRASTRUCTURE of tests/test_gangs_cpu.py, tests/test_gangs_gpu.py and tests/test_gangs_bounds_gpu.py.
"""
import functools

import numpy as np

import unreserve_cases as uc
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import shipped_profile
from rsv_cases import rsv_cluster

N = uc.N
NOW = uc.NOW
CPU, MEM, GPU = nat.RES_CPU, nat.RES_MEMORY, nat.RES_EXTENDED
STRICT = nat.GANG_STRICT
ALLOWED, WAITING, REJECTED = nat.GANG_ALLOWED, nat.GANG_WAITING, nat.GANG_REJECTED
FIT_LA_EQ = ("NodeResourcesFit", "LoadAwareScheduling", "ElasticQuota")


# ---- the model -------------------------------------------------------------------------------------------------------
def run_model(driver, n_pods, pod_gang, gang_min, gang_flags, gang_group=None, release_waiting=False):
    """Rules 1-5 over `driver`; returns (nodes int32 [P], scores int64 [P], verdicts uint8 [n_gangs], rolled back
    pod indices)."""
    ng = len(gang_min)
    group = list(range(ng)) if gang_group is None else [int(x) for x in gang_group]
    rejected = [False] * ng
    nodes = np.full(n_pods, -1, np.int32)
    scores = np.full(n_pods, -1, np.int64)
    rolled = []

    def roll_back(G, end):
        for q in range(end):
            if pod_gang[q] >= 0 and group[pod_gang[q]] == G and nodes[q] >= 0:
                driver.release(q, int(nodes[q]))
                nodes[q] = scores[q] = -1
                rolled.append(q)

    for p in range(n_pods):
        g = int(pod_gang[p])
        strict = g >= 0 and bool(gang_flags[g] & STRICT)
        if strict and rejected[group[g]]:
            continue
        nodes[p], scores[p] = driver.cycle(p)
        if nodes[p] < 0 and strict:
            rejected[group[g]] = True
            roll_back(group[g], p)
    have = [0] * ng
    for p in range(n_pods):
        if pod_gang[p] >= 0 and nodes[p] >= 0:
            have[pod_gang[p]] += 1
    waiting = [False] * ng
    for g in range(ng):
        if have[g] < int(gang_min[g]):
            waiting[group[g]] = True
    verdicts = np.array([REJECTED if rejected[group[g]] else WAITING if waiting[group[g]] else ALLOWED
                         for g in range(ng)], np.uint8)
    if release_waiting:
        for G in range(ng):
            if waiting[G] and not rejected[G]:
                roll_back(G, n_pods)
    return nodes, scores, verdicts, rolled


def _get(rl, q):
    return int(rl["v"][q]) if (int(rl["present"]) >> q) & 1 else 0


def _leq(pod, used, limit):
    for q in range(nat.NUM_RES):
        if (int(limit["present"]) >> q) & 1 and (int(pod["numa_request_present"]) >> q) & 1 and \
                int(pod["numa_request"][q]) + _get(used, q) > int(limit["v"][q]):
            return False
    return True


def quota_pass(quotas, pod, check_parent):
    """ElasticQuota PreFilter of one pod row on the QUOTA array."""
    g = int(pod["quota"])
    if g < 0:
        return True
    q = quotas[g]
    if not _leq(pod, q["used"], q["used_limit"]):
        return False
    if int(pod["flags"]) & nat.POD_NON_PREEMPTIBLE and not _leq(pod, q["non_preemptible_used"], q["min"]):
        return False
    a = int(q["parent"])
    while check_parent and a >= 0:
        if not _leq(pod, quotas[a]["used"], quotas[a]["used_limit"]):
            return False
        a = int(quotas[a]["parent"])
    return True


class HostDriver:
    def __init__(self, cfg, rows, pods, quotas=None, elig=None):
        self.cfg, self.rows, self.pods = cfg, rows.copy(), pods
        self.plug = int(cfg["enabled_plugins"])
        self.quotas = None if quotas is None else quotas.copy()
        self.elig = elig   # bool [K][N] or None

    def _quota_on(self, pod):
        return self.quotas is not None and self.plug & nat.PLUGIN_ELASTICQUOTA and int(pod["quota"]) >= 0

    def cycle(self, p):
        pod = self.pods[p:p + 1]
        if self._quota_on(pod[0]) and not quota_pass(self.quotas, pod[0], bool(int(self.cfg["eq_check_parent_quota"]))):
            return -1, -1
        wf, wl = int(self.cfg["weight_fit"]), int(self.cfg["weight_loadaware"])
        best, node = -1, -1
        for j in range(len(self.rows)):
            cls = int(pod["elig_class"][0])
            if cls > 0 and not self.elig[cls - 1][j]:
                continue
            f, fit, la, _ = engine.row_eval(self.cfg, self.rows[j:j + 1], pod, NOW)
            if f and wf * fit + wl * la > best:
                best, node = wf * fit + wl * la, j
        if node < 0:
            return -1, -1
        engine.row_commit(self.cfg, self.rows[node:node + 1], pod)
        if self._quota_on(pod[0]):
            uc.restate_quota(self.quotas, pod[0], +1)
        return node, best

    def release(self, p, node):
        pod = self.pods[p:p + 1]
        engine.row_unreserve(self.cfg, self.rows[node:node + 1], pod)
        if self._quota_on(pod[0]):
            uc.restate_quota(self.quotas, pod[0], -1)


class TwinDriver:
    def __init__(self, eng, pods):
        self.eng, self.pods = eng, pods
        self.quota = bool(int(eng.cfg["enabled_plugins"]) & nat.PLUGIN_ELASTICQUOTA)

    def cycle(self, p):
        pod = self.pods[p:p + 1]
        if not self.quota:
            r = self.eng.cycle_one(pod, NOW, commit=True)
            return int(r["node"]), int(r["score"])
        self.eng.set_pods(pod)
        node, total = engine.decode_top1(self.eng.eval(NOW, mask=False, scores=False, top1=True)["top1"])
        if node[0] < 0:
            return -1, -1
        assert self.eng.commit(0, int(node[0]))
        return int(node[0]), int(total[0])

    def release(self, p, node):
        assert self.eng.unreserve(self.pods[p:p + 1], [node]).all()


# ---- engines ---------------------------------------------------------------------------------------------------------
def make_engine(cfg, rows, quotas=None, elig=None, forms=0):
    eng = uc.make_engine(cfg, rows, quotas=quotas)
    if elig is not None:
        eng.set_eligibility(elig)
    if forms:
        eng.set_forms(forms)
    return eng


def twin_reference(case, gangs, release_waiting=False):
    """The model over a twin engine: (nodes, scores, verdicts, rolled, rows, quotas) with the twin's final state."""
    with make_engine(case["cfg"], case["rows"], case.get("quotas"), case.get("elig")) as twin:
        nodes, scores, verdicts, rolled = run_model(TwinDriver(twin, case["pods"]), len(case["pods"]), gangs["pod_gang"],
                                                    gangs["gang_min"], gangs["gang_flags"], gangs.get("gang_group"),
                                                    release_waiting)
        quotas = twin.download_quotas() if case.get("quotas") is not None else None
        return nodes, scores, verdicts, rolled, twin.download(), quotas


def engine_run(case, gangs, release_waiting=False, place_chunk=None, forms=0, second=None):
    """place_gangs on the engine under test: (nodes, scores, verdicts, rows, quotas, generations, placed counter,
    the second batch's eval or None)."""
    cfg = case["cfg"]
    if place_chunk is not None:
        cfg = cfg.copy()
        cfg["place_chunk"] = place_chunk
    with make_engine(cfg, case["rows"], case.get("quotas"), case.get("elig"), forms) as eng:
        eng.set_pods(case["pods"])
        g0 = eng.generation()
        c0 = eng.counters()["placed"]
        nodes, scores, verdicts = eng.place_gangs(NOW, gangs["pod_gang"], gangs["gang_min"], gangs["gang_flags"],
                                                  gangs.get("gang_group"), release_waiting)
        g1 = eng.generation()
        placed = eng.counters()["placed"] - c0
        rows = eng.download()
        quotas = eng.download_quotas() if case.get("quotas") is not None else None
        ev = None
        if second is not None:
            eng.set_pods(second)
            ev = eng.eval(NOW)
    return dict(nodes=nodes, scores=scores, verdicts=verdicts, rows=rows, quotas=quotas, generations=(g0, g1),
                placed=placed, eval=ev)


def fresh_eval(case, rows, quotas, second):
    """The second batch's eval on a fresh engine loaded from the model's final state."""
    with make_engine(case["cfg"], rows, quotas, case.get("elig")) as eng:
        eng.set_pods(second)
        return eng.eval(NOW)


def compare(case, gangs, release_waiting=False, **kw):
    """place_gangs against the twin model in the four ways of the GPU tests; returns (engine result, model result)."""
    got = engine_run(case, gangs, release_waiting, second=case["second"], **kw)
    ref = twin_reference(case, gangs, release_waiting)
    np.testing.assert_array_equal(got["nodes"], ref[0], err_msg="out_node")
    np.testing.assert_array_equal(got["scores"], ref[1], err_msg="out_score")
    np.testing.assert_array_equal(got["verdicts"], ref[2], err_msg="verdicts")
    assert got["rows"].tobytes() == ref[4].tobytes(), "download() differs from the twin's rows"
    if ref[5] is not None:
        np.testing.assert_array_equal(got["quotas"], ref[5], err_msg="download_quotas()")
    uc.same_eval(got["eval"], fresh_eval(case, ref[4], ref[5], case["second"]), "second batch")
    assert got["placed"] == int((got["nodes"] >= 0).sum())
    return got, ref


# ---- batches ---------------------------------------------------------------------------------------------------------
def unfit(pods, which):
    """A copy of the pod rows where the pods `which` fit nowhere (a cpu request no node can hold)."""
    out = pods.copy()
    for p in which:
        out["request"][p, CPU] = 1 << 40
        out["fit_score_request"][p, CPU] = 1 << 40
    return out


def gangs_of(n_pods, spans, strict=True, gang_min=None, groups=None):
    """pod_gang for gangs given as lists of pod indices (or (begin, end) ranges), one gang each."""
    pg = np.full(n_pods, -1, np.int32)
    for g, s in enumerate(spans):
        idx = range(*s) if isinstance(s, tuple) else s
        for p in idx:
            pg[p] = g
    ng = len(spans)
    flags = np.full(ng, STRICT if strict else 0, np.uint8) if np.isscalar(strict) else np.asarray(strict, np.uint8)
    mins = np.array([len(range(*s)) if isinstance(s, tuple) else len(s) for s in spans], np.int32) if gang_min is None \
        else np.asarray(gang_min, np.int32)
    d = dict(pod_gang=pg, gang_min=mins, gang_flags=flags)
    if groups is not None:
        d["gang_group"] = np.asarray(groups, np.int32)
    return d


@functools.lru_cache(maxsize=None)
def fit_la_case(most=False):
    """Fit + LoadAware on N = 2100 nodes, a 128-pod first batch and a 64-pod second one; most: the MostAllocated
    profile (members of a gang pile up on one node)."""
    cfg, rows, first, second = uc.fit_la_cluster()
    if most:
        cfg = shipped_profile(place_chunk=16, fit_strategy="MostAllocated")
        cl = synth.make_cluster(N, 256, seed=70)
        rows = engine.build_node_rows(cfg, cl)
        pods = engine.build_pod_rows(cfg, cl, np.arange(256))
        for a in (rows, pods):
            a.setflags(write=False)
        first, second = pods[:128], pods[128:]
    return dict(cfg=cfg, rows=rows, pods=first, second=second[:64])


@functools.lru_cache(maxsize=None)
def scarce_case():
    """example.com/gpu on six nodes only (4 each, one in every tile and at the tile edges): a strict gang of 8 pods
    asking 4 each cannot complete and hands the nodes it took back to the plain gpu pods queued behind it."""
    base = fit_la_case()
    rows = base["rows"].copy()
    rows["alloc"][:, GPU] = 0
    rows["requested"][:, GPU] = 0
    rows["alloc_present"] &= ~np.uint32(1 << GPU)
    for j in (3, 1023, 1024, 1500, 2048, N - 1):
        rows["alloc"][j, GPU] = 4
        rows["alloc_present"][j] |= 1 << GPU
    pods = base["pods"][:64].copy()
    gpu_pods = list(range(8, 16)) + [20, 21, 30, 40, 41, 50]
    for p in gpu_pods:
        pods["request"][p, GPU] = 4
        pods["request_present"][p] |= 1 << GPU
    for a in (rows, pods):
        a.setflags(write=False)
    gangs = gangs_of(len(pods), [(8, 16)])
    return dict(cfg=base["cfg"], rows=rows, pods=pods, second=base["second"]), gangs, gpu_pods


@functools.lru_cache(maxsize=None)
def quota_case():
    """Fit + LoadAware + ElasticQuota with a quota tree checked up the chain, no reservation slots."""
    cfg = shipped_profile(plugins=FIT_LA_EQ, place_chunk=16, eq_check_parent_quota=1)
    cl = rsv_cluster(N, 192, seed=91, rsv_node_frac=0.0, n_quotas=12, quota_ratio=0.7, quota_tree=True, owned_frac=0.0)
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(192))
    quotas = cl.quota_arr.copy()
    assert (quotas["parent"] >= 0).any(), "the tree has inner groups"
    for a in (rows, pods, quotas):
        a.setflags(write=False)
    return dict(cfg=cfg, rows=rows, pods=pods[:128], second=pods[128:], quotas=quotas)


def quota_gang(case):
    """A strict gang of the first 12 pods of the busiest leaf group whose k-th member fails the quota gate: every
    limit on the leaf's chain is lifted except the leaf's batch-cpu used_limit, which is set to what it uses now plus
    the requests of the first k - 1 members.  Returns (case with those quotas, gangs, members, k)."""
    pods = case["pods"]
    q = case["quotas"].copy()
    leaves = np.setdiff1d(np.arange(len(q)), q["parent"][q["parent"] >= 0])
    leaf = int(leaves[np.argmax([(pods["quota"] == g).sum() for g in leaves])])
    members = np.flatnonzero(pods["quota"] == leaf)[:12].tolist()
    k = 7
    assert len(members) == 12 and int(q["parent"][leaf]) >= 0
    bcpu = nat.RES_BATCH_CPU
    g = leaf
    while g >= 0:
        q["used_limit"]["v"][g] = 1 << 45
        q["min"]["v"][g] = 1 << 45
        g = int(q["parent"][g])
    demand = sum(int(pods["numa_request"][p, bcpu]) for p in members[:k - 1])
    assert int(pods["numa_request"][members[k - 1], bcpu]) > 0
    q["used_limit"]["v"][leaf, bcpu] = _get(q["used"][leaf], bcpu) + demand   # members 1 .. k - 1 fill it exactly
    q["used_limit"]["present"][leaf] |= 1 << bcpu
    out = dict(case, quotas=q)
    return out, gangs_of(len(pods), [members]), members, k


# ---- the two cases the bounds build repeats -----------------------------------------------------------------------------
def scarce_summary():
    case, gangs, gpu_pods = scarce_case()
    got, ref = compare(case, gangs)
    with make_engine(case["cfg"], case["rows"]) as eng:
        eng.set_pods(case["pods"])
        plain = eng.place(NOW)[0]
    return dict(nodes=got["nodes"], verdicts=got["verdicts"], rolled=np.array(ref[3]), plain=plain,
                gpu_pods=np.array(gpu_pods), rows=got["rows"])


def quota_summary():
    case, gangs, members, k = quota_gang(quota_case())
    got, ref = compare(case, gangs)
    return dict(nodes=got["nodes"], verdicts=got["verdicts"], rolled=np.array(ref[3]), members=np.array(members),
                k=np.array(k), quotas=got["quotas"], rows=got["rows"], quotas0=case["quotas"])
