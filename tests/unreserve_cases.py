"""Unreserve (kg_row_unreserve, kg_unreserve): the release rules restated in Python, a host model of the engine
state, and the clusters / rows the CPU and GPU tests share.

The restatement (restate_*) is written from the header's contract with Python integers, not from the C code:

    node part     requested[r], nonzero_requested, pod_count - 1, la_used / la_used_x (the prod terms for a prod pod):
                  plain subtraction, no clamp
    zones         for a zone z < n_zones that has an allocation entry and each r with release[z][r] > 0:
                  zone_allocated[z][r] = max(0, zone_allocated[z][r] - release), key bit 2z + r set; bits never cleared
    reservation   m = numa_request_present & allocatable.present: allocated.v[q] = max(0, allocated.v[q] - request[q])
                  for q in m, present |= m, n_assigned - 1
    quota         the group and every ancestor: used.v[q] -= request[q] for the request's keys (and
                  non_preemptible_used for a non-preemptible pod), the keys joining `present`

Model is a numpy copy of the engine state in the style of churn_cases.Model: rows changed by engine.row_commit per
placement and engine.row_unreserve per release, reservation slots and quota groups changed by the restatement of
their Reserve and of their release (restate_rsv / restate_quota with sign +1 / -1).

TEST INFRASTRUCTURE of tests/test_unreserve_cpu.py, tests/test_unreserve_gpu.py and
tests/test_unreserve_bounds_gpu.py; everything is built once and handed out read-only.
"""
import functools

import numpy as np

import churn_cases as ch
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import shipped_profile
from numa_cases import numa_config
from rsv_cases import rsv_cluster

N = ch.N
NOW = synth.NOW_NS
CPU, MEM = nat.RES_CPU, nat.RES_MEMORY
LA_EXTRA_W = {"cpu": 1, "memory": 1, "ephemeral-storage": 1, "example.com/gpu": 2, "kubernetes.io/batch-cpu": 1}
LA_EXTRA_SF = {"ephemeral-storage": 60, "example.com/gpu": 100}
RSV_EQ = ("NodeResourcesFit", "LoadAwareScheduling", "Reservation", "ElasticQuota")


# ---- flag predicates (kg_finalize_flags) -----------------------------------------------------------------------------
def pods_full(row):
    return int(row["pod_count"]) + 1 > int(row["allowed_pods"])


def over_cpu(row):
    return int(row["alloc"][CPU]) - int(row["requested"][CPU]) < 0


def slow(cfg, row):
    return bool(ch.rows_slow(cfg, np.array([row]))[0][0])


# ---- the restatement -------------------------------------------------------------------------------------------------
def restate_row_unreserve(cfg, row, pod, zone_release=None):
    """The released copy of one NODE_ROW record."""
    out = row.copy()
    prod = bool(int(pod["flags"]) & nat.POD_PROD)
    for r in range(nat.NUM_RES):
        out["requested"][r] = int(row["requested"][r]) - int(pod["request"][r])
    for r in range(2):
        out["nonzero_requested"][r] = int(row["nonzero_requested"][r]) - int(pod["nonzero_request"][r])
        out["la_used"][0][r] = int(row["la_used"][0][r]) - int(pod["la_estimate"][r])
        if prod:
            out["la_used"][1][r] = int(row["la_used"][1][r]) - int(pod["la_estimate"][r])
    for x in range(nat.NUM_RES - 2):
        out["la_used_x"][0][x] = int(row["la_used_x"][0][x]) - int(pod["la_estimate_x"][x])
        if prod:
            out["la_used_x"][1][x] = int(row["la_used_x"][1][x]) - int(pod["la_estimate_x"][x])
    out["pod_count"] = int(row["pod_count"]) - 1
    if zone_release is not None and int(cfg["enabled_plugins"]) & nat.PLUGIN_NUMA:
        keys = int(row["zone_alloc_keys"])
        for z in range(int(row["n_zones"])):
            if not (keys >> (2 * z)) & 3:
                continue
            for r in range(2):
                d = int(zone_release[z][r])
                if d > 0:
                    out["zone_allocated"][z][r] = max(0, int(row["zone_allocated"][z][r]) - d)
                    keys |= 1 << (2 * z + r)
        out["zone_alloc_keys"] = keys
    return out


def _get(rl, q):
    return int(rl["v"][q]) if (int(rl["present"]) >> q) & 1 else 0


def restate_rsv(rsv, pod, sign):
    """One RESERVATION record after the Reserve (sign +1) or the release (sign -1) of `pod`, in place."""
    m = int(pod["numa_request_present"]) & int(rsv["allocatable"]["present"])
    for q in range(nat.NUM_RES):
        if (m >> q) & 1:
            v = _get(rsv["allocated"], q) + sign * int(pod["numa_request"][q])
            rsv["allocated"]["v"][q] = v if sign > 0 else max(0, v)
    rsv["allocated"]["present"] = int(rsv["allocated"]["present"]) | m
    rsv["n_assigned"] = int(rsv["n_assigned"]) + sign


def restate_quota(quotas, pod, sign):
    """The QUOTA array after the Reserve (+1) or the release (-1) of `pod`: its group and every ancestor, in place."""
    g = int(pod["quota"])
    lists = ["used"] + (["non_preemptible_used"] if int(pod["flags"]) & nat.POD_NON_PREEMPTIBLE else [])
    keys = int(pod["numa_request_present"])
    while g >= 0:
        for name in lists:
            rl = quotas[name][g]
            for q in range(nat.NUM_RES):
                if (keys >> q) & 1:
                    rl["v"][q] = _get(rl, q) + sign * int(pod["numa_request"][q])
            rl["present"] = int(rl["present"]) | keys
        g = int(quotas["parent"][g])


# ---- the model -------------------------------------------------------------------------------------------------------
class Model:
    """rows (and reservation slots / quota groups) on the host; reserve() returns what the release must hand back."""

    def __init__(self, cfg, rows, rsv=None, quotas=None):
        self.cfg, self.rows = cfg, rows.copy()
        self.plug = int(cfg["enabled_plugins"])
        self.rsv = None if rsv is None else rsv.copy()
        self.quotas = None if quotas is None else quotas.copy()
        self.by_node = {}
        if rsv is not None:
            for k, r in enumerate(rsv):
                self.by_node.setdefault(int(r["node"]), []).append(k)

    def reserve(self, pod, node):
        """The Reserve of one pod row on `node`; returns (zone record, reservation slot) for its later release."""
        j = int(node)
        zones = engine.row_numa_alloc(self.cfg, self.rows[j:j + 1], pod) if self.plug & nat.PLUGIN_NUMA else None
        slot = -1
        if self.rsv is not None and j in self.by_node:
            ks = self.by_node[j]
            nom = engine.row_eval_rsv(self.cfg, self.rows[j:j + 1], self.rsv[ks], pod, NOW)[6]
            if nom >= 0:
                slot = ks[nom]
                restate_rsv(self.rsv[slot], pod[0], +1)
        if self.quotas is not None and self.plug & nat.PLUGIN_ELASTICQUOTA and int(pod["quota"][0]) >= 0:
            restate_quota(self.quotas, pod[0], +1)
        engine.row_commit(self.cfg, self.rows[j:j + 1], pod)
        return zones, slot

    def release(self, pod, node, zones=None, slot=-1):
        j = int(node)
        engine.row_unreserve(self.cfg, self.rows[j:j + 1], pod, zones)
        if slot >= 0:
            restate_rsv(self.rsv[slot], pod[0], -1)
        if self.quotas is not None and self.plug & nat.PLUGIN_ELASTICQUOTA and int(pod["quota"][0]) >= 0:
            restate_quota(self.quotas, pod[0], -1)


def release_choice(nodes):
    """The entries a test rolls back: every third placed pod, plus all pods of the busiest node (repeated entries
    on one node), in call order."""
    placed = np.flatnonzero(nodes >= 0)
    busiest = np.bincount(nodes[placed]).argmax()
    pick = set(placed[::3].tolist()) | set(placed[nodes[placed] == busiest].tolist())
    return np.array(sorted(pick), dtype=np.int64), int(busiest)


# ---- clusters --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fit_la_cluster(extra=False):
    """cfg, node rows, first and second batch (128 pods each) of a Fit + LoadAware engine; extra: LoadAware weights
    beyond cpu / memory."""
    if extra:
        cfg = shipped_profile(place_chunk=16, resource_weights=LA_EXTRA_W, estimated_scaling_factors=LA_EXTRA_SF)
        cl = synth.make_la_extra_cluster(N, 256, seed=71)
    else:
        cfg = shipped_profile(place_chunk=16)
        cl = synth.make_cluster(N, 256, seed=70)
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(256))
    for a in (rows, pods):
        a.setflags(write=False)
    return cfg, rows, pods[:128], pods[128:]


@functools.lru_cache(maxsize=None)
def numa_cluster():
    """NodeNUMAResource without bind policies: no cpuset pod, no node CPU bind policy."""
    cfg = numa_config(place_chunk=16)
    cl = synth.make_numa_cluster(N, 160, seed=72)
    cl.numa_arr["node_cpu_bind_policy"] = nat.NODE_CPU_BIND_NONE
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(160))
    pods = pods[(pods["flags"] & nat.POD_NUMA_CPU_BIND) == 0]
    assert len(pods) >= 128 and not (rows["node_cpu_bind"] != 0).any()
    for a in (rows, pods):
        a.setflags(write=False)
    return cfg, rows, pods[:64], pods[64:128]


@functools.lru_cache(maxsize=None)
def rsv_quota_cluster():
    """Reservation + ElasticQuota: a quota tree checked up the chain, reservations on 60 % of the nodes."""
    cfg = shipped_profile(plugins=RSV_EQ, place_chunk=16, eq_check_parent_quota=1)
    cl = rsv_cluster(N, 256, seed=73, rsv_node_frac=0.6, n_quotas=12, quota_ratio=0.7, quota_tree=True,
                     owned_frac=0.9)
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(256))
    assert (cl.quota_arr["parent"] >= 0).any(), "the tree has inner groups"
    for a in (rows, pods):
        a.setflags(write=False)
    return cfg, rows, pods[:128], pods[128:], cl.rsv_arr.copy(), cl.quota_arr.copy()


# ---- the transition rows: each holds its flag only while the pod is on it --------------------------------------------
@functools.lru_cache(maxsize=None)
def transition_rows():
    """{name: (row before the Reserve, pod row)} on the shipped profile: after row_commit the row is PODS_FULL /
    over-cpu / outside the fp64 bounds (a NonZeroRequested cpu base at KG_VAL_LIMIT), before it is not."""
    cfg, rows, pods, _ = fit_la_cluster()
    pod = pods[np.flatnonzero((pods["request"][:, CPU] > 0) & (pods["nonzero_request"][:, 0] > 0))[:1]].copy()
    ok = [j for j in np.flatnonzero(((rows["flags"] & nat.NODE_VALID) != 0) & (rows["pod_count"] < 100)).tolist()[:200]
          if engine.row_eval(cfg, rows[j:j + 1], pod, NOW)[0]]   # nodes that take the pod as they are
    full = rows[ok[0]].copy()
    full["allowed_pods"] = 110
    full["pod_count"] = 109                      # 109 + 1 ≤ 110, 110 + 1 > 110
    over = rows[ok[1]].copy()
    over["pod_count"] = 3
    over["requested"][CPU] = over["alloc"][CPU] - int(pod["request"][0, CPU]) + 1   # free cpu: the request − 1
    val = rows[ok[2]].copy()
    val["pod_count"] = 3
    val["nonzero_requested"][0] = ch.VAL_LIMIT - int(pod["nonzero_request"][0, 0])  # the base reaches 2^50 with the pod
    pod.setflags(write=False)
    return cfg, {"pods_full": (full, pod), "over_cpu": (over, pod), "val_limit": (val, pod)}


TRANSITION_FLAG = {"pods_full": lambda cfg, r: pods_full(r), "over_cpu": lambda cfg, r: over_cpu(r),
                   "val_limit": lambda cfg, r: slow(cfg, r)}


# ---- engines ---------------------------------------------------------------------------------------------------------
def make_engine(cfg, rows, rsv=None, quotas=None):
    eng = engine.Engine(cfg)
    eng.load_snapshot(rows)
    if rsv is not None:
        eng.set_reservations(rsv)
    if quotas is not None:
        eng.set_quotas(quotas)
    return eng


def same_eval(a, b, what):
    """Two Engine.eval results bit for bit (mask, score planes, the optional planes, top1)."""
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def roll_back(eng, model, first, nodes, pick, recs):
    """kg_unreserve of the entries `pick` of a placed batch on the engine and the model; returns the released flags."""
    zr = None
    if model.plug & nat.PLUGIN_NUMA:
        zr = np.stack([recs[i][0] for i in pick])
    sl = None
    if model.rsv is not None:
        sl = np.array([recs[i][1] for i in pick], dtype=np.int32)
    rel = eng.unreserve(first[pick], nodes[pick], zone_release=zr, rsv_slot=sl)
    for i in pick:
        model.release(first[i:i + 1], nodes[i], *(recs[i] if recs else (None, -1)))
    return rel


def place_on_both(eng, model, first):
    """Engine.place of `first`, replayed into the model; recs[i] = (zone record, slot) of pod i's Reserve."""
    eng.set_pods(first)
    nodes, _ = eng.place(NOW)
    recs = {}
    for i, j in enumerate(nodes.tolist()):
        if j >= 0:
            recs[i] = model.reserve(first[i:i + 1], j)
    return nodes, recs


def fit_la_rollback(extra=False):
    """The Fit + LoadAware case end to end on whatever engine library is loaded (the GPU test and the bounds-build
    child run this): place, roll back, and compare rows, a second batch's eval and its placement with a fresh twin
    loaded from the model.  Returns a summary the caller asserts on."""
    cfg, rows, first, second = fit_la_cluster(extra)
    model = Model(cfg, rows)
    with make_engine(cfg, rows) as eng:
        nodes, recs = place_on_both(eng, model, first)
        pick, busiest = release_choice(nodes)
        g0 = eng.generation()
        rel = roll_back(eng, model, first, nodes, pick, recs)
        g1 = eng.generation()
        got_rows = eng.download()
        eng.set_pods(second)
        got_eval = eng.eval(NOW)
        got_place = eng.place(NOW)
    with make_engine(cfg, model.rows) as twin:
        twin.set_pods(second)
        ref_eval = twin.eval(NOW)
        ref_place = twin.place(NOW)
    return dict(nodes=nodes, pick=pick, busiest=busiest, released=rel, generations=(g0, g1), rows=got_rows,
                model_rows=model.rows, eval=got_eval, ref_eval=ref_eval, place=got_place, ref_place=ref_place)


def rsv_quota_rollback():
    """The Reservation + ElasticQuota case end to end (as fit_la_rollback)."""
    cfg, rows, first, second, rsv, quotas = rsv_quota_cluster()
    model = Model(cfg, rows, rsv, quotas)
    with make_engine(cfg, rows, rsv, quotas) as eng:
        nodes, recs = place_on_both(eng, model, first)
        placed_rsv, placed_q = eng.download_reservations(), eng.download_quotas()
        pick, busiest = release_choice(nodes)
        mid = Model(cfg, model.rows, model.rsv, model.quotas)   # the model after the placements
        rel = roll_back(eng, model, first, nodes, pick, recs)
        got = dict(rows=eng.download(), rsv=eng.download_reservations(), quotas=eng.download_quotas())
        eng.set_pods(second)
        got_place = eng.place(NOW)
    with make_engine(cfg, model.rows, model.rsv, model.quotas) as twin:
        twin.set_pods(second)
        ref_place = twin.place(NOW)
    return dict(nodes=nodes, pick=pick, busiest=busiest, released=rel, recs=recs, got=got, model=model, mid=mid,
                placed_rsv=placed_rsv, placed_quotas=placed_q, place=got_place, ref_place=ref_place)
