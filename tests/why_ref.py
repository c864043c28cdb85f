"""Reason words of (pod, node) pairs from engine rows alone: an independent numpy restatement of the KG_WHY_* table
of include/koord_gpu.h, in the structure of rows_ref.rows_eval (per-resource compares, pod-full, the LoadAware
pass, the valid flag).

TEST INFRASTRUCTURE: the reference of kg_row_why / kg_diagnose (tests/test_why_*.py pin it against the oracle at
object level); the product path never uses it.
"""
import numpy as np

from koordinator_amd import _native as nat


def first_group(w):
    """KG_DIAG_FIRST_FAIL: the bits of the first failing group — ABSENT, ELIG, NodeResourcesFit, LOADAWARE, NUMA."""
    w = np.asarray(w, dtype=np.uint32)
    fit = w & np.uint32(nat.WHY_FIT_MASK)
    out = w & np.uint32(nat.WHY_NUMA)
    out = np.where(w & np.uint32(nat.WHY_LOADAWARE), np.uint32(nat.WHY_LOADAWARE), out)
    out = np.where(fit != 0, fit, out)
    out = np.where(w & np.uint32(nat.WHY_ELIG), np.uint32(nat.WHY_ELIG), out)
    out = np.where(w & np.uint32(nat.WHY_ABSENT), np.uint32(nat.WHY_ABSENT), out)
    return out.astype(np.uint32)


def why_ref(cfg, nodes, pods, now_ns, first_fail=False, elig=None, numa_bad=None):
    """[P][N] uint32 reason words.  `elig`: bool [K][N] eligibility classes (None: the classes are ignored, as
    kg_row_why does); `numa_bad`: bool [P][N], NodeNUMAResource rejects the pair (from the oracle; required when the
    plugin is enabled)."""
    N, P = len(nodes), len(pods)
    plug = int(cfg["enabled_plugins"])
    fit_on, la_on, numa_on = bool(plug & nat.PLUGIN_FIT), bool(plug & nat.PLUGIN_LOADAWARE), bool(plug & nat.PLUGIN_NUMA)
    valid = (nodes["flags"] & nat.NODE_VALID) != 0
    full = nodes["pod_count"].astype(np.int64) + 1 > nodes["allowed_pods"].astype(np.int64)
    has_metric = (nodes["flags"] & nat.NODE_HAS_METRIC) != 0
    has_upd = (nodes["flags"] & nat.NODE_HAS_UPDATE_TIME) != 0
    exp_ns = int(cfg["la_expiration_seconds"]) * 10**9 if cfg["la_has_expiration"] else 0
    expired = ~has_upd | ((exp_ns > 0) & (now_ns - nodes["metric_update_ns"] >= exp_ns))
    skip_filter = bool(cfg["la_filter_expired_node_metrics"]) and bool(cfg["la_has_expiration"])
    free = nodes["alloc"] - nodes["requested"]
    out = np.zeros((P, N), np.uint32)
    for i, p in enumerate(pods):
        w = np.zeros(N, np.uint32)
        k = int(p["elig_class"])
        if elig is not None and k >= 1:
            w |= np.where(np.asarray(elig[k - 1], bool), 0, nat.WHY_ELIG).astype(np.uint32)
        if fit_on:
            w |= np.where(full, nat.WHY_FIT_PODS, 0).astype(np.uint32)
            if p["flags"] & nat.POD_HAS_REQUEST:
                for r in range(nat.NUM_RES):
                    if r < 3 or (int(p["request_present"]) >> r) & 1:
                        w |= np.where(p["request"][r] > free[:, r], nat.WHY_FIT_RES(r), 0).astype(np.uint32)
        if la_on and not (p["flags"] & nat.POD_DAEMONSET):
            bit = nat.NODE_LA_PASS_PROD if p["flags"] & nat.POD_PROD else nat.NODE_LA_PASS_NONPROD
            passes = ~has_metric | (skip_filter & expired) | ((nodes["flags"] & bit) != 0)
            w |= np.where(passes, 0, nat.WHY_LOADAWARE).astype(np.uint32)
        if numa_on and not (p["flags"] & nat.POD_NUMA_SKIP):
            w |= np.where(np.asarray(numa_bad[i], bool), nat.WHY_NUMA, 0).astype(np.uint32)
        out[i] = np.where(valid, w, nat.WHY_ABSENT)
    return first_group(out) if first_fail else out


def counts_ref(why, pod_first=True):
    """kg_diagnose's counts [P][WHY_SLOTS] of a [P][N] word matrix."""
    why = np.asarray(why, dtype=np.uint32)
    out = np.zeros((len(why), nat.WHY_SLOTS), np.uint32)
    for b in range(28):
        out[:, b] = ((why >> np.uint32(b)) & np.uint32(1)).sum(axis=1)
    out[:, nat.WHY_SLOT_REJECTED] = ((why != 0) & (why != nat.WHY_ABSENT)).sum(axis=1)
    out[:, nat.WHY_SLOT_FEASIBLE] = (why == 0).sum(axis=1)
    return out


def quota_leq(p, used, limit):
    for q in range(nat.NUM_RES):
        if (int(limit["present"]) >> q) & 1 and (int(p["numa_request_present"]) >> q) & 1:
            u = int(used["v"][q]) if (int(used["present"]) >> q) & 1 else 0
            if int(p["numa_request"][q]) + u > int(limit["v"][q]):
                return False
    return True


def pod_why_ref(cfg, pods, quotas=None, rsv_slots=False):
    """The pod-level words [P]: the ElasticQuota PreFilter (kg_quota_pass: used + request ≤ used_limit on the
    resources both name, the min gate of a non-preemptible pod, every ancestor under eq_check_parent_quota) and a
    required reservation without loaded slots."""
    plug = int(cfg["enabled_plugins"])
    out = np.zeros(len(pods), np.uint32)
    for i, p in enumerate(pods):
        g = int(p["quota"])
        if plug & nat.PLUGIN_ELASTICQUOTA and quotas is not None and g >= 0:
            q = quotas[g]
            ok = quota_leq(p, q["used"], q["used_limit"])
            if ok and p["flags"] & nat.POD_NON_PREEMPTIBLE:
                ok = quota_leq(p, q["non_preemptible_used"], q["min"])
            if ok and int(cfg["eq_check_parent_quota"]):
                a = int(q["parent"])
                while ok and a >= 0:
                    ok = quota_leq(p, quotas[a]["used"], quotas[a]["used_limit"])
                    a = int(quotas[a]["parent"])
            if not ok:
                out[i] |= nat.WHY_POD_QUOTA
        if plug & nat.PLUGIN_RESERVATION and int(p["rsv_affinity_class"]) >= 0 and not rsv_slots:
            out[i] |= nat.WHY_POD_RSV_REQUIRED
    return out
