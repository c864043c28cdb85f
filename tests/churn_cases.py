"""Long-lived engines: seeded scripts of snapshot deltas, batch swaps, shard moves and clock changes on ONE engine.

Every other GPU test builds an engine, loads one snapshot, uploads one batch and calls one entry point.  Here a script
is a list of steps (Step.kind):

    upsert   rows `idx` of the snapshot are rewritten from the edited view `view` (engine.build_node_rows)
    remove   Engine.remove(node)
    pods     Engine.set_pods of the pods `idx` of the view (elig: their elig_class, or None)
    shard    Engine.set_shard(begin, end)
    elig     Engine.set_eligibility(masks);  elig_update: Engine.update_eligibility(cls, nodes, eligible)
    rsv      Engine.set_reservations(rsv) (the view carries the same records from then on)
    check    a checkpoint: Engine.eval(now_ns) compared with every reference that applies (label names the step)
    place    Engine.place(now_ns) — under a shard Engine.place_sharded on one rank — compared with the sequential cycle
             over the shard's nodes

Model walks a script on the host and hands out the references of a checkpoint:

    1. oracle_planes   the oracle on the edited view (valid until the first commit),
    2. rows / rows_planes   the model rows — a numpy copy of the snapshot, changed by the same upserts and by
       engine.row_commit per placement — and, for Fit + LoadAware engines, rows_ref.rows_eval on them (exact int64),
    3. the fresh twin is built by the GPU test from Model.rows and the model's side tables.

N = 2100 nodes everywhere: two full 1024-node tiles and a ragged third.

TEST INFRASTRUCTURE shared by tests/test_churn_cpu.py (which asserts that the scripts reach the transitions they are
written for) and tests/test_churn_gpu.py.  Scripts are built once and handed out read-only.
"""
import functools

import numpy as np

import elig_cases
import rows_ref
import wide_cases as wc
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import shipped_profile
from numa_cases import numa_config
from oracle import oracle

N = 2100
NOW = synth.NOW_NS
SEC = 10**9
GI = 1 << 30
CAP_LIMIT, VAL_LIMIT = 1 << 41, 1 << 50          # KG_CAP_LIMIT, KG_VAL_LIMIT (kg_common.h)
CORNERS = (0, 1023, 1024, N - 1)                 # first / last node of a full tile, first of the next, last of the ragged
RAGGED = 2048                                    # first node of the ragged tile
BATCH_CPU, BATCH_MEM = "kubernetes.io/batch-cpu", "kubernetes.io/batch-memory"
CPU, MEM, EPH = nat.RES_CPU, nat.RES_MEMORY, nat.RES_EPHEMERAL_STORAGE
FIT_LA = nat.PLUGIN_FIT | nat.PLUGIN_LOADAWARE


class Step:
    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)

    def __repr__(self):
        return f"Step({self.kind}, {getattr(self, 'label', '')})"


# ---- predicates restated from the engine (kg_common.h) -------------------------------------------------------------
def val_out(x):
    """kg_val_out: outside [0, KG_VAL_LIMIT)."""
    return (x < 0) | (x >= VAL_LIMIT)


def cap_out(a):
    return (a < 0) | (a >= CAP_LIMIT)


def rows_slow(cfg, rows):
    """(slow, xslow) per node row: outside the fp64 bounds of a Fit / LoadAware cpu-memory plane (KGD_SLOW without the
    extra-resource term), and additionally of a weighted LoadAware extra resource's plane (KGD_XSLOW)."""
    fw, lw = cfg["fit_resource_weight"], cfg["la_resource_weight"]
    slow = np.zeros(len(rows), bool)
    for r in range(nat.NUM_RES):
        if fw[r] <= 0:
            continue
        a = rows["alloc"][:, r]
        present = np.ones(len(rows), bool) if r < 3 else ((rows["alloc_present"] >> r) & 1) == 1
        base = rows["nonzero_requested"][:, r] if r < 2 else rows["requested"][:, r]
        slow |= present & (a != 0) & (cap_out(a) | val_out(base))
    for r in range(2):
        a = rows["la_alloc"][:, r]
        slow |= (a != 0) & (cap_out(a) | val_out(rows["la_used"][:, 0, r]) | val_out(rows["la_used"][:, 1, r]))
    xslow = slow.copy()
    for x in range(nat.NUM_RES - 2):
        if lw[2 + x] <= 0:
            continue
        a = rows["la_alloc_x"][:, x]
        xslow |= (a != 0) & (cap_out(a) | val_out(rows["la_used_x"][:, 0, x]) | val_out(rows["la_used_x"][:, 1, x]))
    return slow, xslow


def rows_expired(cfg, rows, now_ns):
    """The expiry rule of rows_ref.rows_eval: nodes with a metric whose update time is too old at now_ns."""
    has_upd = (rows["flags"] & nat.NODE_HAS_UPDATE_TIME) != 0
    exp_ns = int(cfg["la_expiration_seconds"]) * SEC if cfg["la_has_expiration"] else 0
    return has_upd & (exp_ns > 0) & (now_ns - rows["metric_update_ns"] >= exp_ns)


def pod_fit_w(cfg, pod_rows):
    """Each pod's NodeResourcesFit weight sum (kg_pod_hot_from_row's w): a power of two ⇔ the pod is specialisable."""
    fw = cfg["fit_resource_weight"].astype(np.int64)
    out = np.zeros(len(pod_rows), np.int64)
    for r in range(nat.NUM_RES):
        if fw[r] > 0:
            out += np.where((pod_rows["fit_score_request"][:, r] != 0) | (r < 3), fw[r], 0)
    return out


def is_pow2(w):
    w = np.asarray(w)
    return (w & (w - 1)) == 0


def distinct_rows(pod_rows):
    return len({r.tobytes() for r in pod_rows})


# ---- node edits (in place on a NODE_SPEC array; `base` is the pristine copy) ------------------------------------------
def _set(rl, idx, r, v):
    rl["v"][idx, r] = v
    rl["present"][idx] |= np.uint32(1 << r)


def reload(nodes, base, which, rng):
    """Back to the pristine spec with a fresh random load (requested, usage, pod count)."""
    which = np.asarray(which)
    nodes[which] = base[which]
    k = len(which)
    cpu, mem = base["allocatable"]["v"][which, CPU], base["allocatable"]["v"][which, MEM]
    rc, rm = (cpu * rng.integers(0, 71, k)) // 100, (mem // 100) * rng.integers(0, 71, k)
    nodes["requested"]["v"][which, CPU] = rc
    nodes["requested"]["v"][which, MEM] = rm
    nodes["nonzero_requested"][which, 0] = rc + 100 * rng.integers(0, 3, k)
    nodes["nonzero_requested"][which, 1] = rm
    nodes["node_usage"]["v"][which, CPU] = (cpu * rng.integers(0, 81, k)) // 100
    nodes["node_usage"]["v"][which, MEM] = (mem // 100) * rng.integers(0, 91, k)
    nodes["pod_count"][which] = rng.integers(0, 60, k)


def out_alloc(nodes, which):
    """Allocatable memory at or beyond 2^41: outside the fp64 bounds."""
    nodes["allocatable"]["v"][which, MEM] = (1 << 43) + 12345
    nodes["requested"]["v"][which, MEM] = (1 << 42) + 777


def out_base(nodes, which):
    """A NonZeroRequested cpu base at or beyond 2^50: outside the fp64 bounds (the score is 0: base > cap)."""
    nodes["nonzero_requested"][which, 0] = VAL_LIMIT + 17


def drop_metric(nodes, which):
    for f in ("has_node_metric", "has_update_time", "has_report_interval", "has_node_metric_info"):
        nodes[f][which] = 0


def heat(nodes, base, which, percent):
    """Node cpu usage at `percent` of allocatable (above the 65 % threshold the LoadAware filter rejects)."""
    nodes["node_usage"]["v"][which, CPU] = base["allocatable"]["v"][which, CPU] * percent // 100


def star(nodes, k, now_ns):
    """Node k becomes the emptiest, largest node of the cluster with a fresh metric: the best node of most pods."""
    z = np.zeros((), nodes.dtype)
    z["allowed_pods"] = 110
    z["numa"] = nodes["numa"][k]
    for f in ("has_node_metric", "has_update_time", "has_report_interval", "has_node_metric_info"):
        z[f] = 1
    z["update_time_ns"] = now_ns - 30 * SEC
    z["report_interval_seconds"] = 60
    nodes[k] = z
    _set(nodes["allocatable"], k, CPU, 128_000)
    _set(nodes["allocatable"], k, MEM, 512 * GI)
    _set(nodes["allocatable"], k, nat.RES_BATCH_CPU, 76_800)
    _set(nodes["allocatable"], k, nat.RES_BATCH_MEMORY, 300 * GI)
    for r in (CPU, MEM, EPH, nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY):
        _set(nodes["requested"], k, r, 0)
    _set(nodes["node_usage"], k, CPU, 0)
    _set(nodes["node_usage"], k, MEM, 0)


# ---- scripts -------------------------------------------------------------------------------------------------------
class Script:
    """cfg, the initial view, the steps; while it is built, `nodes` / `numa` are the working copies the edits change."""

    def __init__(self, name, cfg, view0, forms=0):
        self.name, self.cfg, self.view0, self.forms = name, cfg, view0, forms
        self.base = view0.nodes.copy()
        self.nodes = view0.nodes.copy()
        self.numa = view0.numa_arr.copy()
        self.rsv = view0.rsv_arr
        self.view = view0
        self.steps = []
        self.touched = {}           # node → number of upserts

    def _mkview(self):
        v = self.view0
        self.view = synth.SynthView(v.pods, v.containers, self.nodes.copy(), v.now_ns, self.numa.copy(), self.rsv,
                                    v.quota_arr, v.aggregated_arr, v.pod_metrics_arr, v.assigned_arr)
        return self.view

    def upsert(self, which, label=""):
        idx = np.unique(np.asarray(which, dtype=np.int32))
        for j in idx.tolist():
            self.touched[j] = self.touched.get(j, 0) + 1
        self.steps.append(Step("upsert", idx=idx, view=self._mkview(), label=label))

    def remove(self, node):
        self.steps.append(Step("remove", node=int(node), label=f"remove {node}"))

    def pods(self, idx, elig=None, label=""):
        idx = np.asarray(idx, dtype=np.int32)
        self.steps.append(Step("pods", idx=idx, elig=None if elig is None else np.asarray(elig, np.int32), label=label))

    def shard(self, b, e):
        self.steps.append(Step("shard", shard=(int(b), int(e)), label=f"shard {b}:{e}"))

    def elig(self, masks):
        self.steps.append(Step("elig", masks=np.array(masks, dtype=bool), label="set_eligibility"))

    def elig_update(self, cls, nodes, eligible):
        self.steps.append(Step("elig_update", cls=int(cls), nodes=np.asarray(nodes, np.int32), eligible=bool(eligible),
                               label="update_eligibility"))

    def set_rsv(self, rsv, label="set_reservations"):
        self.rsv = rsv
        self.steps.append(Step("rsv", rsv=rsv, view=self._mkview(), label=label))

    def check(self, now_ns, label):
        self.steps.append(Step("check", now_ns=int(now_ns), label=label))

    def place(self, now_ns, label="place"):
        self.steps.append(Step("place", now_ns=int(now_ns), label=label))

    def kinds(self):
        return [s.kind for s in self.steps]


def _keys(m, total, begin):
    """top-1 keys (total + 1) << 32 | (0xFFFFFFFF − node) of the best feasible column, ties to the lowest node."""
    node, best = elig_cases.best_of(m, total, begin)
    keys = np.zeros(len(m), np.uint64)
    ok = best >= 0
    keys[ok] = ((best[ok].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | \
        (np.uint64(0xFFFFFFFF) - node[ok].astype(np.uint64))
    return keys


class Model:
    """The host-side state of a script: the edited view, the model rows, the batch, the side tables."""

    def __init__(self, script):
        self.s, self.cfg = script, script.cfg
        self.view = script.view0
        self.rows = engine.build_node_rows(self.cfg, self.view)
        self.n = len(self.rows)
        self.plug = int(self.cfg["enabled_plugins"])
        self.committed = False
        self.removed = set()
        self.pod_idx = self.pod_rows = self.elig_class = self.masks = self.rsv = None
        self.shard = (0, self.n)

    # -- steps: each returns what the engine side of the step needs ---------------------------------------------------
    def upsert(self, st):
        rows = engine.build_node_rows(self.cfg, st.view, st.idx)
        self.rows[st.idx] = rows
        self.view = st.view
        self.removed -= set(st.idx.tolist())
        return rows

    def remove(self, st):
        self.rows[st.node] = np.zeros((), nat.NODE_ROW)
        self.removed.add(st.node)

    def pods(self, st):
        rows = engine.build_pod_rows(self.cfg, self.view, st.idx)
        self.elig_class = st.elig
        if st.elig is not None:
            rows["elig_class"] = st.elig
        self.pod_idx, self.pod_rows = st.idx, rows
        return rows

    def apply(self, st):
        """A step that only changes tables (shard, elig, elig_update, rsv)."""
        if st.kind == "shard":
            self.shard = st.shard
        elif st.kind == "elig":
            self.masks = st.masks.copy()
        elif st.kind == "elig_update":
            self.masks[st.cls, st.nodes] = st.eligible
        elif st.kind == "rsv":
            self.rsv, self.view = st.rsv, st.view
        else:
            raise ValueError(st.kind)

    # -- references ---------------------------------------------------------------------------------------------------
    @property
    def restricted(self):
        return self.elig_class is not None and bool(np.any(self.elig_class != 0))

    def _restrict(self, m):
        if self.restricted:
            return elig_cases.restrict(m, self.masks, self.elig_class, self.shard[0])
        return m

    def _finish(self, m, f, l, numa=None, rsv=None, top1=None):
        b, e = self.shard
        gone = [j - b for j in self.removed if b <= j < e]
        planes = [np.array(a) for a in (m, f, l)] + [None if a is None else np.array(a) for a in (numa, rsv)]
        for a in planes:
            if a is not None and gone:
                a[:, gone] = 0                       # a removed node: a zero row, never feasible, every score 0
        m, f, l, numa, rsv = planes
        m = self._restrict(m.astype(bool))
        if top1 is None:
            top1 = _keys(m, elig_cases.totals(self.cfg, f, l, numa if self.plug & nat.PLUGIN_NUMA else None), b)
        return dict(mask=m, fit=f, la=l, numa=numa, rsv=rsv, top1=top1)

    def oracle_planes(self, now_ns):
        """Reference 1: the oracle on the edited view, over the shard's columns."""
        assert not self.committed, "the view does not describe committed rows"
        b, e = self.shard
        uniq, inv = np.unique(self.pod_idx, return_inverse=True)   # (a repeated pod is evaluated once)
        if self.plug & nat.PLUGIN_RESERVATION:
            assert (b, e) == (0, self.n) and not self.removed and not self.restricted
            m, f, l, nm, rs, top1 = oracle.eval_matrix5(self.cfg, self.view, uniq, now_ns)
            return self._finish(m[inv], f[inv], l[inv], None, rs[inv], top1[inv])
        if self.plug & nat.PLUGIN_NUMA:
            m, f, l, nm = oracle.eval_matrix3(self.cfg, self.view, uniq, now_ns, b, e)
            return self._finish(m[inv], f[inv], l[inv], nm[inv])
        m, f, l = oracle.eval_matrix_range(self.cfg, self.view, uniq, b, e, now_ns)
        return self._finish(m[inv], f[inv], l[inv])

    @property
    def has_rows_eval(self):
        """rows_ref.rows_eval answers Fit + LoadAware over cpu / memory weights."""
        return self.plug == FIT_LA and not self.cfg["la_resource_weight"][2:].any()

    def rows_planes(self, now_ns):
        """Reference 2: rows_ref.rows_eval on the model rows (exact numpy int64)."""
        assert self.has_rows_eval
        b, e = self.shard
        m, f, l = rows_ref.rows_eval(self.cfg, self.rows[b:e], self.pod_rows, now_ns)
        return self._finish(m, f, l)

    def place(self, st):
        """The sequential cycle over the shard: the oracle on the edited view before the first commit, afterwards the
        replay on the model rows (rows_ref.pair_totals argmax, lowest index on ties).  Commits into the model rows."""
        b, e = self.shard
        assert not self.removed and not self.restricted
        if not self.committed:
            view = self.view if (b, e) == (0, self.n) else self.view.subset_nodes(b, e)
            if getattr(st, "cycle", None) is None:   # (the oracle's cycle is computed once per script)
                nodes, scores = oracle.schedule(self.cfg, view, self.pod_idx, st.now_ns)
                st.cycle = np.where(nodes >= 0, nodes + b, -1).astype(np.int32), scores
            nodes, scores = st.cycle
            for p, j in enumerate(nodes.tolist()):
                if j >= 0:
                    engine.row_commit(self.cfg, self.rows[j:j + 1], self.pod_rows[p:p + 1])
            ref = "oracle.schedule on the edited view"
        else:
            assert self.has_rows_eval
            nodes = np.full(len(self.pod_rows), -1, np.int32)
            scores = np.full(len(self.pod_rows), -1, np.int64)
            for p in range(len(self.pod_rows)):
                ok, tot = rows_ref.pair_totals(self.cfg, self.rows[b:e], self.pod_rows[p], st.now_ns)
                t = np.where(ok, tot, -1)
                if t.max() >= 0:
                    j = b + int(t.argmax())
                    nodes[p], scores[p] = j, int(t.max())
                    engine.row_commit(self.cfg, self.rows[j:j + 1], self.pod_rows[p:p + 1])
            ref = "replay on the model rows"
        self.committed = True
        return nodes, scores, ref


def compare(got, ref, width, full_scores, what):
    """An Engine.eval result against reference planes over `width` columns: mask and its pad bits, the score planes
    (everywhere, or where feasible when the batch has spill or restricted pods: their scores are meaningful where the
    mask bit is set), the NUMA / Reservation planes the reference has, and top-1."""
    m = ref["mask"]
    bits = np.unpackbits(np.ascontiguousarray(got["mask"]).view(np.uint8).reshape(len(m), -1), axis=1, bitorder="little")
    np.testing.assert_array_equal(bits[:, :width].astype(bool), m, err_msg=f"{what}: mask")
    assert not bits[:, width:].any(), f"{what}: mask pad bits set"
    keep = np.ones_like(m) if full_scores else m
    for k, plane in (("fit", got["scores"][:, :width, 0]), ("la", got["scores"][:, :width, 1])):
        np.testing.assert_array_equal(np.where(keep, plane, 0), np.where(keep, ref[k], 0), err_msg=f"{what}: {k}")
    if ref.get("numa") is not None and "numa_scores" in got:
        np.testing.assert_array_equal(np.where(keep, got["numa_scores"][:, :width], 0), np.where(keep, ref["numa"], 0),
                                      err_msg=f"{what}: numa")
    if ref.get("rsv") is not None:
        np.testing.assert_array_equal(got["rsv_scores"][:, :width], ref["rsv"], err_msg=f"{what}: rsv")
    np.testing.assert_array_equal(got["top1"], ref["top1"], err_msg=f"{what}: top1")


def same_planes(a, b, what):
    """Two reference dicts agree (references 1 and 2 before the GPU sees them)."""
    for k in ("mask", "fit", "la", "top1"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


# ---- scenario A: row deltas on a Fit + LoadAware engine ----------------------------------------------------------------
A_P = 65
A_HOT = (5, 1021, 1500, 2077, 2097)          # rewritten at almost every step
A_OUT = {"alloc": (0, 1023, 640, 2060, 2099), "base": (1024, 77, 1999, 2051, 2098)}   # out of the bounds and back
A_OUT2 = {"alloc": (3, 1025, 2070, 2096), "base": (1022, 2047, 2048, 2090)}            # again after the first place
A_GONE = 1700                                # removed, later upserted valid again
A_STAR = 2088                                # becomes some pods' best node after a delta (ragged tile)
A_SLOT_FIT = {"cpu": 2, "memory": 1, BATCH_CPU: 3}   # cpu / memory pods weigh 3: the batch takes k_eval2


def _a_cluster(seed):
    cl = synth.make_cluster(N, A_P, seed=seed)
    # the last pod asks for more cpu than any node has: unschedulable in every place
    c = int(cl.pods["first_container"][A_P - 1])
    for rl in (cl.containers["requests"], cl.containers["limits"]):
        _set(rl, c, CPU, 10**7)
    return cl


@functools.lru_cache(maxsize=None)
def scenario_a(slot=False):
    """12 delta steps on the class path (slot: 6 on k_eval2), each followed by a checkpoint; one place in the middle
    against the oracle, then rows-only references and a second place against the replay."""
    rng = np.random.default_rng(29 if slot else 23)
    cfg = shipped_profile(place_chunk=16, fit_resources=A_SLOT_FIT) if slot else shipped_profile(place_chunk=16)
    s = Script("a_slot" if slot else "a_class", cfg, _a_cluster(31 if slot else 30))
    nd, base = s.nodes, s.base
    metric = np.flatnonzero((base["has_node_metric"] != 0) & (base["update_time_ns"] == NOW - 30 * SEC))
    metric = metric[~np.isin(metric, A_HOT + A_OUT["alloc"] + A_OUT["base"] + A_OUT2["alloc"] + A_OUT2["base"]
                             + (A_GONE, A_STAR))]
    lose, flip, stale = metric[:8], metric[8:16], metric[16:38]
    hot = np.array(A_HOT)

    def some(k):
        return np.concatenate([hot, rng.choice(metric[50:], k - len(hot), replace=False)])

    s.pods(np.arange(A_P), label="65 pods")
    s.check(NOW, "initial")
    # 1: a plain load delta, 40 rows
    w = some(40)
    reload(nd, base, w, rng)
    s.upsert(w, "load 40")
    s.check(NOW, "after load 40")
    # 2: out of the fp64 bounds, both ways in (alloc ≥ 2^41, base ≥ 2^50); the corners and the ragged tile among them
    out_alloc(nd, list(A_OUT["alloc"]))
    out_base(nd, list(A_OUT["base"]))
    s.upsert(A_OUT["alloc"] + A_OUT["base"], "10 nodes out of bounds")
    s.check(NOW, "out of bounds")
    # 3: load delta, and a node leaves
    w = some(20)
    reload(nd, base, w, rng)
    s.upsert(w, "load 20")
    s.remove(A_GONE)
    s.check(NOW, "node removed")
    if slot:
        # 4: back inside; metrics lost, LoadAware-pass flags flip
        w = np.array(A_OUT["alloc"] + A_OUT["base"])
        reload(nd, base, w, rng)
        drop_metric(nd, lose)
        heat(nd, base, flip, 90)
        s.upsert(np.concatenate([w, lose, flip]), "back in bounds, metric lost, flags flip")
        s.check(NOW, "back in bounds")
        # 5: the node returns, a star is born, metrics back
        reload(nd, base, [A_GONE], rng)
        star(nd, A_STAR, NOW)
        reload(nd, base, lose, rng)
        heat(nd, base, flip, 10)
        s.upsert(np.concatenate([[A_GONE, A_STAR], lose, flip, hot[:1]]), "node back, star, metric back")
        s.check(NOW, "star")
        s.place(NOW, "place 1 (oracle)")
        s.check(NOW, "after place 1")
        # 6: whole rows overwrite committed ones
        w = np.concatenate([some(30), [A_STAR]])
        reload(nd, base, w, rng)
        s.upsert(w, "load 31 over committed rows")
        s.check(NOW, "after load 30")
        return s
    # 4: back inside the bounds
    w = np.array(A_OUT["alloc"] + A_OUT["base"])
    reload(nd, base, w, rng)
    s.upsert(np.concatenate([w, hot]), "back in bounds")
    s.check(NOW, "back in bounds")
    # 5: metrics lost, LoadAware-pass flags flip
    drop_metric(nd, lose)
    heat(nd, base, flip, 90)
    s.upsert(np.concatenate([lose, flip]), "metric lost, flags flip")
    s.check(NOW, "metric lost")
    # 6: the removed node returns valid; a node becomes the best of the batch
    reload(nd, base, [A_GONE], rng)
    star(nd, A_STAR, NOW)
    s.upsert([A_GONE, A_STAR] + list(A_HOT), "node back, star")
    s.check(NOW, "star")
    # 7: metrics back, flags back; 22 nodes' metrics age (fresh at NOW, expired 100 s later)
    reload(nd, base, lose, rng)
    heat(nd, base, flip, 10)
    nd["update_time_ns"][stale] = NOW - 250 * SEC
    s.upsert(np.concatenate([lose, flip, stale]), "metric back, 22 ageing")
    s.check(NOW, "before expiry")
    # 8: no delta, the clock alone moves
    s.check(NOW + 100 * SEC, "after expiry")
    # the first place: still the oracle's sequential cycle on the edited view
    s.place(NOW, "place 1 (oracle)")
    s.check(NOW, "after place 1")
    # 9: whole rows overwrite committed ones; out of bounds again
    w = np.concatenate([some(30), [A_STAR]])
    reload(nd, base, w, rng)
    out_alloc(nd, list(A_OUT2["alloc"]))
    out_base(nd, list(A_OUT2["base"]))
    s.upsert(np.concatenate([w, A_OUT2["alloc"], A_OUT2["base"]]), "load 30 over committed rows, 8 out of bounds")
    s.check(NOW, "rows after commit")
    # 10: back inside
    w = np.array(A_OUT2["alloc"] + A_OUT2["base"])
    reload(nd, base, w, rng)
    s.upsert(np.concatenate([w, hot]), "8 back in bounds")
    s.check(NOW + 100 * SEC, "back in bounds, later clock")
    # 11: one row
    reload(nd, base, hot[:1], rng)
    s.upsert(hot[:1], "one row")
    s.check(NOW, "one row")
    w = some(15)
    reload(nd, base, w, rng)
    s.upsert(w, "load 15")
    s.check(NOW, "after load 15")
    # the second place: the replay on the model rows
    s.place(NOW, "place 2 (replay)")
    # 12
    w = some(25)
    reload(nd, base, w, rng)
    s.upsert(w, "load 25")
    s.check(NOW, "final")
    return s


# ---- scenario B: batch swaps --------------------------------------------------------------------------------------------
B_POOL = 900
B_FIT = {"cpu": 1, "memory": 1, BATCH_CPU: 1, BATCH_MEM: 1, "nvidia.com/gpu": 2, "koordinator.sh/gpu-core": 1,
         "kubernetes.io/mid-cpu": 1, "kubernetes.io/mid-memory": 1}
B_EIGHT = 0x3 | 1 << nat.RES_BATCH_CPU | 1 << nat.RES_BATCH_MEMORY | 1 << nat.RES_EXT0 | 1 << nat.RES_EXT1 | \
    1 << nat.RES_MID_CPU | 1 << nat.RES_MID_MEMORY


class Pool:
    """The pod pool of scenario B with each pod's needed resources, Fit weight sum and prod-score flag."""


@functools.lru_cache(maxsize=None)
def b_pool():
    cl = wc.wide_cluster(N, B_POOL, 57)
    # every pending pod gets a cpu (or batch-cpu) request of its own, so every pod row is distinct
    cont = cl.containers
    for i in range(B_POOL):
        c = int(cl.pods["first_container"][i])
        for rl in (cont["requests"], cont["limits"]):
            for r in (CPU, nat.RES_BATCH_CPU):
                if rl["present"][c] & np.uint32(1 << r):
                    rl["v"][c, r] += i
    cfg = shipped_profile(extended_resources=wc.EXT_NAMES, fit_resources=B_FIT, score_according_prod_usage=True)
    p = Pool()
    p.cl, p.cfg = cl, cfg
    p.rows = engine.build_pod_rows(cfg, cl, np.arange(B_POOL))
    p.need = wc.pod_need(cfg, p.rows)
    p.fit_w = pod_fit_w(cfg, p.rows)
    p.prod = (p.rows["flags"] & nat.POD_LA_PROD_SCORE) != 0
    return p


def _pick(sel, k, rng=None):
    idx = np.flatnonzero(sel)
    assert len(idx) >= k, (len(idx), k)
    return idx[:k] if rng is None else np.sort(rng.choice(idx, k, replace=False))


@functools.lru_cache(maxsize=None)
def scenario_b():
    p = b_pool()
    rng = np.random.default_rng(61)
    s = Script("b_swaps", p.cfg, p.cl)
    nd, base = s.nodes, s.base
    pow2 = is_pow2(p.fit_w)
    two = p.need == 0x3                                              # cpu + memory: 2 slots, prod pods
    four = ((p.need & ~0x1B) == 0) & ((p.need & 0x18) != 0)          # batch pods: 4 slots, not prod
    eight = ((p.need & ~B_EIGHT) == 0) & ((p.need & ~0x1B) != 0)     # a named scalar or mid resource: 8 slots
    masks = elig_cases.class_masks(N)
    s.elig(masks)
    s.pods(_pick(two & pow2 & p.prod, 96), label="96 cpu/memory pods: 2 slots, class path, la_prod on (growth)")
    s.check(NOW, "b1")
    s.pods(np.concatenate([_pick(eight & ~pow2, 5), _pick(eight & pow2, 3)]),
           label="8 pods: 8 slots, slot path (a weight sum of 3), smaller than the buffers")
    s.check(NOW, "b2")
    s.pods(_pick(four & pow2 & ~p.prod, 1), label="1 batch pod: 4 slots, class path, la_prod off")
    s.check(NOW, "b3")
    s.pods(_pick(two & pow2 & p.prod, 65, rng), label="65 cpu/memory pods: 2 slots, la_prod on")
    s.check(NOW, "b4")
    s.pods(rng.choice(B_POOL, 96, replace=False), label="96 pods over more than 8 resources: spill pods")
    s.check(NOW, "b5")
    s.pods(_pick(eight | four | two, 96, rng), label="96 pods within 8 resources: no spill pods")
    s.check(NOW, "b6")
    w = rng.choice(N, 40, replace=False)
    reload(nd, base, w, rng)
    out_alloc(nd, w[:4])
    s.upsert(np.concatenate([w, CORNERS]), "delta 1")
    cls = np.array([(0, 1, 2, 3)[i % 4] for i in range(64)], np.int32)
    s.pods(_pick(two | four, 64, rng), elig=cls, label="64 pods, three in four restricted (classes 1..3)")
    s.check(NOW, "b7")
    s.pods(_pick(two | four, 63, rng), label="63 pods, none restricted")
    s.check(NOW, "b8")
    s.elig_update(0, np.arange(0, N, 3), False)
    s.elig_update(2, [0, 1, 2098], True)
    w = rng.choice(N, 30, replace=False)
    reload(nd, base, w, rng)
    s.upsert(w, "delta 2")
    cls = np.array([(1, 3, 0, 2, 1)[i % 5] for i in range(65)], np.int32)
    s.pods(_pick(two | four, 65, rng), elig=cls, label="65 pods restricted again, after update_eligibility")
    s.check(NOW, "b9")
    few = _pick(two & pow2, 6, rng)
    s.pods(few[rng.integers(0, 6, 96)], label="96 pods over 6 rows: k_eval3_dup")
    s.check(NOW, "b10")
    s.pods(_pick(pow2 & (two | four), 96, rng), label="96 distinct rows, class path")
    s.check(NOW, "b11")
    return s


# ---- scenario C: a moving shard under one batch -----------------------------------------------------------------------
C_SHARDS = ((0, N), (1024, N), (0, 1024), (2048, N), (0, N))


@functools.lru_cache(maxsize=None)
def scenario_c():
    rng = np.random.default_rng(71)
    s = Script("c_shard", shipped_profile(place_chunk=16), synth.make_cluster(N, 65, seed=72))
    s.pods(np.arange(65), label="65 pods, class path")
    for k, (b, e) in enumerate(C_SHARDS):
        if k == 3:
            w = np.concatenate([rng.choice(N, 36, replace=False), CORNERS])
            reload(s.nodes, s.base, w, rng)
            out_alloc(s.nodes, [2050, 1030])
            star(s.nodes, 2090, NOW)
            s.upsert(np.concatenate([w, [2050, 1030, 2090]]), "delta between shards")
        s.shard(b, e)
        s.check(NOW, f"shard {b}:{e}")
    s.shard(1024, N)
    s.place(NOW, "place at shard 1024:2100")
    s.check(NOW, "after place")
    return s


# ---- scenario D: NodeNUMAResource ---------------------------------------------------------------------------------------
def _zones(s, which, rng):
    """Rewrite the zones' allocated cpu / memory of nodes `which` (free amounts change)."""
    for j in np.asarray(which).tolist():
        for z in range(int(s.numa["n_zones"][j])):
            tot, al = s.numa["zone_total"][j, z], s.numa["zone_allocated"][j, z]
            al["v"][CPU] = int(tot["v"][CPU]) * int(rng.integers(0, 91)) // 100 // 1000 * 1000
            al["v"][MEM] = int(tot["v"][MEM]) // 100 * int(rng.integers(0, 91))
            al["present"] |= np.uint32(0x3)


def _toggle(s, which):
    """The node's topology policy moves on: None → Restricted → SingleNUMANode → None."""
    order = (nat.NUMA_NONE, nat.NUMA_RESTRICTED, nat.NUMA_SINGLE_NUMA_NODE)
    for j in np.asarray(which).tolist():
        s.numa["policy"][j] = order[(order.index(int(s.numa["policy"][j])) + 1) % 3]


@functools.lru_cache(maxsize=None)
def scenario_d():
    rng = np.random.default_rng(81)
    # (2 to 4 zones: the oracle's hint enumeration over 8 zones would take most of the test's time)
    cl = synth.make_numa_cluster(N, 100, seed=82, zones=(2, 3, 4), distinct_pods=True)
    assert not cl.pods["cpu_bind_required"][:100].any()
    cfg = numa_config(place_chunk=16)
    s = Script("d_numa", cfg, cl, forms=nat.FORM_PLACE_PIPELINE)
    eq = np.concatenate([np.arange(70), rng.integers(0, 70, 26)])       # 96 pods over 70 rows: eq_on, eq_perm_on
    rng.shuffle(eq)
    s.pods(eq, label="96 pods over 70 rows: eq_on, eq_perm_on")
    s.check(NOW, "d1")
    w = np.concatenate([rng.choice(N, 36, replace=False), CORNERS])
    _zones(s, w, rng)
    _toggle(s, w[:12])
    s.upsert(w, "zones rewritten, 12 policies toggled")
    s.check(NOW, "d2")
    s.pods(np.arange(30, 95), label="65 distinct rows: eq_on off")
    s.check(NOW, "d3")
    s.place(NOW, "place (pipelined)")
    # nodes the place touched (the oracle's cycle says which) are rewritten whole, with others
    m = Model(s)
    for st in s.steps:
        if st.kind == "upsert":
            m.upsert(st)
        elif st.kind == "pods":
            m.pods(st)
    placed, _, _ = m.place(s.steps[-1])
    hit = np.unique(placed[placed >= 0])[:20]
    s.placed_nodes = hit
    w = np.concatenate([hit, rng.choice(N, 10, replace=False)])
    _zones(s, w, rng)
    _toggle(s, w[:5])
    s.upsert(w, "zones of placed nodes rewritten")
    s.check(NOW, "d4 (twin)")
    return s


# ---- scenario E: LoadAware extra resources --------------------------------------------------------------------------
E_OUT1 = (0, 1023, 1024, 2099, 517, 2055)
E_OUT2 = (1, 1022, 2048, 2098, 1400)


@functools.lru_cache(maxsize=None)
def scenario_e():
    import matrix_cases as mc
    cl = synth.make_la_extra_cluster(N, 48, seed=91)
    cfg = shipped_profile(resource_weights=mc.LA_W, estimated_scaling_factors=mc.LA_SF)
    s = Script("e_la_extra", cfg, cl)
    nd, base = s.nodes, s.base

    def push(which):
        for j in which:   # ephemeral-storage usage beyond 2^50 on a node that reports the resource and a metric
            _set(nd["allocatable"], j, EPH, 400 * GI)
            for f in ("has_node_metric", "has_update_time", "has_report_interval", "has_node_metric_info"):
                nd[f][j] = 1
            nd["update_time_ns"][j] = NOW - 30 * SEC
            _set(nd["node_usage"], j, CPU, 1000)
            _set(nd["node_usage"], j, EPH, VAL_LIMIT + 9)

    s.pods(np.arange(48), label="48 pods, k_eval2's LAX form")
    s.check(NOW, "e1")
    push(E_OUT1)
    s.upsert(E_OUT1, "6 nodes' ephemeral-storage usage past the bound")
    s.check(NOW, "e2")
    nd[list(E_OUT1)] = base[list(E_OUT1)]
    push(E_OUT2)
    s.upsert(E_OUT1 + E_OUT2, "6 back, 5 others out")
    s.check(NOW, "e3")
    nd[list(E_OUT2)] = base[list(E_OUT2)]
    s.upsert(E_OUT2, "5 back")
    s.check(NOW, "e4")
    return s


# ---- scenario F: reservations -------------------------------------------------------------------------------------------
F_PLUGINS = ("NodeResourcesFit", "LoadAwareScheduling", "Reservation")


@functools.lru_cache(maxsize=None)
def scenario_f():
    rng = np.random.default_rng(101)
    cl = synth.make_rsv_cluster(N, 65, seed=102, rsv_node_frac=0.1)
    cfg = shipped_profile(plugins=F_PLUGINS)
    s = Script("f_rsv", cfg, cl)
    rsv0 = cl.rsv_arr.copy()
    holders = np.unique(rsv0["node"])
    free = np.setdiff1d(np.arange(N), holders)
    s.set_rsv(rsv0, "set_reservations: the cluster's slots")
    s.pods(np.arange(65), label="65 batch pods")
    s.check(NOW, "f1")
    free20 = rng.choice(free[(free > 0) & (free < N - 1)], 20, replace=False)
    w = np.concatenate([holders[:10], holders[-3:], free20, [0, N - 1]])
    reload(s.nodes, s.base, w, rng)
    # outside the fp64 bounds: two holders that will lose their slots, two nodes that will gain their first, two others
    s.slow_nodes = np.concatenate([holders[:2], free20[:4]])
    out_alloc(s.nodes, s.slow_nodes)
    for r in (nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY):   # batch pods: the batch resources' load moves too
        a = s.base["allocatable"]["v"][w, r]
        s.nodes["requested"]["v"][w, r] = a // 100 * rng.integers(0, 50, len(w))
    s.upsert(w, "rows of slot holders and of others")
    s.check(NOW, "f2")
    # another slot set: the first third of the holders lose every slot, nodes without one gain their first
    rsv1 = rsv0.copy()
    losers = holders[: len(holders) // 3]
    gain = np.concatenate([free20[:2], rng.choice(np.setdiff1d(free, free20), len(losers) - 2, replace=False)])
    for a, b in zip(losers.tolist(), gain.tolist()):
        rsv1["node"][rsv1["node"] == a] = b
    rsv1 = rsv1[np.argsort(rsv1["node"], kind="stable")]
    s.losers, s.gainers = losers, np.sort(gain)
    s.set_rsv(rsv1, "set_reservations: a third of the holders lose all, others gain their first")
    s.check(NOW, "f3")
    return s


# ---- scenario G: duplicate indices in one upsert ----------------------------------------------------------------------
class DupCase:
    pass


@functools.lru_cache(maxsize=None)
def dup_case():
    """600 entries over 300 nodes, each twice (first, then last, anywhere in the call): the two rows of a node differ in
    allocatable, requested and usage, and for half of the nodes one of the two is outside the fp64 bounds."""
    rng = np.random.default_rng(111)
    cl = synth.make_cluster(N, 64, seed=112)
    cfg = shipped_profile()
    c = DupCase()
    c.cfg, c.cl = cfg, cl
    sel = np.concatenate([CORNERS, rng.choice(np.setdiff1d(np.arange(N), CORNERS), 296, replace=False)])
    first, last = cl.nodes.copy(), cl.nodes.copy()
    for k, nodes in enumerate((first, last)):
        reload(nodes, cl.nodes, sel, rng)
        nodes["allocatable"]["v"][sel, CPU] += 1000 * (1 + k)
        nodes["allocatable"]["v"][sel, MEM] += GI * (1 + k)
    out_alloc(first, sel[0:150:2])      # the superseded row is outside, the last one inside
    out_alloc(last, sel[1:150:2])       # the other way round
    out_base(last, sel[1:40:4])
    c.view_first, c.view_last = cl.with_nodes(first), cl.with_nodes(last)
    c.rows_first = engine.build_node_rows(cfg, c.view_first, sel)
    c.rows_last = engine.build_node_rows(cfg, c.view_last, sel)
    # one call: a random order in which each node's first entry precedes its last
    pos = rng.permutation(600)
    a, b = np.minimum(pos[:300], pos[300:]), np.maximum(pos[:300], pos[300:])
    c.idx = np.zeros(600, np.int32)
    c.rows = np.zeros(600, nat.NODE_ROW)
    c.idx[a], c.idx[b] = sel, sel
    c.rows[a], c.rows[b] = c.rows_first, c.rows_last
    c.sel = sel
    c.expect = engine.build_node_rows(cfg, c.view_last)
    c.pod_idx = np.arange(64)
    return c


SCENARIOS = {
    "a_class": lambda: scenario_a(False),
    "a_slot": lambda: scenario_a(True),
    "b_swaps": scenario_b,
    "c_shard": scenario_c,
    "d_numa": scenario_d,
    "e_la_extra": scenario_e,
    "f_rsv": scenario_f,
}


def script(name):
    return SCENARIOS[name]()
