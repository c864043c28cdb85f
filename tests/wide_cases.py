"""Wide clusters: batches whose pods compare or score more than 8 resources, so kg_pods_set's 8-slot map cannot
hold them all and some pods are spill pods (kg_batch_slot_map; evaluated by k_eval_spill on the generic pair path).

wide_cluster(N, P, seed) starts from synth.make_scalar_cluster (cpu, memory, batch-cpu, batch-memory and the named
slots RES_EXT0..3), gives ephemeral-storage to every node and mid-cpu, mid-memory and RES_EXT4 to about two nodes in
three (partly requested), and adds requests (= limits) for each of those four to about a quarter of the containers.
Configs name the fifth slot: extended_resources = EXT_NAMES.

TEST INFRASTRUCTURE shared by tests/test_wide_batch_cpu.py and tests/test_wide_batch_gpu.py; the oracle's answers are
computed once per case and handed out read-only.
"""
import functools

import numpy as np

from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile

GI, MI = 1 << 30, 1 << 20
EXT_NAMES = synth.SCALAR_NAMES + ("example.com/fpga",)
WIDE_RES = (nat.RES_EPHEMERAL_STORAGE, nat.RES_MID_CPU, nat.RES_MID_MEMORY, nat.RES_EXT4)

# NodeResourcesFit profiles of the matrix tests: LeastAllocated over 9 resources (weight sum 10) and MostAllocated
# over 4 with a non-power-of-two weight sum (6)
FIT9 = {"cpu": 1, "memory": 1, "kubernetes.io/batch-cpu": 1, "kubernetes.io/batch-memory": 1,
        "kubernetes.io/mid-cpu": 1, "kubernetes.io/mid-memory": 1, "ephemeral-storage": 1, "nvidia.com/gpu": 2,
        "koordinator.sh/gpu-core": 1}
MOST4 = {"cpu": 1, "memory": 1, "nvidia.com/gpu": 1, "kubernetes.io/mid-memory": 3}
PROFILES = {
    "least9": dict(fit_resources=FIT9),
    "most4": dict(fit_strategy="MostAllocated", fit_resources=MOST4),
}


def wide_config(name="least9", **kw):
    return shipped_profile(extended_resources=EXT_NAMES, **PROFILES[name], **kw)


def numa_wide_config(**kw):
    return make_config(plugins=("NodeResourcesFit", "LoadAwareScheduling", "NodeNUMAResource"),
                       extended_resources=EXT_NAMES, fit_resources=FIT9, **kw)


def _view(base, cont, nodes):
    return synth.SynthView(base.pods, cont, nodes, base.now_ns, base.numa_arr, base.rsv_arr, base.quota_arr,
                           base.aggregated_arr, base.pod_metrics_arr, base.assigned_arr)


def _named_scalars(base, seed, lo):
    """synth.make_scalar_cluster's named slots RES_EXT0..3 on another base cluster (requests of at least `lo`)."""
    rng = np.random.default_rng(seed + 5151)
    nodes, cont = base.nodes.copy(), base.containers.copy()
    n, c = len(nodes), len(cont)
    caps = {nat.RES_EXT0: 9, nat.RES_EXT1: 801, nat.RES_EXT2: 5, nat.RES_EXT3: 65}
    wants = rng.random(c) < 0.4
    for r, hi in caps.items():
        unit = 2 * MI if r == nat.RES_EXT3 else 1
        has = rng.random(n) < 0.6
        a = rng.integers(0, hi, n) * unit
        synth._rl_fill(nodes["allocatable"], r, a, has)
        synth._rl_fill(nodes["requested"], r, (a * rng.integers(0, 5, n)) // 4, has & (rng.random(n) < 0.7))
        pick = wants & (rng.random(c) < 0.5)
        v = rng.integers(lo, max(2, hi // 3), c) * unit
        synth._rl_fill(cont["requests"], r, v, pick)
        synth._rl_fill(cont["limits"], r, v, pick)
    return _view(base, cont, nodes)


def wide_cluster(N, P, seed, numa=False):
    """numa: on synth.make_numa_cluster instead (NodeNUMAResource zones), every scalar request at least 1 (a
    zero-valued key is a NUMA hint list of its own, and the engine answers at most two lists per pod)."""
    if numa:
        base = _named_scalars(synth.make_numa_cluster(N, P, seed), seed, 1)
    else:
        base = synth.make_scalar_cluster(N, P, seed)
    rng = np.random.default_rng(seed + 8181)
    nodes, cont = base.nodes.copy(), base.containers.copy()
    n, c = len(nodes), len(cont)
    cpu = nodes["allocatable"]["v"][:, nat.RES_CPU]
    mem = nodes["allocatable"]["v"][:, nat.RES_MEMORY]
    node_cap = {
        nat.RES_EPHEMERAL_STORAGE: rng.choice(np.array([100, 200, 400, 800], np.int64), n) * GI,
        nat.RES_MID_CPU: (cpu * rng.integers(10, 41, n)) // 100,
        nat.RES_MID_MEMORY: (mem // 100) * rng.integers(10, 41, n),
        nat.RES_EXT4: rng.integers(0, 9, n),
    }
    pod_req = {
        nat.RES_EPHEMERAL_STORAGE: rng.integers(1, 120, c) * GI,
        nat.RES_MID_CPU: rng.choice(np.array([250, 500, 1000, 2000, 8000], np.int64), c),
        nat.RES_MID_MEMORY: rng.choice(np.array([256, 1024, 4096, 32768], np.int64), c) * MI,
        nat.RES_EXT4: rng.integers(1 if numa else 0, 4, c),
    }
    for r in WIDE_RES:
        has = np.ones(n, bool) if r == nat.RES_EPHEMERAL_STORAGE else rng.random(n) < 0.65
        synth._rl_fill(nodes["allocatable"], r, node_cap[r], has)
        synth._rl_fill(nodes["requested"], r, (node_cap[r] * rng.integers(0, 71, n)) // 100, has & (rng.random(n) < 0.7))
        pick = rng.random(c) < 0.25
        synth._rl_fill(cont["requests"], r, pod_req[r], pick)
        synth._rl_fill(cont["limits"], r, pod_req[r], pick)
    return _view(base, cont, nodes)


def slot_map_rule(need):
    """The rule of kg_batch_slot_map restated: `need` = one resource bit mask per pod.  Returns (n_slots, slot_res
    [8], spill [P] bool)."""
    need = np.asarray(need, dtype=np.int64)
    uni = int(np.bitwise_or.reduce(need)) if len(need) else 0
    none = np.zeros(len(need), bool)
    if not uni & ~0x3:
        return 2, [0, 1] + [-1] * 6, none
    if not uni & ~0x1B:
        return 4, [0, 1, nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY] + [-1] * 4, none
    others = [r for r in range(2, nat.NUM_RES) if (uni >> r) & 1]
    if len(others) > 6:
        count = {r: int(((need >> r) & 1).sum()) for r in others}
        others = sorted(sorted(others, key=lambda r: (-count[r], r))[:6])
    held = 0x3 | sum(1 << r for r in others)
    return 8, [0, 1] + others + [-1] * (6 - len(others)), (need & ~held) != 0


def pod_need(cfg, rows):
    """The resources each pod row needs a slot for (kg_pod_hot_from_row's `need`): compared by the Fit filter (natives
    with a non-zero request, scalar keys present) or scored by NodeResourcesFit."""
    fit_on = bool(int(cfg["enabled_plugins"]) & nat.PLUGIN_FIT)
    out = np.zeros(len(rows), np.int64)
    if not fit_on:
        return out
    w = cfg["fit_resource_weight"]
    for i, p in enumerate(rows):
        need = 0
        if p["flags"] & nat.POD_HAS_REQUEST:
            for r in range(3):
                if p["request"][r] != 0:
                    need |= 1 << r
            need |= int(p["request_present"]) & 0xFF8
        for r in range(nat.NUM_RES):
            if w[r] > 0 and not (r >= 3 and p["fit_score_request"][r] == 0):
                need |= 1 << r
        out[i] = need
    return out


class Case:
    """One wide batch: cluster, config, node and pod rows, and (lazily, once) the oracle's answers."""

    def __init__(self, N, P, seed, profile="least9", idx=None, numa=False, edit=None, **cfg_kw):
        self.N, self.seed, self.numa = N, seed, numa
        self.cl = wide_cluster(N, P, seed, numa=numa)
        if edit is not None:
            edit(self.cl, P)
        self.cfg = numa_wide_config(**cfg_kw) if numa else wide_config(profile, **cfg_kw)
        self.idx = np.arange(P) if idx is None else np.asarray(idx)
        self.P = len(self.idx)
        self.node_rows = engine.build_node_rows(self.cfg, self.cl)
        self.pod_rows = engine.build_pod_rows(self.cfg, self.cl, self.idx)
        self.n_slots, self.slot_res, self.spill = engine.batch_slot_map(self.cfg, self.pod_rows)
        for a in (self.node_rows, self.pod_rows, self.spill):
            a.setflags(write=False)

    @functools.cached_property
    def matrix(self):
        from oracle import oracle
        out = oracle.eval_matrix(self.cfg, self.cl, self.idx, self.cl.now_ns)
        for a in out:
            a.setflags(write=False)
        return out

    def matrix3(self, begin=0, end=None):
        from oracle import oracle
        return oracle.eval_matrix3(self.cfg, self.cl, self.idx, self.cl.now_ns, begin, self.N if end is None else end)

    @functools.cached_property
    def schedule(self):
        from oracle import oracle
        out = oracle.schedule(self.cfg, self.cl, self.idx, self.cl.now_ns)
        for a in out:
            a.setflags(write=False)
        return out

    def replay(self, nodes):
        """The snapshot after the placements `nodes`, by the host Reserve (kg_row_commit)."""
        rows = self.node_rows.copy()
        for p, n in enumerate(np.asarray(nodes).tolist()):
            if n >= 0:
                engine.row_commit(self.cfg, rows[n:n + 1], self.pod_rows[p:p + 1])
        return rows

    def check_mixed(self, mask=None):
        """The preconditions of a mixed batch: 25 %–75 % spill pods, each with a feasible and an infeasible node."""
        share = self.spill.mean()
        assert self.n_slots == 8 and 0.25 <= share <= 0.75, share
        self.check_spill_rows(mask)

    def check_spill_rows(self, mask=None):
        m = self.matrix[0] if mask is None else mask
        assert self.spill.any()
        feas = m[self.spill].sum(axis=1)
        assert (feas >= 1).all() and (feas < m.shape[1]).all(), (feas.min(), feas.max(), m.shape[1])


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


SMALL = {nat.RES_EPHEMERAL_STORAGE: GI, nat.RES_MID_CPU: 100, nat.RES_MID_MEMORY: 64 * MI, nat.RES_EXT4: 1}


def _containers_of(cl, P):
    """The containers of the P pending pods (one each)."""
    assert (cl.pods["n_containers"][:P] == 1).all()
    return cl.pods["first_container"][:P]


def _only(pod):
    """Pod `pod` (negative: from the end) requests all four wide resources; every other pod loses them and the named
    slots RES_EXT2 / RES_EXT3, so the others' union stays within 8 resources and only `pod` is a spill pod."""
    def edit(cl, P):
        ci = _containers_of(cl, P)
        keep = ci[pod]
        others = ci[ci != keep]
        drop = np.uint32(sum(1 << r for r in WIDE_RES + (nat.RES_EXT2, nat.RES_EXT3)))
        for arr in (cl.containers["requests"], cl.containers["limits"]):
            arr["present"][others] &= ~drop
            for r in WIDE_RES + (nat.RES_EXT2, nat.RES_EXT3):
                arr["v"][others, r] = 0
            for r in WIDE_RES:
                arr["v"][keep, r] = SMALL[r]
                arr["present"][keep] |= np.uint32(1 << r)
    return edit


def _all_wide(cl, P):
    """Every pod requests all four wide resources (small amounts) and carries the keys of three named slots (zero-
    valued where it did not request them) next to what it has: each pod alone needs more than 8 resources."""
    ci = _containers_of(cl, P)
    for arr in (cl.containers["requests"], cl.containers["limits"]):
        for r in WIDE_RES:
            arr["v"][ci, r] = SMALL[r]
            arr["present"][ci] |= np.uint32(1 << r)
        for r in (nat.RES_EXT0, nat.RES_EXT1, nat.RES_EXT2):
            arr["present"][ci] |= np.uint32(1 << r)


def _ten(cl, P):
    """Pod 0 requests 10 resources, all non-zero."""
    k = _containers_of(cl, P)[0]
    want = {nat.RES_CPU: 500, nat.RES_MEMORY: GI, nat.RES_BATCH_CPU: 100, nat.RES_BATCH_MEMORY: 64 * MI,
            nat.RES_EXT0: 1, nat.RES_EXT1: 1, **SMALL}
    for arr in (cl.containers["requests"], cl.containers["limits"]):
        arr["v"][k] = 0
        arr["present"][k] = 0
        for r, v in want.items():
            arr["v"][k, r] = v
            arr["present"][k] |= np.uint32(1 << r)


SEED = 81
CASES = {
    "matrix_least9": lambda: Case(1_100, 300, SEED, "least9"),
    "matrix_most4": lambda: Case(1_100, 300, SEED, "most4"),
    "shard": lambda: Case(3_000, 120, SEED + 1, "least9"),
    "first": lambda: Case(1_100, 37, SEED + 2, "least9", edit=_only(0)),
    "last": lambda: Case(1_100, 37, SEED + 2, "least9", edit=_only(-1)),
    "all": lambda: Case(1_100, 37, SEED + 2, "least9", edit=_all_wide),
    "ten": lambda: Case(1_100, 37, SEED + 2, "least9", edit=_ten),
    "numa_eq": lambda: Case(1_100, 24, SEED + 3, numa=True,
                            idx=np.random.default_rng(SEED + 3).integers(0, 24, 64)),
    "place": lambda: Case(1_100, 400, SEED + 4, "least9", place_chunk=16),
    "place1": lambda: Case(1_100, 400, SEED + 4, "least9", place_chunk=1),
}
