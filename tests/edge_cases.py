"""The step-edge cluster: operands that sit on the steps of the score quotients.

The pair score of the fast path is `max((int)fma(-pr, R, F), 0)` (kg_common.h header) and must equal Go's
`(cap - req) * 100 / cap`, req = base(node) + pr(pod).  The quotient steps down exactly where req passes
`cap - ceil(k * cap / 100)`: that request still scores k and the next one scores k - 1 (caps of at least 100).  The
synthetic clusters of koordinator_amd.synth never come near such a step (power-of-two memory, whole percentages);
here every aligned node sits on one, for each of the six scored operands ("slots"):

    slot 0 / 1   NodeResourcesFit cpu / memory          base = NonZeroRequested
    slot 2 / 3   NodeResourcesFit batch-cpu / -memory   base = Requested (also the Fit filter's operand)
    slot 4 / 5   LoadAwareScheduling cpu / memory       base = the NodeMetric usage

Pods come in adjacent pairs (pr, pr + 1).  Pair j holds four pods: 4j, 4j + 1 request cpu and memory with a limit
above the request (their LoadAware estimate is then the limit itself, so the four effective requests of slots 0, 1, 4,
5 are free to choose), 4j + 2, 4j + 3 request batch-cpu and batch-memory (slots 2, 3).  Pair j belongs to cap class
j mod C and has small requests (j < C) or requests just below cap / 100 (j >= C: up to about 2^34 on the caps next
to 2^41), so that every quotient 1..99 is reachable with a non-negative base.

Aligned node i (i < N_ALIGNED = C * 101) has cap CAPS[i mod C] on every slot, pod pair i mod J, and per slot s the
target quotient k = slot_k(i, s); its base makes `base + pr` the last request that scores k (LeastAllocated; for
MostAllocated the mirror: `base + pr + 1` is the first request that scores k).  Where that base would be negative
(k too high for the pair's request) it is 0 and the node is simply not on a step.  The LoadAware filter is switched off
per node (custom usage thresholds of 0), requested cpu / memory is 0, so the aligned pairs are feasible.

After the aligned nodes: FILTER nodes whose Fit filter operand is exact (free == request and free == request - 1 at
2^33 + 5 and at the largest request the engine admits, KG_VAL_LIMIT - 1), BIG nodes whose bases reach 2^50 - 1 with
base > cap (scores clamp to 0, MostAllocated to 100), with `negative` the NEG nodes (bases in (-2^49, 0) whose sum with
a designated pod's request lies in [0, cap]; three recorded operand tuples first; a pod that is not designated
for such a node would have base + pr < 0, a score above 100 in the reference too, so the tuple pods are kept off the
sweep nodes and off each other's nodes by a request (NEG_GATE) only their own tuple's node can hold, the sweep pods' request exceeds every tuple's, and the
negative tests evaluate the designated pods alone and compare scores where the pair is feasible), and with `wide` every node carries
eight more resources and twelve more pods request one each (a batch of more than 8 resources: spill pods).

TEST INFRASTRUCTURE shared by tests/test_score_edges_cpu.py and tests/test_score_edges_gpu.py; clusters and oracle
answers are computed once and handed out read-only.
"""
import functools

import numpy as np

from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile
from oracle import oracle

CAP_LIMIT, VAL_LIMIT = 1 << 41, 1 << 50      # KG_CAP_LIMIT, KG_VAL_LIMIT (kg_common.h)
CAPS = ((1 << 41) - 1, (1 << 41) - 3, (1 << 40) + 1, 10**12 + 39, 3 * (1 << 39) - 1, 1, 2, 3, 7, 99, 100, 101, 12_800,
        1 << 36)
C = len(CAPS)
J = 2 * C                                    # pod pairs: class j mod C, small (j < C) or large (j >= C) requests
N_ALIGNED = C * 101                          # 1,414: past one 1,024-node tile
N_PAIR_PODS = 4 * J
SLOTS = 6
SLOT_NAMES = ("fit cpu", "fit memory", "fit batch-cpu", "fit batch-memory", "loadaware cpu", "loadaware memory")
# (chosen so that, under the configs of CONFIGS, some pods' best node wins by one point and some pods' two best
# nodes lie in different 1,024-node tiles: tests/test_score_edges_cpu.py asserts both)
_K_MUL, _K_ADD = (52, 49, 11, 25, 70, 90), (11, 95, 32, 7, 92, 52)
BATCH_CPU, BATCH_MEM = "kubernetes.io/batch-cpu", "kubernetes.io/batch-memory"
EXT_NAMES = synth.SCALAR_NAMES + ("example.com/fpga",)
WIDE_RES = (nat.RES_EPHEMERAL_STORAGE, nat.RES_MID_CPU, nat.RES_MID_MEMORY, nat.RES_EXT0, nat.RES_EXT1, nat.RES_EXT2,
            nat.RES_EXT3, nat.RES_EXT4)
FILTER_REQ = ((1 << 33) + 5, VAL_LIMIT - 1)  # the exact Fit filter operands (memory / batch-memory)
# (cap, base, pr): fast-path LeastAllocated quotients that were off by one before negative bases left the fast path
NEG_TUPLES = ((6, -531169216302749, 531169216302750), (13, -295819977655557, 295819977655560),
              (2199023254720, -462544787795525, 463754250585621))
NEG_GATE = (nat.RES_MID_CPU, nat.RES_MID_MEMORY, nat.RES_EPHEMERAL_STORAGE)   # tuple t's pods fit only its own node
NEG_X = (1 << 49) - (1 << 40)                # the request of the negative variant's sweep pods (LoadAware: + 7)


def slot_k(i, s):
    """Target quotient of slot s on aligned node i: every k in 0..100 once per cap class, another order per slot."""
    return ((i // C) * _K_MUL[s] + _K_ADD[s]) % 101


def ceil_div(n, d):
    return -((-n) // d)


def pair_requests(j):
    """Effective requests (pr of the pair's first pods; the second ones add 1) of pair j on the six slots."""
    a = CAPS[j % C]
    if j >= C and a >= 12_800:
        h = a // 100
        return (h - 10, h - 11, h - 3, h - 5, h - 2, h - 4)
    if a < 12_800:   # cap / 100 is at most 1: only the smallest requests reach the high quotients
        return (1, 1, 1, 1, 2, 2) if j < C else (2, 2, 2, 2, 3, 3)
    c = 1 + j % C
    return (c, c + 1, c, c + 2, c + 1 + c % 3, c + 2 + c % 2)


def step_base(a, k, pr, most):
    """The base that puts `base + pr` on the step of quotient k (see the module docstring); 0 where unreachable."""
    e = ceil_div(k * a, 100) - 1 if most else a - ceil_div(k * a, 100)
    return max(e - pr, 0)


def least(req, a):
    return 0 if a == 0 or req > a else (a - req) * 100 // a


def most(req, a):
    return 0 if a == 0 else min(req, a) * 100 // a


def _set(rl, idx, r, v):
    rl["v"][idx, r] = v
    rl["present"][idx] |= np.uint32(1 << r)


def _ls_pod(cont, p, cpu, mem, lcpu, lmem):
    _set(cont["requests"], p, nat.RES_CPU, cpu)
    _set(cont["requests"], p, nat.RES_MEMORY, mem)
    _set(cont["limits"], p, nat.RES_CPU, lcpu)
    _set(cont["limits"], p, nat.RES_MEMORY, lmem)


def _batch_pod(cont, p, bcpu, bmem):
    for rl in (cont["requests"], cont["limits"]):
        _set(rl, p, nat.RES_BATCH_CPU, bcpu)
        _set(rl, p, nat.RES_BATCH_MEMORY, bmem)


def _node(nodes, i, a, bases, requested=(0, 0)):
    """Node i: cap a (one value or one per resource cpu, memory, batch-cpu, batch-memory) and the six slot bases."""
    caps = (a,) * 4 if np.isscalar(a) or isinstance(a, int) else a
    for r, v in zip((nat.RES_CPU, nat.RES_MEMORY, nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY), caps):
        _set(nodes["allocatable"], i, r, v)
    nodes["nonzero_requested"][i] = bases[0], bases[1]
    _set(nodes["requested"], i, nat.RES_CPU, requested[0])
    _set(nodes["requested"], i, nat.RES_MEMORY, requested[1])
    _set(nodes["requested"], i, nat.RES_BATCH_CPU, bases[2])
    _set(nodes["requested"], i, nat.RES_BATCH_MEMORY, bases[3])
    _set(nodes["node_usage"], i, nat.RES_CPU, bases[4])
    _set(nodes["node_usage"], i, nat.RES_MEMORY, bases[5])


class EdgeCluster:
    """view: the SynthView; pods / nodes by role (index arrays); pair_of_node[i] for the aligned nodes."""


@functools.lru_cache(maxsize=None)
def edge_cluster(most_allocated=False, negative=False, wide=False):
    n_filter, n_big = 4, 2 * C
    n_neg = len(NEG_TUPLES) + 10 * C if negative else 0
    N = N_ALIGNED + n_filter + n_big + n_neg
    n_special = 3
    n_negpods = 2 * len(NEG_TUPLES) + 2 if negative else 0
    n_wide = len(WIDE_RES) + 4 if wide else 0
    P = N_PAIR_PODS + n_special + n_negpods + n_wide
    assert P <= 160
    sk = synth.make_cluster(N, P, seed=4141, decorated=False)
    pods, cont, nodes = sk.pods, sk.containers, sk.nodes
    for rl in (cont["requests"], cont["limits"], nodes["allocatable"], nodes["requested"], nodes["node_usage"]):
        rl["v"][:] = 0
        rl["present"][:] = 0
    nodes["nonzero_requested"][:] = 0
    rng = np.random.default_rng(99)
    nodes["pod_count"] = rng.integers(0, 60, N)
    nodes["allowed_pods"] = 110
    # every node reports a fresh NodeMetric; its own usage thresholds are 0 (= not checked: LoadAware's filter passes)
    for f in ("has_node_metric", "has_update_time", "has_report_interval", "has_node_metric_info"):
        nodes[f] = 1
    nodes["update_time_ns"] = sk.now_ns - 30 * 10**9
    nodes["custom_thresholds_state"] = 1
    nodes["custom_usage_thresholds"]["present"][:] = 0x3

    ec = EdgeCluster()
    # pod pairs
    for j in range(J):
        q = pair_requests(j)
        for d in (0, 1):
            _ls_pod(cont, 4 * j + d, q[0] + d, q[1] + d, q[4] + d, q[5] + d)
            _batch_pod(cont, 4 * j + 2 + d, q[2] + d, q[3] + d)
    ec.pair_pods = np.arange(N_PAIR_PODS)
    # aligned nodes
    for i in range(N_ALIGNED):
        a, q = CAPS[i % C], pair_requests(i % J)
        _node(nodes, i, a, [step_base(a, slot_k(i, s), q[s], most_allocated and s < 4) for s in range(SLOTS)])
    ec.aligned = np.arange(N_ALIGNED)
    ec.pair_of_node = ec.aligned % J
    # FILTER nodes: free == request and free == request − 1 of memory and batch-memory, two magnitudes
    p0 = N_PAIR_PODS
    _ls_pod(cont, p0, 1000, FILTER_REQ[0], 1000, FILTER_REQ[0])
    _batch_pod(cont, p0 + 1, 1000, FILTER_REQ[0])
    _ls_pod(cont, p0 + 2, 1000, FILTER_REQ[1], 1000, FILTER_REQ[1])
    ec.filter_pods = np.arange(p0, p0 + 3)
    n0 = N_ALIGNED
    for x, (req, alloc) in enumerate(((FILTER_REQ[0], 1 << 38), (FILTER_REQ[1], 1 << 51))):
        for d in (0, 1):   # free = request − d
            used = alloc - req + d
            _node(nodes, n0 + 2 * x + d, (64_000, alloc, 64_000, alloc), (63_000, used, 0, used, 63_000, alloc - 5), (0, used))
    ec.filter_nodes = np.arange(n0, n0 + n_filter)
    # BIG nodes: bases up to 2^50 − 1, above the cap on every slot
    n0 += n_filter
    for x in range(n_big):
        a = CAPS[x % C]
        top = VAL_LIMIT - 1 - (x // 2) * 977 if x % 3 else a + 1 + x
        _node(nodes, n0 + x, a, (top, top - 1, top - 2, top - 3, top - 4, top - 5))
    ec.big_nodes = np.arange(n0, n0 + n_big)
    n0 += n_big
    p0 += n_special
    ec.neg_pods = ec.neg_nodes = np.zeros(0, np.int64)
    if negative:
        # pods: per recorded tuple one whose Fit requests and one whose LoadAware estimates (the limits) are the
        # tuple's pr (the other two slots one request away); then an adjacent pair at NEG_X
        for t, (_, _, pr) in enumerate(NEG_TUPLES):
            _ls_pod(cont, p0 + 2 * t, pr, pr, pr + 1, pr + 1)
            _ls_pod(cont, p0 + 2 * t + 1, pr - 1, pr - 1, pr, pr)
            for d in (0, 1):
                for rl in (cont["requests"], cont["limits"]):
                    _set(rl, p0 + 2 * t + d, NEG_GATE[t], 1)
        ps = p0 + 2 * len(NEG_TUPLES)
        for d in (0, 1):
            _ls_pod(cont, ps + d, NEG_X + d, NEG_X + d, NEG_X + 7 + d, NEG_X + 7 + d)
        ec.neg_pods = np.arange(p0, ps + 2)
        ec.neg_sweep_pods = np.arange(ps, ps + 2)
        for t, (a, base, _) in enumerate(NEG_TUPLES):
            _node(nodes, n0 + t, a, (base, base, 0, 0, base, base), (base, base))
            _set(nodes["allocatable"], n0 + t, NEG_GATE[t], 10)
        # sweep nodes: on the step of k for the NEG_X pair (slots 0, 1, 4, 5); no pod of theirs scores batch resources
        for x in range(10 * C):
            a, i = CAPS[x % C], n0 + len(NEG_TUPLES) + x
            b = [0 if s in (2, 3) else step_base(a, slot_k(7 * x, s), 0, most_allocated and s < 4) - NEG_X - (7 if s > 3 else 0)
                 for s in range(SLOTS)]
            _node(nodes, i, a, b, (b[0], b[1]))
        ec.neg_nodes = np.arange(n0, n0 + n_neg)
        p0 = ps + 2
    ec.wide_pods = np.zeros(0, np.int64)
    if wide:
        # eight more resources on every node; pod p0 + x is a copy of a pair pod that also requests one of resource x,
        # the last four named slots twice: the 8-slot map then keeps those (and the batch resources), and the pods of
        # ephemeral-storage, mid-cpu, mid-memory and the first named slot are the spill pods — all of them resources
        # the generic pair path scores with the fast formula
        for x, r in enumerate(WIDE_RES + WIDE_RES[4:]):
            _set(nodes["allocatable"], np.arange(N), r, 10)
            src = 4 * ((3 * x) % J) + (x & 1)
            cont[p0 + x] = cont[src]
            for rl in (cont["requests"], cont["limits"]):
                _set(rl, p0 + x, r, 1)
        ec.wide_pods = np.arange(p0, p0 + n_wide)
    ec.view = synth.SynthView(pods, cont, nodes, sk.now_ns)
    ec.n_pods, ec.n_nodes = P, N
    for a in (pods, cont, nodes):
        a.flags.writeable = False
    return ec


# ---- configs -------------------------------------------------------------------------------------------------------
LA_ODD = {"cpu": 2, "memory": 1}             # a LoadAware weight sum that is no power of two: the batch leaves the class path
MOST_W = dict(fit_strategy="MostAllocated", fit_resources={"cpu": 2, "memory": 1, BATCH_CPU: 3})
CONFIGS = {
    # class path (k_eval3 / k_eval3_dup)
    "shipped": lambda **kw: shipped_profile(**kw),
    "most4": lambda **kw: shipped_profile(fit_strategy="MostAllocated", **kw),
    "w3_5": lambda **kw: shipped_profile(weight_fit=3, weight_loadaware=5, **kw),
    "big_20000": lambda **kw: shipped_profile(weight_fit=20_000, weight_loadaware=20_000, **kw),
    "big_39999": lambda **kw: shipped_profile(weight_fit=39_999, weight_loadaware=1, **kw),
    # slot kernels (k_eval2)
    "slot_pow2": lambda **kw: shipped_profile(resource_weights=LA_ODD, **kw),
    "slot_fit6": lambda **kw: make_config(fit_resources={"cpu": 2, "memory": 1, BATCH_CPU: 3}, resource_weights=LA_ODD, **kw),
    "slot_fit599": lambda **kw: make_config(fit_resources={"cpu": 298, "memory": 300, BATCH_CPU: 1},
                                            resource_weights=LA_ODD, **kw),
    "slot_fit600": lambda **kw: make_config(fit_resources={"cpu": 299, "memory": 300, BATCH_CPU: 1},
                                            resource_weights=LA_ODD, **kw),
    "slot_la599": lambda **kw: shipped_profile(resource_weights={"cpu": 300, "memory": 299}, **kw),
    # (cpu / memory pods weigh 2 + 1 = 3: no power of two, so this batch takes the slot kernels under any LoadAware weights)
    "most_w": lambda **kw: make_config(**MOST_W, **kw),
    "slot_most": lambda **kw: make_config(**MOST_W, resource_weights=LA_ODD, **kw),
    "slot_big_20000": lambda **kw: shipped_profile(weight_fit=20_000, weight_loadaware=20_000, resource_weights=LA_ODD, **kw),
    "slot_big_39999": lambda **kw: shipped_profile(weight_fit=39_999, weight_loadaware=1, resource_weights=LA_ODD, **kw),
}
BIG_CONFIGS = ("big_20000", "big_39999", "slot_big_20000", "slot_big_39999")


def is_most(name):
    return name in ("most_w", "most4", "slot_most")


def config(name, **kw):
    return CONFIGS[name](**kw)


class Ref:
    pass


def restricted(ref, elig_class, masks):
    """`ref` with the pods' eligibility classes applied (elig_class [P]: 0 none, k: row k − 1 of masks [K][N])."""
    r = Ref()
    r.ec, r.cfg, r.idx, r.fit, r.la = ref.ec, ref.cfg, ref.idx, ref.fit, ref.la
    ok = np.ones_like(ref.mask)
    for p, k in enumerate(elig_class):
        if k:
            ok[p] = masks[k - 1]
    r.mask = ref.mask & ok
    total = int(r.cfg["weight_fit"]) * r.fit.astype(np.int64) + int(r.cfg["weight_loadaware"]) * r.la.astype(np.int64)
    r.total = np.where(r.mask, total, -1)
    return r


@functools.lru_cache(maxsize=None)
def reference(name, negative=False, wide=False, pods=None):
    """The oracle's answer for config `name` on its edge cluster over `pods` (a tuple; default every pod), read-only:
    mask, fit, la [P][N], total (−1 where infeasible), and the top-1 node / total per pod."""
    ec = edge_cluster(is_most(name), negative, wide)
    cfg = config(name, extended_resources=EXT_NAMES) if wide else config(name)
    idx = np.arange(ec.n_pods) if pods is None else np.asarray(pods)
    r = Ref()
    r.ec, r.cfg, r.idx = ec, cfg, idx
    r.mask, r.fit, r.la = oracle.eval_matrix(cfg, ec.view, idx, ec.view.now_ns)
    total = int(cfg["weight_fit"]) * r.fit.astype(np.int64) + int(cfg["weight_loadaware"]) * r.la.astype(np.int64)
    r.total = np.where(r.mask, total, -1)
    r.best_total = r.total.max(axis=1)
    r.best_node = np.where(r.best_total >= 0, r.total.argmax(axis=1), -1)   # the lowest index among ties
    for a in (r.mask, r.fit, r.la, r.total, r.best_total, r.best_node):
        a.flags.writeable = False
    return r


def check_eval(ref, res, n_nodes=None, col0=0, feasible_only=False):
    """Mask, both score planes and top-1 of an Engine.eval result against the reference (columns [col0, col0 + n)).
    feasible_only: scores are compared where the pair is feasible (the negative variant, see the module docstring)."""
    n = ref.ec.n_nodes - col0 if n_nodes is None else n_nodes
    sl = slice(col0, col0 + n)
    if "mask" in res:
        np.testing.assert_array_equal(engine.unpack_mask(res["mask"], n), ref.mask[:, sl])
    if "scores" in res:
        keep = ref.mask[:, sl] if feasible_only else np.ones_like(ref.mask[:, sl])
        np.testing.assert_array_equal(np.where(keep, res["scores"][:, :n, 0], 0), np.where(keep, ref.fit[:, sl], 0))
        np.testing.assert_array_equal(np.where(keep, res["scores"][:, :n, 1], 0), np.where(keep, ref.la[:, sl], 0))
    if "top1" in res:
        tot = ref.total[:, sl]
        best = tot.max(axis=1)
        node, got = engine.decode_top1(res["top1"])
        np.testing.assert_array_equal(got, best)
        np.testing.assert_array_equal(node, np.where(best >= 0, tot.argmax(axis=1) + col0, -1))
