"""Clusters, profiles and references shared by the kg_cycle_one tests (tests/test_cycle_one_*.py).

TEST INFRASTRUCTURE: the references are computed once per process and handed out read-only.
"""
import functools

import numpy as np

from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile

N_NODES, N_PODS = 1_100, 96            # 4 full 256-node blocks and a ragged one of 76
BIG = np.arange(3, N_NODES, 97)        # nodes beyond the fp64 bounds: the exact pair path
LA_W = {"cpu": 1, "memory": 1, "ephemeral-storage": 1, "example.com/gpu": 2, "kubernetes.io/batch-cpu": 1}
LA_SF = {"ephemeral-storage": 60, "example.com/gpu": 100}
PROFILES = ("default", "shipped", "most", "la_extra")


def config(profile):
    return {"default": make_config, "shipped": shipped_profile,
            "most": lambda: make_config(fit_strategy="MostAllocated",
                                        fit_resources={"cpu": 2, "memory": 1, "kubernetes.io/batch-cpu": 3}),
            "la_extra": lambda: shipped_profile(resource_weights=LA_W, estimated_scaling_factors=LA_SF)}[profile]()


@functools.lru_cache(maxsize=None)
def cluster(la_extra=False):
    """synth.make_cluster(1_100, 96, seed=31) with the nodes BIG raised beyond the fp64 bounds (la_extra: the
    cluster whose LoadAware inputs carry the extra resources)."""
    make = synth.make_la_extra_cluster if la_extra else synth.make_cluster
    cl = make(N_NODES, N_PODS, seed=31)
    cl.nodes["allocatable"]["v"][BIG, 1] = (1 << 43) + 99
    return cl.with_nodes(cl.nodes)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(profile):
    """(cfg, cluster, node rows, pod rows) of a profile on the shared cluster; the rows are read-only."""
    cfg = config(profile)
    cl = cluster(profile == "la_extra")
    rows, pods = _frozen(engine.build_node_rows(cfg, cl), engine.build_pod_rows(cfg, cl, np.arange(N_PODS)))
    return cfg, cl, rows, pods


@functools.lru_cache(maxsize=None)
def oracle_matrix(profile):
    """(mask, fit, la, total with −1 where infeasible) of the oracle for the profile's 96 pods."""
    from oracle import oracle
    cfg, cl, _, _ = case(profile)
    m, f, l = oracle.eval_matrix(cfg, cl, np.arange(N_PODS), cl.now_ns)
    tot = np.where(m, int(cfg["weight_fit"]) * f.astype(np.int64) + int(cfg["weight_loadaware"]) * l.astype(np.int64), -1)
    return _frozen(m, f, l, tot)


def key_of(total_row):
    """The top-1 key of one pod from its totals (−1 where infeasible): lowest index among the best."""
    j = int(np.argmax(total_row))
    return 0 if total_row[j] < 0 else ((int(total_row[j]) + 1) << 32) | (0xFFFFFFFF - j)


def rows_totals(cfg, rows, pod_row, now_ns):
    """(mask, fit, la, totals with −1 where infeasible) of one pod from engine rows (tests/rows_ref.rows_eval)."""
    from rows_ref import rows_eval
    m, f, l = rows_eval(cfg, rows, np.asarray(pod_row).reshape(1), now_ns)
    tot = np.where(m[0], int(cfg["weight_fit"]) * f[0] + int(cfg["weight_loadaware"]) * l[0], -1)
    return m[0], f[0], l[0], tot


def check_planes(res, n, mask, fit, la):
    np.testing.assert_array_equal(engine.unpack_mask(res["mask"], n)[0], mask)
    np.testing.assert_array_equal(res["scores"][0, :n, 0], fit)
    np.testing.assert_array_equal(res["scores"][0, :n, 1], la)
    assert not res["numa_scores"].any()   # NodeNUMAResource is off in these profiles


def shipped_planes_keys(n_nodes=None):
    """The shipped case through cycle_one(commit=False, planes=True) on the first n_nodes nodes: the keys and the
    planes of every pod (the bounds build runs this in a child process)."""
    cfg, cl, rows, pods = case("shipped")
    rows = rows if n_nodes is None else rows[:n_nodes]
    keys, masks, scores = [], [], []
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(rows)
        for p in pods[:N_PODS if n_nodes is None else 8]:
            r = eng.cycle_one(p, cl.now_ns, commit=False, planes=True)
            keys.append(r["key"])
            masks.append(engine.unpack_mask(r["mask"], len(rows))[0])
            scores.append(r["scores"][0, :len(rows)].copy())
    return keys, np.array(masks), np.array(scores)
