#!/usr/bin/env python
"""kg_preempt measured beside the diagnosis of the same pods, in one process (config 2, shipped profile: Fit +
LoadAware, with ElasticQuota's preemption over it):

  the config-2 cluster filled up - every node's requested cpu topped up until 2 to 20 cores are free, the state in
  which preemption runs - with a synthetic bound-pod table - about 30 pods per node whose requests add up to the
  node's `requested`, priorities from 4 classes, a tenth of them non-preemptible - and 64 preemptors of the highest
  class asking 24 cores and more, so they fit nowhere and every node is dry-run;

  P  Engine.preempt, picks only;  Q  with the status plane;  D  Engine.diagnose (counts only) for the same 64 pods.

--pdb adds the PDB form: 6 synthetic PodDisruptionBudgets (DisruptionsAllowed 0, 1, 0, 2, 1000, 1; a bound pod under
none, one or two of them), their thresholds from kg_pdb_thresholds loaded as the engine's plane, and the shapes
P_pdb / Q_pdb measured in the same interleaved repetitions (the plane is loaded and dropped outside the timed loops).
The result then carries `pdb_over_plain`: the ratio of the medians with the spread of the per-repetition ratios.

Every call ends in a stream synchronisation, so a host clock around a loop of calls times them; each shape is warmed
first and the runs are interleaved per repetition.  The picks are checked once against kg_row_preempt on the picked
nodes.  Prints one JSON line (--out: also written there).  For the kernel time of k_preempt / k_preempt_pick, run it
under `rocprofv3 --kernel-trace --stats` (no counters)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PRIOS = (0, 1_000, 5_000, 9_000)


def bound_table(node_rows, per_node: int, seed: int):
    """(first, rows, priority, start_ns): per node per_node - 6 .. per_node + 2 pods sharing its requested cpu / memory."""
    from koordinator_amd import _native as nat
    rng = np.random.default_rng(seed)
    N = len(node_rows)
    lengths = rng.integers(max(per_node - 6, 1), per_node + 3, N)
    first = np.zeros(N + 1, np.int32)
    first[1:] = np.cumsum(lengths)
    total = int(first[-1])
    node_of = np.repeat(np.arange(N), lengths)
    w = rng.random(total) + 0.2
    w /= np.add.reduceat(w, first[:-1])[node_of]
    rows = np.zeros(total, dtype=nat.POD_ROW)
    for r in (nat.RES_CPU, nat.RES_MEMORY):
        v = (np.maximum(node_rows["requested"][node_of, r], 0) * w).astype(np.int64)
        rows["request"][:, r] = rows["numa_request"][:, r] = v
        rows["nonzero_request"][:, r] = v
    rows["numa_request_present"] = 0b11
    rows["flags"] = nat.POD_HAS_REQUEST | nat.POD_VALID
    rows["flags"][rng.random(total) < 0.1] |= nat.POD_NON_PREEMPTIBLE
    rows["quota"] = -1
    prio = rng.choice(PRIOS[:3], total).astype(np.int32)
    start = (1_700_000_000 + rng.integers(0, 86_400, total)).astype(np.int64) * 10**9
    return first, rows, prio, start


PDB_ALLOWED = (0, 1, 0, 2, 1000, 1)


def pdb_thresholds(first, rows, prio, start, seed: int):
    """A synthetic PDB assignment (45 % of the pods under no PDB, 40 % under one, 15 % under two) folded into the
    per-pod thresholds, node by node."""
    from koordinator_amd import _native as nat
    from koordinator_amd import engine
    rng = np.random.default_rng(seed)
    total = len(rows)
    u = rng.random(total)
    k = np.where(u < 0.45, 0, np.where(u < 0.85, 1, 2))
    a = rng.integers(0, len(PDB_ALLOWED), total)
    b = (a + rng.integers(1, len(PDB_ALLOWED), total)) % len(PDB_ALLOWED)
    ids_first = np.zeros(total + 1, np.int32)
    ids_first[1:] = np.cumsum(k)
    ids = np.zeros(int(ids_first[-1]), np.int32)
    ids[ids_first[:-1][k >= 1]] = a[k >= 1]
    ids[ids_first[:-1][k == 2] + 1] = b[k == 2]
    non_pre = (rows["flags"] & nat.POD_NON_PREEMPTIBLE) != 0
    quota = np.ascontiguousarray(rows["quota"])
    allowed = np.array(PDB_ALLOWED, np.int32)
    out = np.full(total, nat.PDB_PRIO_NONE, np.int32)
    for j in range(len(first) - 1):
        lo, hi = int(first[j]), int(first[j + 1])
        if hi > lo:
            out[lo:hi] = engine.pdb_thresholds(prio[lo:hi], start[lo:hi], quota[lo:hi], non_pre[lo:hi],
                                               ids_first[lo:hi + 1] - ids_first[lo], ids[ids_first[lo]:ids_first[hi]], allowed)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--per-node", type=int, default=30, help="bound pods per node (about)")
    ap.add_argument("--preemptors", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10, help="calls per run")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pdb", action="store_true", help="also measure the PDB form (a threshold plane loaded)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from koordinator_amd import _native as nat
    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    cfg = shipped_profile()
    n_pre = min(args.preemptors, nat.PREEMPT_MAX_PODS)
    cl = synth.make_cluster(args.nodes, n_pre, seed=2)
    node_rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(n_pre))
    # a full cluster: 2 to 20 cores free per node; the preemptors ask more than that, within reach once pods leave
    rng = np.random.default_rng(1)
    node_rows["requested"][:, nat.RES_CPU] = np.maximum(node_rows["requested"][:, nat.RES_CPU],
                                                        node_rows["alloc"][:, nat.RES_CPU] - rng.integers(2_000, 20_001, len(node_rows)))
    node_rows["nonzero_requested"][:, 0] = np.maximum(node_rows["nonzero_requested"][:, 0], node_rows["requested"][:, nat.RES_CPU])
    cpu = 24_000 + 100 * np.arange(n_pre)
    pods["request"] = 0
    pods["numa_request"] = 0
    pods["request"][:, nat.RES_CPU] = pods["numa_request"][:, nat.RES_CPU] = cpu
    pods["request_present"], pods["numa_request_present"] = 0, 0b1
    pods["flags"] |= nat.POD_HAS_REQUEST
    prio = np.full(n_pre, PRIOS[3], np.int32)
    first, b_rows, b_prio, b_start = bound_table(node_rows, args.per_node, seed=3)
    max_per_node = int(np.diff(first).max())
    now, N = cl.now_ns, args.nodes

    eng = engine.Engine(cfg)
    eng.load_snapshot(node_rows)
    t0 = time.perf_counter()
    eng.set_bound_pods(first, b_rows, b_prio, b_start, max_per_node)
    set_s = time.perf_counter() - t0
    diag = eng.diagnose(pods, now)
    assert not diag["counts"][:, nat.WHY_SLOT_FEASIBLE].any(), "a preemptor fits somewhere"
    got = eng.preempt(pods, prio, now, plane=True)
    for i in range(0, n_pre, 7):   # the picks against the host routine on the picked nodes
        j = int(got["node"][i])
        assert j >= 0, "a preemptor without a candidate"
        lo, hi = int(first[j]), int(first[j + 1])
        one = engine.row_preempt(cfg, node_rows[j:j + 1], b_rows[lo:hi], b_prio[lo:hi], b_start[lo:hi], pods[i:i + 1],
                                 int(prio[i]), now)
        assert one["status"] == nat.PRE_CANDIDATE and (one["victims"] == got["victims"][i]).all()
        assert (one["n_victims"], one["hi_prio"], one["prio_sum"]) == (got["n_victims"][i], got["hi_prio"][i], got["prio_sum"][i])

    got_pdb = None
    if args.pdb:
        t0 = time.perf_counter()
        th = pdb_thresholds(first, b_rows, b_prio, b_start, seed=4)
        th_s = time.perf_counter() - t0
        eng.set_bound_pdb(first, th)
        got_pdb = eng.preempt(pods, prio, now, plane=True)
        for i in range(0, n_pre, 7):   # the picks against the host routine's PDB form on the picked nodes
            j = int(got_pdb["node"][i])
            assert j >= 0, "a preemptor without a candidate"
            lo, hi = int(first[j]), int(first[j + 1])
            one = engine.row_preempt_pdb(cfg, node_rows[j:j + 1], b_rows[lo:hi], b_prio[lo:hi], b_start[lo:hi], th[lo:hi],
                                         pods[i:i + 1], int(prio[i]), now)
            assert one["status"] == nat.PRE_CANDIDATE and (one["victims"] == got_pdb["victims"][i]).all()
            assert (one["n_victims"], one["n_violating"]) == (got_pdb["n_victims"][i], got_pdb["n_violating"][i])
        eng.set_bound_pdb(None, None)

    def run(f, calls):
        t = time.perf_counter()
        for _ in range(calls):
            f()
        return (time.perf_counter() - t) / calls

    shapes = {"P_pick": lambda: eng.preempt(pods, prio, now), "Q_plane": lambda: eng.preempt(pods, prio, now, plane=True),
              "D_diagnose": lambda: eng.diagnose(pods, now)}
    pdb_shapes = {"P_pdb": shapes["P_pick"], "Q_pdb": shapes["Q_plane"]} if args.pdb else {}
    for f in shapes.values():
        f()
    runs = {k: [] for k in list(shapes) + list(pdb_shapes)}
    for _ in range(args.reps):
        for name, f in shapes.items():
            runs[name].append(round(run(f, args.calls) * 1e3, 3))
        if args.pdb:   # the same calls with the plane loaded: the PDB instantiations of k_preempt
            eng.set_bound_pdb(first, th)
            for name, f in pdb_shapes.items():
                f()
                runs[name].append(round(run(f, args.calls) * 1e3, 3))
            eng.set_bound_pdb(None, None)
    eng.close()
    status = got["status"][:, :N]
    res = {"tool": "preempt", "workload": f"config2: {N} nodes, shipped profile, {int(first[-1])} bound pods "
                                          f"(max {max_per_node} per node), {n_pre} preemptors that fit nowhere",
           "nodes": N, "preemptors": n_pre, "bound_pods": int(first[-1]), "calls": args.calls, "runs_ms": runs,
           "median_ms": {k: float(np.median(v)) for k, v in runs.items()}, "bound_set_s": round(set_s, 3),
           "candidates_per_pod": float(got["n_candidates"].mean()), "victims_of_pick": float(got["n_victims"].mean()),
           "status_counts": {str(s): int((status == s).sum()) for s in range(5)},
           "pairs_per_s": float(n_pre * N / (np.median(runs["P_pick"]) * 1e-3))}
    if args.pdb:
        res["pdb"] = {"allowed": list(PDB_ALLOWED), "thresholds_s": round(th_s, 3),
                      "violating_pairs": int((got_pdb["n_violating_plane"][:, :N] > 0).sum()),
                      "picks_moved": int((got_pdb["node"] != got["node"]).sum())}
        res["pdb_over_plain"] = {}
        for plain, form in (("P_pick", "P_pdb"), ("Q_plane", "Q_pdb")):
            ratios = np.array(runs[form]) / np.array(runs[plain])
            res["pdb_over_plain"][form] = {"ratio_of_medians": round(float(np.median(runs[form]) / np.median(runs[plain])), 3),
                                           "per_rep_min": round(float(ratios.min()), 3), "per_rep_max": round(float(ratios.max()), 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
