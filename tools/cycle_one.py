#!/usr/bin/env python
"""The per-pod scheduling cycle, measured both ways in one process (config 2, shipped profile):

  A  the three-call path exactly as bench.py's dropin_cycle drives it — kg_pods_set (P = 1), kg_eval into pinned
     host memory, selectHost, kg_commit;
  B  kg_cycle_one (select + Reserve in one launch, one synchronisation).

Each with the pod's planes in pinned host memory and top-1 only, C cycles from one snapshot per run, the runs
interleaved A/B/A/B/A/B.  Both must place every pod where kg_place places it on the same snapshot (asserted).
Acceptance: the slowest fused top-1 run is faster than the fastest three-call top-1 run.  Prints one JSON line
(--out: also written there).  For the kernel time, run it under `rocprofv3 --kernel-trace --stats` (no counters)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GOAL_US = 50.0   # the per-cycle goal of the drop-in loop


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=10_000, help="pods of the config-2 queue (the first --cycles are scheduled)")
    ap.add_argument("--cycles", type=int, default=1_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    cfg = shipped_profile()
    cl = synth.make_cluster(args.nodes, args.pods, seed=2)
    node_rows = engine.build_node_rows(cfg, cl)
    pod_rows = engine.build_pod_rows(cfg, cl, np.arange(args.pods))
    now, C, N = cl.now_ns, min(args.cycles, args.pods), args.nodes
    one = [np.ascontiguousarray(pod_rows[p:p + 1]) for p in range(C)]

    eng = engine.Engine(cfg)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.set_stream(stream)
    eng.set_stream(stream.cuda_stream)
    W = (N + 63) // 64
    mask = torch.empty((1, W), dtype=torch.int64, pin_memory=True)
    scores = torch.empty((1, W * 64, 2), dtype=torch.uint8, pin_memory=True)
    top1 = torch.zeros(1, dtype=torch.int64, pin_memory=True)
    top_np = top1.numpy().view(np.uint64)

    eng.load_snapshot(node_rows)
    eng.set_pods(pod_rows[:C])
    ref_nodes, _ = eng.place(now)

    def three_call(planes: bool, n: int, out=None) -> float:
        t0 = time.perf_counter()
        for p in range(n):
            eng.set_pods(one[p])
            eng.eval_host(now, mask.data_ptr() if planes else 0, scores.data_ptr() if planes else 0, top1.data_ptr())
            node = -1 if top_np[0] == 0 else int(0xFFFFFFFF - (int(top_np[0]) & 0xFFFFFFFF))
            if node >= 0:
                eng.commit(0, node)
            if out is not None:
                out.append(node)
        return time.perf_counter() - t0

    def fused(planes: bool, n: int, out=None) -> float:
        mp, sp = (mask.data_ptr(), scores.data_ptr()) if planes else (0, 0)
        t0 = time.perf_counter()
        for p in range(n):
            r = eng.cycle_one_host(one[p], now, True, mp, sp)
            if out is not None:
                out.append(r.node)
        return time.perf_counter() - t0

    for f in (three_call, fused):   # warm-up (first-use allocations)
        eng.load_snapshot(node_rows)
        f(True, 8)
    runs = {"three_call": {"planes": [], "top1": []}, "fused": {"planes": [], "top1": []}}
    same = True
    for _ in range(args.reps):
        for name, f in (("three_call", three_call), ("fused", fused)):
            for kind in ("planes", "top1"):
                eng.load_snapshot(node_rows)
                got = []
                dt = f(kind == "planes", C, got)
                runs[name][kind].append(round(dt / C * 1e6, 2))
                same = same and np.array_equal(np.asarray(got), ref_nodes[:C])
    eng.close()
    assert same, "the per-pod paths and kg_place disagree on a placement"

    def summary(v):
        return {"median_us": float(np.median(v)), "runs_us": v}

    slowest_fused, fastest_three = max(runs["fused"]["top1"]), min(runs["three_call"]["top1"])
    res = {"tool": "cycle_one", "workload": f"config2: {C} cycles of one pod over {N} nodes, shipped profile",
           "cycles": C, "nodes": N, "matches_kg_place": bool(same),
           "three_call": {k: summary(v) for k, v in runs["three_call"].items()},
           "fused": {k: summary(v) for k, v in runs["fused"].items()},
           "accepted": bool(slowest_fused < fastest_three),
           "speedup_top1": round(float(np.median(runs["three_call"]["top1"]) / np.median(runs["fused"]["top1"])), 2),
           "goal_us": GOAL_US, "goal_met": bool(np.median(runs["fused"]["top1"]) <= GOAL_US)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
