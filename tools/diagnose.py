#!/usr/bin/env python
"""kg_diagnose against the cycle it explains, measured in one process (config 2, shipped profile: Fit + LoadAware):

  A  Engine.diagnose, counts only, for n = 1, 16 and 256 pods;
  B  n = 1 with the reason plane into pinned host memory;
  C  the three-call cycle of one pod exactly as tools/cycle_one.py path A drives it (top-1 only): kg_pods_set (P = 1),
     kg_eval into pinned host memory, selectHost, kg_commit.

Every call ends in a stream synchronisation, so a host clock around a loop of calls times them; each shape is warmed
first and the runs are interleaved A1/A16/A256/B/C per repetition.  A is checked against the counts of matrix mode (the
feasible slot equals the mask's popcount).
Acceptance: the slowest run of A (n = 1) is faster than the fastest run of C — a diagnosis follows a failed cycle and
must not cost more than the cycle it explains.  Prints one JSON line (--out: also written there).  For the kernel time
of k_why / k_why_reduce, run it under `rocprofv3 --kernel-trace --stats` (no counters)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=1_000, help="pods of the config-2 queue the shapes draw from")
    ap.add_argument("--calls", type=int, default=200, help="calls per run of A (n = 1), B and C")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from koordinator_amd import _native as nat
    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    cfg = shipped_profile()
    cl = synth.make_cluster(args.nodes, args.pods, seed=2)
    node_rows = engine.build_node_rows(cfg, cl)
    pod_rows = engine.build_pod_rows(cfg, cl, np.arange(args.pods))
    now, N, C = cl.now_ns, args.nodes, min(args.calls, args.pods)
    one = [np.ascontiguousarray(pod_rows[p:p + 1]) for p in range(C)]

    eng = engine.Engine(cfg)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.set_stream(stream)
    eng.set_stream(stream.cuda_stream)
    W = (N + 63) // 64
    top1 = torch.zeros(1, dtype=torch.int64, pin_memory=True)
    top_np = top1.numpy().view(np.uint64)
    counts = torch.zeros((256, nat.WHY_SLOTS), dtype=torch.int32, pin_memory=True)
    pod_why = torch.zeros(256, dtype=torch.int32, pin_memory=True)
    why = torch.empty((1, W * 64), dtype=torch.int32, pin_memory=True)
    eng.load_snapshot(node_rows)

    # the counts against matrix mode, once
    eng.set_pods(pod_rows[:16])
    mask = engine.unpack_mask(eng.eval(now, scores=False, top1=False)["mask"], N)
    got = eng.diagnose(pod_rows[:16], now)
    assert np.array_equal(got["counts"][:, nat.WHY_SLOT_FEASIBLE], mask.sum(axis=1)), "counts disagree with matrix mode"

    def diag(n: int, calls: int, plane: bool = False) -> float:
        t0 = time.perf_counter()
        for k in range(calls):
            rows = one[k % C] if n == 1 else pod_rows[:n]
            eng.diagnose_host(rows, now, counts.data_ptr(), pod_why.data_ptr(), why.data_ptr() if plane else 0)
        return (time.perf_counter() - t0) / calls

    def three_call(calls: int) -> float:
        t0 = time.perf_counter()
        for p in range(calls):
            eng.set_pods(one[p])
            eng.eval_host(now, 0, 0, top1.data_ptr())
            node = -1 if top_np[0] == 0 else int(0xFFFFFFFF - (int(top_np[0]) & 0xFFFFFFFF))
            if node >= 0:
                eng.commit(0, node)
        return (time.perf_counter() - t0) / calls

    big_calls = max(4, C // 10)
    shapes = {"A1": lambda: diag(1, C), "A16": lambda: diag(16, big_calls), "A256": lambda: diag(256, big_calls),
              "B1_plane": lambda: diag(1, C, True), "C_three_call": lambda: three_call(C)}
    for f in (lambda: diag(1, 8), lambda: diag(16, 2), lambda: diag(256, 2), lambda: diag(1, 8, True),
              lambda: three_call(8)):   # warm-up (first-use allocations)
        f()
    runs = {k: [] for k in shapes}
    for _ in range(args.reps):
        for name, f in shapes.items():
            if name == "C_three_call":
                eng.load_snapshot(node_rows)   # every run of C commits from the same snapshot
            runs[name].append(round(f() * 1e6, 2))
    eng.close()

    slowest_a1, fastest_c = max(runs["A1"]), min(runs["C_three_call"])
    res = {"tool": "diagnose", "workload": f"config2: {N} nodes, shipped profile (Fit + LoadAware)", "nodes": N,
           "calls": C, "runs_us": runs, "median_us": {k: float(np.median(v)) for k, v in runs.items()},
           "slowest_A1_us": slowest_a1, "fastest_C_us": fastest_c, "accepted": bool(slowest_a1 < fastest_c),
           "plane_bytes": int(4 * W * 64)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if res["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
