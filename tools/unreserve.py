#!/usr/bin/env python
"""Rolling back k placements of a placed batch, measured both ways in one process (config 2, shipped profile):

  A  kg_unreserve: the k (pod, node) entries in one call;
  B  the Upsert path, which is all the engine offered before kg_unreserve: the host rebuilds the full row of every
     touched node (kg_build_node_rows of those nodes, timed as `build`) and pushes the true rows with
     kg_snapshot_upsert (timed as `upsert`).

Each from the same placed snapshot, --reps times, for k = 1, 64 and 1024 (--entries).  Both must leave identical
snapshots, equal to the host model (engine.row_unreserve on the placed rows): asserted on the whole download.  Also
times a single kg_commit, the yardstick a batch is expected to cost about one of.  Prints one JSON line (--out: also
written there)."""
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
    ap.add_argument("--pods", type=int, default=2_048, help="pods of the placed batch")
    ap.add_argument("--entries", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    cfg = shipped_profile()
    cl = synth.make_cluster(args.nodes, args.pods, seed=2)
    node_rows = engine.build_node_rows(cfg, cl)
    pod_rows = engine.build_pod_rows(cfg, cl, np.arange(args.pods))
    now = cl.now_ns

    eng = engine.Engine(cfg)
    eng.load_snapshot(node_rows)
    eng.set_pods(pod_rows)
    nodes, _ = eng.place(now)
    placed_rows = eng.download()
    placed = np.flatnonzero(nodes >= 0)

    def us(v):
        return {"median_us": round(float(np.median(v)) * 1e6, 1), "runs_us": [round(x * 1e6, 1) for x in v]}

    res = {"tool": "unreserve", "workload": f"config2: {len(placed)} of {args.pods} pods placed on {args.nodes} nodes, "
           "shipped profile", "nodes": args.nodes, "reps": args.reps, "entries": {}}
    same = True
    for k in args.entries:
        pick = placed[:: max(1, len(placed) // k)][:k]
        k = len(pick)
        touched = np.unique(nodes[pick]).astype(np.int32)
        want = placed_rows.copy()
        for i in pick:
            engine.row_unreserve(cfg, want[nodes[i]:nodes[i] + 1], pod_rows[i:i + 1])
        rel_pods, rel_nodes = np.ascontiguousarray(pod_rows[pick]), np.ascontiguousarray(nodes[pick])
        t_unr, t_build, t_ups = [], [], []
        for rep in range(args.reps + 1):   # (rep 0: first-use allocations, not kept)
            eng.upsert(touched, placed_rows[touched])
            t0 = time.perf_counter()
            rel = eng.unreserve(rel_pods, rel_nodes)
            dt = time.perf_counter() - t0
            assert rel.all()
            if rep == 0:
                same = same and eng.download().tobytes() == want.tobytes()
            else:
                same = same and eng.download(int(touched[0]), 1).tobytes() == want[touched[:1]].tobytes()
                t_unr.append(dt)
            eng.upsert(touched, placed_rows[touched])
            t0 = time.perf_counter()
            engine.build_node_rows(cfg, cl, touched)          # the host rebuild (from NodeInfo, NodeMetric, assign cache)
            t1 = time.perf_counter()
            eng.upsert(touched, want[touched])                # the true rows
            t2 = time.perf_counter()
            if rep == 0:
                same = same and eng.download().tobytes() == want.tobytes()
            else:
                t_build.append(t1 - t0)
                t_ups.append(t2 - t1)
        total = [a + b for a, b in zip(t_build, t_ups)]
        res["entries"][str(k)] = {"distinct_nodes": int(len(touched)), "kg_unreserve": us(t_unr),
                                  "upsert_path": {"build": us(t_build), "upsert": us(t_ups), "total": us(total)},
                                  "speedup": round(float(np.median(total) / np.median(t_unr)), 2)}
    # one kg_commit
    eng.upsert(np.arange(args.nodes, dtype=np.int32), node_rows)
    eng.set_pods(pod_rows[:1])
    t_commit = []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        eng.commit(0, int(nodes[placed[0]]))
        if rep:
            t_commit.append(time.perf_counter() - t0)
    eng.close()
    assert same, "kg_unreserve, the Upsert path and the host model disagree on the snapshot"
    res["kg_commit"] = us(t_commit)
    res["identical_snapshots"] = bool(same)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
