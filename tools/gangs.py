#!/usr/bin/env python
"""Gang-aware placement (kg_place_gangs) on a synthetic colocation burst (config 2, shipped profile).

Default: a small scenario — the batch is cut into strict gangs of --gang consecutive pods (each its own group), every
--fail-every-th gang gets one member that fits nowhere (a cpu request no node holds) in its middle.  Prints the
verdict counts, the pods rolled back (the members queued before the injected one in each rejected gang: they were
reserved, then unreserved on the device before the next pod's cycle) and the pods skipped behind it, and places the
same batch without gangs through kg_place for comparison: how many pods hold a node either way and how many pods
land on a different node because the rejected gangs handed their capacity back.

--time: median of --reps runs of place_gangs on an all-success gang batch (no injected member) against place of the
same batch, each from the same reloaded snapshot.

Prints one JSON line (--out: also written there)."""
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
    ap.add_argument("--nodes", type=int, default=2_100)
    ap.add_argument("--pods", type=int, default=256)
    ap.add_argument("--gang", type=int, default=16, help="pods per gang")
    ap.add_argument("--fail-every", type=int, default=4, help="every n-th gang gets a member that fits nowhere")
    ap.add_argument("--place-chunk", type=int, default=0, help="kg_config.place_chunk (0: the profile's)")
    ap.add_argument("--time", action="store_true", help="time place_gangs against place on an all-success batch")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from koordinator_amd import _native as nat
    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    cfg = shipped_profile(place_chunk=args.place_chunk) if args.place_chunk else shipped_profile()
    cl = synth.make_cluster(args.nodes, args.pods, seed=2)
    node_rows = engine.build_node_rows(cfg, cl)
    pod_rows = engine.build_pod_rows(cfg, cl, np.arange(args.pods))
    now = cl.now_ns
    P, G = args.pods, max(1, args.gang)
    n_gangs = (P + G - 1) // G
    pod_gang = (np.arange(P) // G).astype(np.int32)
    gang_min = np.bincount(pod_gang, minlength=n_gangs).astype(np.int32)
    gang_flags = np.full(n_gangs, nat.GANG_STRICT, np.uint8)
    injected = {}
    if not args.time and args.fail_every > 0:
        for g in range(args.fail_every - 1, n_gangs, args.fail_every):
            p = g * G + int(gang_min[g]) // 2
            pod_rows["request"][p, nat.RES_CPU] = pod_rows["fit_score_request"][p, nat.RES_CPU] = 1 << 40
            injected[g] = p
    all_nodes = np.arange(args.nodes, dtype=np.int32)
    res = {"tool": "gangs", "nodes": args.nodes, "pods": P, "gang": G, "n_gangs": n_gangs,
           "place_chunk": int(cfg["place_chunk"])}

    with engine.Engine(cfg) as eng:
        eng.load_snapshot(node_rows)
        eng.set_pods(pod_rows)
        if args.time:
            t_gang, t_plain = [], []
            verdicts = None
            for rep in range(args.reps + 1):   # (rep 0: first-use allocations, not kept)
                eng.upsert(all_nodes, node_rows)
                t0 = time.perf_counter()
                g_nodes, _, verdicts = eng.place_gangs(now, pod_gang, gang_min, gang_flags)
                t1 = time.perf_counter()
                eng.upsert(all_nodes, node_rows)
                t2 = time.perf_counter()
                p_nodes, _ = eng.place(now)
                t3 = time.perf_counter()
                if rep:
                    t_gang.append(t1 - t0)
                    t_plain.append(t3 - t2)
            mg, mp = float(np.median(t_gang)), float(np.median(t_plain))
            res.update(mode="time", reps=args.reps, all_allowed=bool((verdicts == nat.GANG_ALLOWED).all()),
                       same_as_place=bool(np.array_equal(g_nodes, p_nodes)),
                       place_gangs={"median_ms": round(mg * 1e3, 3), "pods_per_s": round(P / mg, 1),
                                    "runs_ms": [round(x * 1e3, 3) for x in t_gang]},
                       place={"median_ms": round(mp * 1e3, 3), "pods_per_s": round(P / mp, 1),
                              "runs_ms": [round(x * 1e3, 3) for x in t_plain]},
                       ratio=round(mg / mp, 3))
        else:
            g_nodes, _, verdicts = eng.place_gangs(now, pod_gang, gang_min, gang_flags)
            eng.upsert(all_nodes, node_rows)
            p_nodes, _ = eng.place(now)
            rejected = np.flatnonzero(verdicts == nat.GANG_REJECTED).tolist()
            rolled = sum(injected[g] - g * G for g in rejected if g in injected)
            skipped = sum(min((g + 1) * G, P) - 1 - injected[g] for g in rejected if g in injected)
            res.update(mode="scenario",
                       verdicts={"allowed": int((verdicts == nat.GANG_ALLOWED).sum()),
                                 "waiting": int((verdicts == nat.GANG_WAITING).sum()), "rejected": len(rejected)},
                       injected_gangs=len(injected), rejected_without_injection=len([g for g in rejected if g not in injected]),
                       rolled_back_pods=int(rolled), skipped_pods=int(skipped),
                       placed={"place_gangs": int((g_nodes >= 0).sum()), "place": int((p_nodes >= 0).sum())},
                       partial_gangs_left_by_place=int(sum(1 for g in range(n_gangs)
                                                           if 0 < (p_nodes[pod_gang == g] >= 0).sum() < gang_min[g])),
                       pods_on_another_node=int(((g_nodes >= 0) & (p_nodes >= 0) & (g_nodes != p_nodes)).sum()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
