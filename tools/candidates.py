#!/usr/bin/env python
"""kg_candidates against planes mode for a profile with Score plugins outside the engine, measured in one process
(config 2, shipped profile: Fit + LoadAware; 256 pods x 100k nodes by default), for k = 16 and k = 64:

  A  Engine.candidates: the k best feasible nodes of every pod with their plugin scores, in one call;
  B  what the caller did before: kg_pods_set + kg_eval with the mask and score planes into pinned host memory, then
     a NumPy top-k over the P x N pairs (totals from the score pairs, the mask applied, np.argpartition on the
     64-bit keys, the k survivors sorted).

Every call ends in a stream synchronisation, so a host clock around a call times it; both ways are warmed first and the
runs are interleaved A16 / A64 / B16 / B64 per repetition; the figures are medians.  A and B are checked against each
other (same keys, same scores, n_feasible = the mask's popcount) before anything is timed.
Prints one JSON line (--out: also written there); exit status 1 when the two ways disagree.  For the kernel time of
k_cand / k_cand_merge, run it under `rocprofv3 --kernel-trace --stats` (no counters)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planes_topk(cfg, mask_words: np.ndarray, scores: np.ndarray, n_nodes: int, k: int):
    """(keys [P][k] u64, scores [P][k][4] u8, n_feasible [P]) from kg_eval's host planes: the host pass of way B."""
    P = len(mask_words)
    feas = np.unpackbits(mask_words.view(np.uint8), axis=1, bitorder="little")[:, :n_nodes].astype(bool)
    pair = scores[:, :n_nodes]
    tot = int(cfg["weight_fit"]) * pair[..., 0].astype(np.uint64) + int(cfg["weight_loadaware"]) * pair[..., 1].astype(np.uint64)
    keys = ((tot + np.uint64(1)) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n_nodes, dtype=np.uint64))[None, :]
    keys[~feas] = 0
    kk = min(k, n_nodes)
    idx = np.argpartition(keys, n_nodes - kk, axis=1)[:, n_nodes - kk:]
    rows = np.arange(P)[:, None]
    order = np.argsort(keys[rows, idx], axis=1)[:, ::-1]
    idx = idx[rows, order]
    out_k = np.zeros((P, k), dtype=np.uint64)
    out_s = np.zeros((P, k, 4), dtype=np.uint8)
    out_k[:, :kk] = keys[rows, idx]
    out_s[:, :kk, :2] = np.where((out_k[:, :kk] != 0)[..., None], pair[rows, idx], 0)
    return out_k, out_s, feas.sum(axis=1).astype(np.uint32)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    cfg = shipped_profile()
    N, P = args.nodes, args.pods
    cl = synth.make_cluster(N, P, seed=2)
    node_rows = engine.build_node_rows(cfg, cl)
    pod_rows = engine.build_pod_rows(cfg, cl, np.arange(P))
    now = cl.now_ns

    eng = engine.Engine(cfg)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.set_stream(stream)
    eng.set_stream(stream.cuda_stream)
    eng.load_snapshot(node_rows)
    W = (N + 63) // 64
    mask = torch.zeros((P, W), dtype=torch.int64, pin_memory=True)
    scores = torch.zeros((P, W * 64, 2), dtype=torch.uint8, pin_memory=True)
    mask_np, scores_np = mask.numpy().view(np.uint64), scores.numpy()

    def way_a(k: int):
        t0 = time.perf_counter()
        res = eng.candidates(pod_rows, now, k)
        return time.perf_counter() - t0, res

    def way_b(k: int):
        t0 = time.perf_counter()
        eng.set_pods(pod_rows)
        eng.eval_host(now, mask.data_ptr(), scores.data_ptr())
        t1 = time.perf_counter()
        res = planes_topk(cfg, mask_np, scores_np, N, k)
        return time.perf_counter() - t0, t1 - t0, res

    agree = True
    for k in (16, 64):   # agreement and warm-up (first-use allocations)
        _, a = way_a(k)
        _, _, (bk, bs, bn) = way_b(k)
        agree = agree and np.array_equal(a["keys"], bk) and np.array_equal(a["scores"], bs) and \
            np.array_equal(a["n_feasible"], bn)
    runs = {"A16": [], "A64": [], "B16": [], "B64": [], "B16_eval": [], "B64_eval": []}
    for _ in range(args.reps):
        for k in (16, 64):
            runs[f"A{k}"].append(round(way_a(k)[0] * 1e3, 3))
        for k in (16, 64):
            t, t_eval, _ = way_b(k)
            runs[f"B{k}"].append(round(t * 1e3, 3))
            runs[f"B{k}_eval"].append(round(t_eval * 1e3, 3))
    eng.close()

    med = {k: float(np.median(v)) for k, v in runs.items()}
    words = (N + 63) // 64
    res = {"tool": "candidates", "workload": f"config2: {P} pods x {N} nodes, shipped profile (Fit + LoadAware)",
           "nodes": N, "pods": P, "reps": args.reps, "agree": bool(agree), "runs_ms": runs, "median_ms": med,
           "ratio_B_over_A": {"k16": round(med["B16"] / med["A16"], 2), "k64": round(med["B64"] / med["A64"], 2)},
           "ratio_B_eval_over_A": {"k16": round(med["B16_eval"] / med["A16"], 2), "k64": round(med["B64_eval"] / med["A64"], 2)},
           "bytes_to_host": {"A16": P * (16 * 12 + 4), "A64": P * (64 * 12 + 4), "B": P * (words * 8 + words * 128)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
