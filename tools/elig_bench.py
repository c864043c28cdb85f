"""k_eval_elig against k_eval_spill on one matrix pass (kg_set_profiling / kg_eval_kernel_times intervals).

Batch: --pods (1000) x --nodes (100000) under the shipped Fit + LoadAware profile, every fourth pod restricted to one
eligibility class.  Three classes, one run each:
  random50   a random 50 % of the nodes
  random5    a random 5 % (every 64-node segment still holds an eligible node: nothing is skipped)
  pool5      a contiguous 5 % (whole tiles: the others are skipped by their tile count)
Baseline: the interval of k_eval_spill on a wide batch (tests/wide_cases.py's generator at the same size) that holds
the same number of spill pods, by the same counters.  A profiled kg_eval records one interval per launch of
launch_eval_plain, in launch order: the slot kernel, then k_eval_spill if the batch has spill pods, then k_eval_elig if
it has restricted pods.

  python tools/elig_bench.py [--reps 10] [--out profiles/r08_elig/elig.json] [--baseline-only]

--baseline-only runs the wide batch alone (no eligibility entry point is called: it also runs on a library that
lacks them).  Medians and minima over --reps passes after two warm-up passes.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def intervals(eng, now_ns, reps, per_pass, dev):
    """[reps][per_pass] ms: the profiled launches of `reps` passes (after two warm-up passes); mask, score pairs and
    top1 into device buffers."""
    import torch
    P, W = eng.n_pods, eng.mask_words
    mask = torch.empty((P, W), dtype=torch.int64, device=dev)
    scores = torch.empty((P, W * 64, 2), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(P, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def one():
        eng.eval_device(now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr())
        eng.sync()

    eng.set_profiling(True)
    for _ in range(2):
        one()
    out = []
    for _ in range(reps):
        one()
        ms = eng.eval_kernel_times(per_pass)
        assert len(ms) == per_pass, (len(ms), per_pass)
        out.append(ms)
    eng.set_profiling(False)
    return np.array(out)


def stats(col):
    return {"median_ms": float(np.median(col)), "min_ms": float(col.min()), "max_ms": float(col.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000)
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_elig", "elig.json"))
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    import torch   # torch's HIP context first: it does not initialise beside a live engine
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile
    import wide_cases as wc

    P, N = a.pods, a.nodes
    n_restricted = (P + 3) // 4
    res = {"pods": P, "nodes": N, "restricted_pods": n_restricted, "reps": a.reps, "tiles": (N + 1023) // 1024}

    # ---- baseline: k_eval_spill on a wide batch with n_restricted spill pods ------------------------------------
    pool = wc.Case(N, 3 * P, wc.SEED, "least9")
    spill = np.flatnonzero(pool.spill)
    plain = np.flatnonzero(~pool.spill)
    assert len(spill) >= n_restricted and len(plain) >= P - n_restricted, (len(spill), len(plain))
    idx = np.sort(np.concatenate([spill[:n_restricted], plain[:P - n_restricted]]))
    rows = pool.pod_rows[idx]
    n_slots, _, sp = engine.batch_slot_map(pool.cfg, rows)   # (the sub-batch chooses its own map)
    with engine.Engine(pool.cfg) as eng:
        eng.load_snapshot(pool.node_rows)
        eng.set_pods(rows)
        n_spill = eng.spill_count()
        assert n_spill == int(sp.sum()) and n_spill > 0
        ms = intervals(eng, pool.cl.now_ns, a.reps, 2, dev)
    res["baseline_spill"] = {"spill_pods": n_spill, "n_slots": n_slots, "slot_kernel": stats(ms[:, 0]),
                             "k_eval_spill": stats(ms[:, 1]),
                             "k_eval_spill_per_pod_us": float(np.median(ms[:, 1])) * 1e3 / n_spill}
    print("baseline", json.dumps(res["baseline_spill"]), flush=True)

    # ---- k_eval_elig ---------------------------------------------------------------------------------------------
    if not a.baseline_only:
        cfg = shipped_profile()
        cl = synth.make_cluster(N, P, seed=2)
        node_rows = engine.build_node_rows(cfg, cl)
        pod_rows = engine.build_pod_rows(cfg, cl, np.arange(P))
        pod_rows["elig_class"][::4] = 1
        rng = np.random.default_rng(8)
        tiles = (N + 1023) // 1024
        pool_tiles = max(1, round(0.05 * tiles))
        pool5 = np.zeros(N, bool)
        pool5[(tiles // 2) * 1024:(tiles // 2 + pool_tiles) * 1024] = True
        classes = {"random50": rng.random(N) < 0.5, "random5": rng.random(N) < 0.05, "pool5": pool5}
        res["k_eval_elig"] = {}
        with engine.Engine(cfg) as eng:
            eng.load_snapshot(node_rows)
            for name, m in classes.items():
                eng.set_eligibility(m[None, :])
                eng.set_pods(pod_rows)
                assert eng.restricted_count() == n_restricted and eng.spill_count() == 0
                ms = intervals(eng, cl.now_ns, a.reps, 2, dev)
                words = np.packbits(np.pad(m, (0, -N % 64)).reshape(-1, 64), axis=1).any(axis=1)
                tile_any = np.pad(m, (0, -N % 1024)).reshape(-1, 1024).any(axis=1)
                r = {"eligible_share": float(m.mean()), "segments_with_an_eligible_node": float(words.mean()),
                     "tiles_with_an_eligible_node": float(tile_any.mean()), "slot_kernel": stats(ms[:, 0]),
                     "k_eval_elig": stats(ms[:, 1])}
                r["vs_spill_same_pods"] = r["k_eval_elig"]["median_ms"] / (
                    res["baseline_spill"]["k_eval_spill_per_pod_us"] * n_restricted / 1e3)
                res["k_eval_elig"][name] = r
                print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
