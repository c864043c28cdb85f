"""Benchmark of the koord-scheduler Filter/Score hot path on MI355X.

Metric (BASELINE.json): pod×node Filter+Score evaluations per second (matrix mode) and pods
placed per second, LoadAwareScheduling + NodeResourcesFit (shipped profile args), synthetic
config 2 = 10k pods × 100k nodes per GPU.

A step = one matrix-mode pass: every (pod, node) pair of the resident pod batch against the
resident node shard → feasibility bit plane + {Fit, LoadAware} u8 score planes + per-pod best
node key; with N > 1 the per-pod keys of all shards are merged with an RCCL all-gather.

Scaling modes (--scaling):
  strong  (default; BASELINE's metric "at 100k nodes, 1/2/4/8 GPU") — one 100k-node cluster (seed 2)
          sharded over the N ranks, rank r owning nodes [r·100k/N, (r+1)·100k/N);
  config4 — BASELINE config 4: a 1M-node cluster sharded the same way (125k nodes per rank at N = 8);
  weak    — every rank owns its own 100k-node cluster (global nodes = N × 100k).
Placement (pods placed/s) runs over the same global node set: one GPU, or dist.place_sharded with
the snapshot replicated and the tile range sharded.

  python bench.py [--gpus N --steps K --warmup W] [--scaling strong|config4|weak] [--dump-outputs DIR] [--full]
  torchrun --nproc-per-node N bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the result line: the headline rate, ms_per_step and
what the timed steps themselves yield (HIP-event kernel time, engine counters).  --dump-outputs DIR also writes
what the last timed step computed as DIR/<name>.npy (dump_outputs).  --full adds every other section, each a run
of its own: host_outputs, placement, the CPU baselines, dropin_cycle, config2_distinct, config3, config5, la_extra;
the --no-* and --c*-pods options select among them.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # MI355X HBM3E peak, bytes/s (MI355X_MICROARCH.md)
BYTES_PER_PAIR = 2.125     # 1/8 feasibility bit + 2 u8 score planes
BYTES_PER_NODE = 104       # node SoA bytes per pass
BYTES_PER_POD = 64         # pod row bytes per pass


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pods", type=int, default=10_000)
    ap.add_argument("--nodes", type=int, default=100_000,
                    help="global nodes (strong) or nodes per GPU (weak); config4 uses 1M")
    ap.add_argument("--scaling", choices=("strong", "config4", "weak"), default="strong")
    ap.add_argument("--backend", default="nccl",
                    help="torch.distributed backend (gloo: CPU rehearsal of N > 1); loopback: gloo for the matrix-mode "
                         "merge and kg_place_sharded's native loop over the host shared-memory communicator "
                         "(kg_comm_init_loopback), so N ranks can share one GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other section (host outputs, placement, CPU baselines, "
                         "drop-in cycle, distinct pods, config 3, config 5, LoadAware extra resources)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64, < 64 MB)")
    ap.add_argument("--no-placement", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-distinct", action="store_true", help="skip the config2_distinct section")
    ap.add_argument("--no-host-outputs", action="store_true", help="skip the host_outputs (pinned, PCIe) section")
    ap.add_argument("--cpu-budget-s", type=float, default=12.0,
                    help="CPU-baseline budget per baseline: one timed run ≈ budget / 6 (warm-up + median of 5)")
    ap.add_argument("--c3-pods", type=int, default=1_000, help="config-3 (NodeNUMAResource) pods; 0 skips it")
    ap.add_argument("--c3-large-pods", type=int, default=10_000, help="config-3 matrix run at this many pods; 0 skips")
    ap.add_argument("--c3-distinct-pods", type=int, default=1_000,
                    help="config-3 matrix run over pairwise distinct pod rows (no equivalence); 0 skips")
    ap.add_argument("--c5-pods", type=int, default=100_000,
                    help="config-5 (Reservation + ElasticQuota) pods placed in sequence; 0 skips it")
    ap.add_argument("--c5-matrix-pods", type=int, default=1_000, help="config-5 matrix-mode pods")
    ap.add_argument("--dropin-cycles", type=int, default=1_000,
                    help="one-pod scheduling cycles through the C-ABI (kg_pods_set, kg_eval to host, kg_commit); 0 skips")
    ap.add_argument("--la-extra-pods", type=int, default=1_000,
                    help="matrix-mode pods with LoadAware resourceWeights beyond cpu / memory (k_eval_exact); 0 skips")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def pmc_traffic(kernel_prefix: str = "k_eval"):
    """HBM bytes per launch of the hot kernel from the committed rocprofv3 PMC passes of this same
    command (profiles/<CURRENT>/summary.json, written by tools/summarize_profile.py), its rocprofv3
    average duration (ms, all class-kind launches of one pass), and the source directory; Nones if absent."""
    try:
        with open(os.path.join(ROOT, "profiles", "CURRENT")) as f:
            tag = f.read().strip()
        with open(os.path.join(ROOT, "profiles", tag, "summary.json")) as f:
            s = json.load(f)
        hot = s.get("hot_kernel") or {}
        if not s.get("hbm_traffic_per_launch") or kernel_prefix not in hot.get("name", ""):
            return None, None, None
        return s["hbm_traffic_per_launch"]["total_bytes"], hot["avg_ns"] / 1e6, f"profiles/{tag}"
    except (OSError, ValueError, KeyError):
        return None, None, None


def cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor()


def host_info() -> dict:
    """The CPU the baselines ran on: model, logical CPUs of the machine and of this process."""
    try:
        avail = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        avail = os.cpu_count()
    return {"model": cpu_model(), "nproc": os.cpu_count(), "affinity_cpus": avail}


def cpu_median(run, cap, target_s=2.0, runs=5, start=4):
    """SURVEY §8d CPU-baseline method: grow the sample k until one run takes about `target_s`
    (k ≤ cap), one warm-up run at that size, then `runs` timed runs; returns (k, median s, all s)."""
    k = max(1, min(start, cap))
    while True:
        t0 = time.perf_counter()
        run(k)
        dt = time.perf_counter() - t0
        if dt >= target_s / 4 or k >= cap:
            break
        k = min(cap, k * 2)
    k = max(1, min(cap, int(k * target_s / max(dt, 1e-3))))
    run(k)
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        run(k)
        ts.append(time.perf_counter() - t0)
    return k, float(np.median(ts)), [round(t, 3) for t in ts]


DUMP_SAMPLE_BYTES = 48 << 20   # budget of the two sampled planes of dump_outputs (everything it writes < 64 MB)


def dump_outputs(out_dir, engine, mask, scores, merged, N):
    """--dump-outputs: what the last timed step left in the caller's buffers, as float arrays two builds can be
    compared by.  Over every pod: the merged top-1 key decoded (top1_node, top1_score: −1 = no feasible node), the
    number of feasible nodes (feasible_nodes) and the sum of each score plane over this rank's nodes (score_sums:
    [P][2] = Fit, LoadAware).  Over a fixed, seeded sample of pod rows, every node of this rank: the feasibility
    bits unpacked (mask_sample: [S][N] 0 / 1) and both u8 score planes (scores_sample: [S][N][2]); sample_pods
    holds the sampled pod indices."""
    import torch

    os.makedirs(out_dir, exist_ok=True)
    P, W = mask.shape
    node, total = engine.decode_top1(merged.cpu().numpy().view(np.uint64))
    arrays = {"top1_node": node.astype(np.float64), "top1_score": total.astype(np.float64)}
    # feasible nodes per pod: popcount of the mask words (bits past N in the last word left out), 1024 pods at a time
    lut = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=mask.device)
    tail = N - 64 * (W - 1)
    counts = torch.empty(P, dtype=torch.int64, device=mask.device)
    for p0 in range(0, P, 1024):
        m = mask[p0:p0 + 1024].clone()
        if tail < 64:
            m[:, -1] &= (1 << tail) - 1
        counts[p0:p0 + 1024] = lut[m.view(torch.uint8).long()].sum(dim=1)
    arrays["feasible_nodes"] = counts.cpu().numpy().astype(np.float64)
    arrays["score_sums"] = scores[:, :N, :].sum(dim=1, dtype=torch.int64).cpu().numpy().astype(np.float64)
    S = int(max(1, min(P, DUMP_SAMPLE_BYTES // (12 * N))))
    pods = np.sort(np.random.default_rng(20240607).choice(P, size=S, replace=False))
    idx = torch.from_numpy(pods).to(mask.device)
    arrays["sample_pods"] = pods.astype(np.float64)
    arrays["mask_sample"] = engine.unpack_mask(mask[idx].cpu().numpy().view(np.uint64), N).astype(np.float32)
    arrays["scores_sample"] = scores[idx][:, :N, :].cpu().numpy().astype(np.float32)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def bench_config3(args, engine, synth, shipped_profile, dev, stream, cpu_model):
    """BASELINE config 3: the shipped profile with NodeNUMAResource (weight 1) over 100k nodes with
    4/6/8 NUMA zones (synth.make_numa_cluster, seed 3).  Matrix mode: feasibility + Fit / LoadAware /
    NUMA score planes + top-1 (k_eval_numa2: pod per lane, per-wave LDS zone table); placement: sequential cycle with zone Reserve."""
    import torch

    from koordinator_amd import _native as nat

    P, N = args.c3_pods, args.nodes
    cl = synth.make_numa_cluster(N, P, seed=3)
    cfg = shipped_profile()
    cfg["enabled_plugins"] |= nat.PLUGIN_NUMA
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(P))
    eng = engine.Engine(cfg)
    eng.set_stream(stream.cuda_stream)
    eng.load_snapshot(rows)
    eng.set_pods(pods)
    W = eng.mask_words
    mask = torch.empty((P, W), dtype=torch.int64, device=dev)
    scores = torch.empty((P, W * 64, 2), dtype=torch.uint8, device=dev)
    numa = torch.empty((P, W * 64), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(P, dtype=torch.int64, device=dev)
    step = lambda: eng.eval_device(cl.now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr(), numa.data_ptr())
    step()
    torch.cuda.synchronize(dev)
    steps = 3
    eng.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    k_ms = float(np.mean(eng.eval_kernel_times(steps)))
    eng.set_profiling(False)
    feasible = float(engine.unpack_mask(mask[: min(P, 64)].cpu().numpy().view(np.uint64), N).mean())
    eng.load_snapshot(rows)
    torch.cuda.synchronize(dev)
    tp0 = time.perf_counter()
    nodes, _ = eng.place(cl.now_ns)
    tp1 = time.perf_counter()
    eng.close()
    out = {"workload": f"config3: {P} pods x {N} nodes, 4/6/8 NUMA zones, policy mix 40% SingleNUMANode / 30% "
                       "Restricted / 30% None, 60% LS / 40% batch pods, shipped profile + NodeNUMAResource",
           "evals_per_s": round(P * N / ((t1 - t0) / steps), 1), "ms_per_step": round((t1 - t0) / steps * 1e3, 3),
           "kernel": "Fit + LoadAware pass (slot kernels) + k_eval_numa2<COMBINE> over the distinct rows (kernel_ms; the k_eq_rows copies are in ms_per_step)",
           "kernel_ms": round(k_ms, 3), "feasible_frac_sample": round(feasible, 4),
           "placement": {"pods": P, "seconds": round(tp1 - tp0, 4), "pods_placed_per_s": round(P / (tp1 - tp0), 1),
                         "placed": int((nodes >= 0).sum())}}
    del mask, scores, numa
    if args.c3_large_pods > 0:
        # the top of SURVEY's 1k–10k pod range, matrix mode only
        PL = args.c3_large_pods
        cl_l = synth.make_numa_cluster(N, PL, seed=3)
        eng = engine.Engine(cfg)
        eng.set_stream(stream.cuda_stream)
        eng.load_snapshot(rows)
        eng.set_pods(engine.build_pod_rows(cfg, cl_l, np.arange(PL)))
        mask = torch.empty((PL, W), dtype=torch.int64, device=dev)
        scores = torch.empty((PL, W * 64, 2), dtype=torch.uint8, device=dev)
        numa = torch.empty((PL, W * 64), dtype=torch.uint8, device=dev)
        top1 = torch.zeros(PL, dtype=torch.int64, device=dev)
        step = lambda: eng.eval_device(cl.now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr(), numa.data_ptr())
        step()
        torch.cuda.synchronize(dev)
        eng.set_profiling(True)
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize(dev)
        tl = time.perf_counter() - t0
        kl = float(np.mean(eng.eval_kernel_times(1)))
        eng.close()
        del mask, scores, numa
        out["large"] = {"pods": PL, "evals_per_s": round(PL * N / tl, 1), "ms_per_step": round(tl * 1e3, 3),
                        "kernel_ms": round(kl, 3)}
    if args.c3_distinct_pods > 0:
        # the same config-3 nodes with pairwise distinct pod rows (continuous cpu / memory requests): no pod
        # equivalence: the class kernels' Fit + LoadAware pass, then k_eval_numa2<COMBINE> on every (pod, node) pair
        PD = args.c3_distinct_pods
        cl_d = synth.make_numa_cluster(N, PD, seed=3, distinct_pods=True)
        prow_d = engine.build_pod_rows(cfg, cl_d, np.arange(PD))
        eng = engine.Engine(cfg)
        eng.set_stream(stream.cuda_stream)
        eng.load_snapshot(rows)
        eng.set_pods(prow_d)
        mask = torch.empty((PD, W), dtype=torch.int64, device=dev)
        scores = torch.empty((PD, W * 64, 2), dtype=torch.uint8, device=dev)
        numa = torch.empty((PD, W * 64), dtype=torch.uint8, device=dev)
        top1 = torch.zeros(PD, dtype=torch.int64, device=dev)
        step = lambda: eng.eval_device(cl.now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr(), numa.data_ptr())
        step()
        torch.cuda.synchronize(dev)
        eng.set_profiling(True)
        t0 = time.perf_counter()
        for _ in range(3):
            step()
        torch.cuda.synchronize(dev)
        td = (time.perf_counter() - t0) / 3
        kd = float(np.mean(eng.eval_kernel_times(3)))
        eng.close()
        del mask, scores, numa
        distinct_rows = len({r.tobytes() for r in prow_d})
        out["distinct"] = {"pods": PD, "distinct_rows": distinct_rows, "evals_per_s": round(PD * N / td, 1),
                           "ms_per_step": round(td * 1e3, 3), "kernel_ms": round(kd, 3),
                           "roofline_frac": round(PD * N * 3.125 / (kd * 1e-3) / HBM_PEAK, 4)}
    if not args.no_cpu_baseline:
        from oracle import oracle  # CPU restatement, timed as the baseline only
        workers = min(16, os.cpu_count() or 1)
        k, med, ts = cpu_median(lambda k: oracle.eval_parallel(cfg, cl, np.arange(k), cl.now_ns, workers), P,
                                target_s=args.cpu_budget_s / 6)
        out["cpu_baseline"] = {"value": round(k * N / med, 1), "unit": "evals/s", "cores": workers, "kind": "port",
                               "sample": f"first {k} pods x {N} nodes of the same config-3 cluster, Filter+Score of "
                                         f"every pair with NodeNUMAResource, {workers}-thread node fan-out "
                                         f"(kgo_eval_parallel); median of {len(ts)} runs", "runs_s": ts,
                               "host": host_info()}
        k2, m2, t2s = cpu_median(lambda k: oracle.schedule_parallel(cfg, cl, np.arange(k), cl.now_ns, workers), P,
                                 target_s=args.cpu_budget_s / 6)
        out["placement"]["cpu_baseline"] = {
            "value": round(k2 / m2, 2), "unit": "pods placed/s", "cores": workers, "kind": "port",
            "sample": f"first {k2} pods, sequential cycle with zone Reserve and a {workers}-thread Parallelizer "
                      f"fan-out over nodes per pod (kgo_schedule_parallel); median of {len(t2s)} runs",
            "runs_s": t2s}
    return out


def bench_config2_distinct(args, engine, synth, cfg, node_rows, N, now, dev, stream):
    """Config 2's shape with pairwise distinct pod rows (synth distinct_pods: cpu / memory requests drawn from
    continuous ranges), so no two pods share an evaluation and every pair runs the per-pair kernel (k_eval3's
    plain part): the per-pair rate beside the headline, whose synthetic batch repeats ~105 request shapes and
    goes through the duplicate-row form (k_eval3_dup)."""
    import torch

    P = args.pods
    pods_cl = synth.make_cluster(1, P, seed=2, distinct_pods=True)
    rows = engine.build_pod_rows(cfg, pods_cl, np.arange(P))
    eng = engine.Engine(cfg)
    eng.set_stream(stream.cuda_stream)
    eng.load_snapshot(node_rows)
    eng.set_pods(rows)
    W = eng.mask_words
    mask = torch.empty((P, W), dtype=torch.int64, device=dev)
    scores = torch.empty((P, W * 64, 2), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(P, dtype=torch.int64, device=dev)
    step = lambda: eng.eval_device(now, mask.data_ptr(), scores.data_ptr(), top1.data_ptr())
    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    steps = max(3, args.steps // 2)
    eng.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    k_ms = float(np.mean(eng.eval_kernel_times(steps)))
    eng.close()
    algo = P * N * BYTES_PER_PAIR + N * BYTES_PER_NODE + P * BYTES_PER_POD
    distinct = len(np.unique(rows[["request", "fit_score_request", "la_estimate", "flags", "request_present"]]))
    return {"workload": f"config2 shape, {P} pods with pairwise distinct rows ({distinct} distinct) x {N} nodes, "
                        "shipped profile", "kernel": "k_eval3 (plain part)",
            "evals_per_s": round(P * N / dt, 1), "ms_per_step": round(dt * 1e3, 4), "kernel_ms": round(k_ms, 4),
            "roofline_frac": round(algo / (k_ms * 1e-3) / HBM_PEAK, 4)}


def bench_host_outputs(args, engine, eng, P, N, now, dev):
    """The drop-in boundary's rate (INTEGRATION.md `Eval`): the config-2 pass with the planes delivered to
    pinned host memory, the PCIe copy back included — what the Go plugins' PreFilter hook waits for."""
    import torch

    W = eng.mask_words
    mask = torch.empty((P, W), dtype=torch.int64, pin_memory=True)
    scores = torch.empty((P, W * 64, 2), dtype=torch.uint8, pin_memory=True)
    top1 = torch.empty(P, dtype=torch.int64, pin_memory=True)
    step = lambda: eng.eval_host(now, mask.data_ptr(), scores.data_ptr(), top1.data_ptr())
    step()
    steps = 3
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    dt = (time.perf_counter() - t0) / steps
    nbytes = mask.numel() * 8 + scores.numel() + top1.numel() * 8
    step2 = lambda: eng.eval_host(now, 0, 0, top1.data_ptr())
    step2()
    t1 = time.perf_counter()
    for _ in range(steps):
        step2()
    dt2 = (time.perf_counter() - t1) / steps
    del mask, scores, top1
    return {"workload": f"config2: {P} pods x {N} nodes, kg_eval into pinned host buffers (out_on_device = 0)",
            "planes": {"evals_per_s": round(P * N / dt, 1), "ms_per_step": round(dt * 1e3, 3),
                       "host_bytes": int(nbytes), "d2h_GB_per_s": round(nbytes / dt / 1e9, 1)},
            "top1_only": {"evals_per_s": round(P * N / dt2, 1), "ms_per_step": round(dt2 * 1e3, 3)}}


def bench_dropin_cycle(args, engine, eng, node_rows, pod_rows, now, ref_nodes):
    """The drop-in boundary as the Go scheduler drives it: scheduleOne is per pod, so every
    cycle is one pod — PreFilter uploads its row (kg_pods_set, P = 1), Filter / Score read the pod's planes from one
    kg_eval over all nodes into pinned host memory (feasibility bits + {Fit, LoadAware} u8 scores + top-1: what the
    plugins' O(1) lookups read), selectHost takes the best node, Reserve commits it (kg_commit).  µs per cycle over
    `--dropin-cycles` pods of the config-2 queue, from the same snapshot as kg_place; the placements must equal
    kg_place's (the sequential cycle) pod for pod."""
    import torch

    C = min(args.dropin_cycles, len(pod_rows))
    N = len(node_rows)
    W = (N + 63) // 64
    mask = torch.empty((1, W), dtype=torch.int64, pin_memory=True)
    scores = torch.empty((1, W * 64, 2), dtype=torch.uint8, pin_memory=True)
    top1 = torch.zeros(1, dtype=torch.int64, pin_memory=True)
    top_np = top1.numpy().view(np.uint64)
    eng.load_snapshot(node_rows)

    def cycles(planes: bool, n: int, out=None):
        t0 = time.perf_counter()
        for p in range(n):
            eng.set_pods(pod_rows[p:p + 1])
            eng.eval_host(now, mask.data_ptr() if planes else 0, scores.data_ptr() if planes else 0, top1.data_ptr())
            node = -1 if top_np[0] == 0 else int(0xFFFFFFFF - (int(top_np[0]) & 0xFFFFFFFF))
            if node >= 0:
                eng.commit(0, node)
            if out is not None:
                out.append(node)
        return time.perf_counter() - t0

    cycles(True, 8)   # warm-up (first-use allocations), then from the fresh snapshot
    eng.load_snapshot(node_rows)
    got = []
    dt = cycles(True, C, got)
    eng.load_snapshot(node_rows)
    dt_top = cycles(False, C)
    eng.load_snapshot(node_rows)
    # the batch upload alone (kg_pods_set's class / equivalence grouping of the 10k headline batch, host work outside
    # every other timer)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        eng.set_pods(pod_rows)
        ts.append(time.perf_counter() - t0)
    return {"workload": f"config2: {C} pods, one scheduling cycle each over {N} nodes (kg_pods_set P = 1 -> kg_eval "
                        "into pinned host planes -> selectHost -> kg_commit)",
            "cycles": C, "us_per_cycle": round(dt / C * 1e6, 1), "pods_per_s": round(C / dt, 1),
            "top1_only": {"us_per_cycle": round(dt_top / C * 1e6, 1), "pods_per_s": round(C / dt_top, 1)},
            "host_bytes_per_cycle": int(W * 8 + W * 64 * 2 + 8),
            "matches_kg_place": bool(np.array_equal(np.asarray(got), np.asarray(ref_nodes[:C]))),
            "pods_set_10k_ms": {"median": round(float(np.median(ts)) * 1e3, 2), "runs": [round(t * 1e3, 2) for t in ts],
                                "pods": int(len(pod_rows))}}


def bench_la_extra(args, engine, synth, shipped_profile, dev, stream):
    """Matrix mode with LoadAware resourceWeights beyond cpu / memory (ephemeral-storage, an extended resource,
    batch-cpu; estimatedScalingFactors for the first two): k_eval2's LAX form reads fp64 planes of the weighted
    extra resources beside the cpu / memory ones (up to KG_LAX = 4 of them; more take k_eval_exact).  Config-2-shaped cluster with those
    resources (synth.make_la_extra_cluster, seed 2), shipped profile."""
    import torch

    P, N = args.la_extra_pods, args.nodes
    weights = {"cpu": 1, "memory": 1, "ephemeral-storage": 1, "example.com/gpu": 2, "kubernetes.io/batch-cpu": 1}
    cl = synth.make_la_extra_cluster(N, P, seed=2)
    cfg = shipped_profile(resource_weights=weights,
                          estimated_scaling_factors={"ephemeral-storage": 60, "example.com/gpu": 100})
    eng = engine.Engine(cfg)
    eng.set_stream(stream.cuda_stream)
    eng.load_snapshot(engine.build_node_rows(cfg, cl))
    eng.set_pods(engine.build_pod_rows(cfg, cl, np.arange(P)))
    W = eng.mask_words
    mask = torch.empty((P, W), dtype=torch.int64, device=dev)
    scores = torch.empty((P, W * 64, 2), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(P, dtype=torch.int64, device=dev)
    step = lambda: eng.eval_device(cl.now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr())
    step()
    torch.cuda.synchronize(dev)
    steps = 3
    eng.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / steps
    k_ms = float(np.mean(eng.eval_kernel_times(steps)))
    eng.close()
    return {"workload": f"{P} pods x {N} nodes, shipped profile, LoadAware resourceWeights {weights}",
            "kernel": "k_eval2 LAX form (fp64 planes of the weighted extra resources; exact pair path for nodes "
                      "outside their bounds)", "evals_per_s": round(P * N / dt, 1), "ms_per_step": round(dt * 1e3, 3),
            "kernel_ms": round(k_ms, 3)}


def bench_config5(args, engine, synth, shipped_profile, dev, stream, cpu_model):
    """BASELINE config 5: colocation burst — batch pods with Reservation (weight 5000) and ElasticQuota
    over 100k nodes, 10 % of them with 1–2 reservations, 16 owner classes, 64 quota groups at 80 % of
    demand (synth.make_rsv_cluster, seed 5).  Placement = greedy sequential commit (kg_place); matrix
    mode on a pod sample; the CPU baseline is the oracle's sequential cycle on a bounded pod prefix."""
    import torch

    from koordinator_amd import _native as nat

    P, N, PM = args.c5_pods, args.nodes, min(args.c5_matrix_pods, args.c5_pods)
    cl = synth.make_rsv_cluster(N, P, seed=5)
    cfg = shipped_profile()
    cfg["enabled_plugins"] |= nat.PLUGIN_RESERVATION | nat.PLUGIN_ELASTICQUOTA
    rows = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(P))
    eng = engine.Engine(cfg)
    eng.set_stream(stream.cuda_stream)

    def reset(pod_rows):
        eng.load_snapshot(rows)
        eng.set_reservations(cl.rsv_arr)
        eng.set_quotas(cl.quota_arr)
        eng.set_pods(pod_rows)

    # matrix mode on the first PM pods
    reset(pods[:PM])
    W = eng.mask_words
    mask = torch.empty((PM, W), dtype=torch.int64, device=dev)
    scores = torch.empty((PM, W * 64, 2), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(PM, dtype=torch.int64, device=dev)
    step = lambda: eng.eval_device(cl.now_ns, mask.data_ptr(), scores.data_ptr(), top1.data_ptr())
    step()
    torch.cuda.synchronize(dev)
    # device time of the whole pass (every launch of kg_eval is on the engine stream: the Fit / LoadAware kernel
    # over the plain nodes, k_rsv_eval / k_rsv_reduce over the reservation nodes, the quota gate)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t0 = time.perf_counter()
    ev[0].record(stream)
    for _ in range(3):
        step()
    ev[1].record(stream)
    torch.cuda.synchronize(dev)
    tm = (time.perf_counter() - t0) / 3
    dev_ms = ev[0].elapsed_time(ev[1]) / 3
    # placement of the whole burst
    reset(pods)
    torch.cuda.synchronize(dev)
    tp0 = time.perf_counter()
    nodes, _ = eng.place(cl.now_ns)
    tp = time.perf_counter() - tp0
    rsv_after = eng.download_reservations()
    eng.close()
    rnodes = set(cl.rsv_arr["node"].tolist())
    on_rsv = int(sum(1 for n in nodes[nodes >= 0].tolist() if n in rnodes))
    out = {"workload": f"config5: {P} batch pods x {N} nodes, {len(rnodes)} nodes with {len(cl.rsv_arr)} reservations "
                       f"(16 owner classes), {len(cl.quota_arr)} ElasticQuota groups at 80% of demand, shipped profile "
                       "+ Reservation (weight 5000) + ElasticQuota",
           "placement": {"pods": P, "seconds": round(tp, 4), "pods_placed_per_s": round(P / tp, 1),
                         "placed": int((nodes >= 0).sum()), "placed_on_reservation_nodes": on_rsv,
                         "reservation_assignments": int((rsv_after["n_assigned"] - cl.rsv_arr["n_assigned"]).sum()),
                         "mode": "kg_place (greedy sequential commit, touched-node re-score)"},
           "matrix": {"pods": PM, "evals_per_s": round(PM * N / tm, 1), "ms_per_step": round(tm * 1e3, 3),
                      "device_ms": round(dev_ms, 3),
                      "roofline_frac": round((PM * N * BYTES_PER_PAIR + N * BYTES_PER_NODE) / (dev_ms * 1e-3) / HBM_PEAK, 4)}}
    if not args.no_cpu_baseline:
        from oracle import oracle  # CPU restatement of the sequential cycle, timed as the baseline only
        k, med, ts = cpu_median(lambda k: oracle.schedule2(cfg, cl, np.arange(k), cl.now_ns), P,
                                target_s=args.cpu_budget_s / 6)
        out["cpu_baseline"] = {"value": round(k / med, 2), "unit": "pods placed/s", "cores": 1, "kind": "port",
                               "sample": f"first {k} pods of the same burst, sequential cycle over all {N} nodes "
                                         f"(oracle/koord_oracle.c kgo_schedule2); median of {len(ts)} runs",
                               "runs_s": ts, "host": host_info()}
    return out


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawned_rank(rank: int, world: int, port: int) -> None:
    """Entry of one rank started by `launch` (a fresh interpreter: nothing GPU-side is inherited)."""
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
                       "LOCAL_WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    main()


def launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks, one process per GPU, before this
    process touches the GPU (torch.cuda.device_count() does not initialise it), and return the worst
    exit code.  Under torchrun (WORLD_SIZE set) --gpus must equal WORLD_SIZE."""
    import torch
    import torch.multiprocessing as mp

    ndev = torch.cuda.device_count()
    if args.backend == "nccl" and args.gpus > ndev:
        print(f"bench.py: --gpus {args.gpus} with backend nccl needs {args.gpus} GPUs, this node has {ndev} "
              "(use --backend gloo to rehearse more ranks than GPUs)", file=sys.stderr)
        return 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_spawned_rank, args=(r, args.gpus, port)) for r in range(args.gpus)]
    for p in procs:
        p.start()
    for p in procs:
        p.join()
    codes = [p.exitcode for p in procs]
    bad = [c for c in codes if c != 0]
    return 0 if not bad else (bad[0] if bad[0] and bad[0] > 0 else 1)


def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch(args))
    if env_world is not None and int(env_world) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}; they must agree", file=sys.stderr)
        sys.exit(2)
    import torch
    import torch.distributed as dist

    from koordinator_amd import engine, synth
    from koordinator_amd.config import shipped_profile

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    gpu = local % ndev if args.backend != "nccl" else local
    if world > 1:
        torch.cuda.set_device(gpu)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", gpu))
        else:
            dist.init_process_group("gloo" if args.backend == "loopback" else args.backend)
    dev = torch.device("cuda", gpu)
    torch.cuda.set_device(dev)

    P = args.pods
    cfg = shipped_profile(device=gpu)
    pods_cl = synth.make_cluster(1, P, seed=2)   # the same pod batch on every rank (config-2 pods)
    pod_rows = engine.build_pod_rows(cfg, pods_cl, np.arange(P))
    if args.scaling == "weak":
        N = args.nodes
        total = N * world
        cl = synth.make_cluster(N, P, seed=2 + 7919 * rank)   # rank 0 = BASELINE config 2 (seed 2)
        global_rows = None
        node_rows = engine.build_node_rows(cfg, cl)
        offset = rank * N
    else:
        total = 1_000_000 if args.scaling == "config4" else args.nodes
        cl = synth.make_cluster(total, P, seed=4 if args.scaling == "config4" else 2)
        global_rows = engine.build_node_rows(cfg, cl)
        offset, end = rank * total // world, (rank + 1) * total // world
        N = end - offset
        node_rows = np.ascontiguousarray(global_rows[offset:end])
    now = cl.now_ns

    eng = engine.Engine(cfg)
    # one dedicated stream for the engine kernels and the torch / RCCL ops around them (the legacy
    # null stream cannot be shared: kg_set_stream(NULL) means an engine-owned stream)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    eng.set_stream(stream.cuda_stream)
    eng.load_snapshot(node_rows)
    eng.set_pods(pod_rows)

    words = eng.mask_words
    mask = torch.empty((P, words), dtype=torch.int64, device=dev)
    scores = torch.empty((P, words * 64, 2), dtype=torch.uint8, device=dev)
    top1 = torch.zeros(P, dtype=torch.int64, device=dev)
    gathered = torch.zeros((world, P), dtype=torch.int64, device=dev) if world > 1 else None

    def step():
        eng.eval_device(now, mask.data_ptr(), scores.data_ptr(), top1.data_ptr())
        if world > 1:
            keys = torch.where(top1 != 0, top1 - offset, top1)       # local → global node index
            if args.backend != "nccl":          # gloo rehearsal: the equivalent max all-reduce
                from koordinator_amd import dist as kdist
                kdist.merge_top1_(keys)
                return keys
            dist.all_gather_into_tensor(gathered.view(-1), keys)
            return gathered.max(dim=0).values
        return top1

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    eng.set_profiling(True)
    eng.reset_counters()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        merged = step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    ctr = eng.counters()   # kg_counters_get over the timed steps (SURVEY §5 metrics)
    kernel_ms = eng.eval_kernel_times(args.steps)
    eng.set_profiling(False)
    elapsed = t1 - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / args.steps * 1e3
    evals_per_s = P * total / (elapsed / args.steps)

    k_ms = float(np.mean(kernel_ms)) if len(kernel_ms) else float("nan")
    algo_bytes = P * N * BYTES_PER_PAIR + N * BYTES_PER_NODE + P * BYTES_PER_POD
    achieved = algo_bytes / (k_ms * 1e-3)
    feasible_pods = int((merged != 0).sum().item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, engine, mask, scores, merged, N)

    full = args.full   # every section below is a run of its own beside the timed steps
    host_out = None   # before placement: the same snapshot as the timed steps
    if full and not args.no_host_outputs and world == 1:
        host_out = bench_host_outputs(args, engine, eng, P, N, now, dev)

    placement = None
    if not full or args.no_placement:
        pass
    elif world == 1:
        eng.load_snapshot(node_rows)
        torch.cuda.synchronize(dev)
        tp0 = time.perf_counter()
        nodes, tot = eng.place(now)
        tp1 = time.perf_counter()
        placement = {"pods": P, "nodes": N, "seconds": round(tp1 - tp0, 6),
                     "pods_placed_per_s": round(P / (tp1 - tp0), 1), "placed": int((nodes >= 0).sum()),
                     "chunk": int(cfg["place_chunk"]), "mode": "kg_place, one GPU"}
    else:
        # node-sharded sequential cycle over the union of every rank's shard (replicated snapshot,
        # per-tile partial keys merged with RCCL all_reduce(MAX), replicated resolve: koordinator_amd/dist.py)
        from koordinator_amd import dist as kdist
        all_rows = global_rows if global_rows is not None else np.concatenate(
            [engine.build_node_rows(cfg, synth.make_cluster(N, 1, seed=2 + 7919 * r)) for r in range(world)])
        # kg_place_sharded on the engine's own communicator: RCCL, or the loopback one (ranks sharing a GPU)
        native = args.backend in ("nccl", "loopback")
        comm = "loopback" if args.backend == "loopback" else "rccl"
        deng = (kdist.native_engine(cfg, all_rows, pod_rows, dev, stream=stream, comm=comm) if native
                else kdist.sharded_engine(cfg, all_rows, pod_rows, dev))
        dist.barrier()
        torch.cuda.synchronize(dev)
        tp0 = time.perf_counter()
        if native:
            nodes, tot = deng.place_sharded(now)
        else:   # gloo rehearsal: the Python chunk loop over torch.distributed
            nodes, tot = kdist.place_sharded(deng, now, dev, chunk=kdist.place_chunk_of(cfg))
        dist.barrier()
        tp1 = time.perf_counter()
        deng_kind = deng.comm_kind() if native else None
        deng.close()
        placement = {"pods": P, "nodes": total, "seconds": round(tp1 - tp0, 6),
                     "pods_placed_per_s": round(P / (tp1 - tp0), 1), "placed": int((nodes >= 0).sum()),
                     "chunk": int(cfg["place_chunk"]),
                     "mode": (f"kg_place_sharded over {world} ranks ({deng_kind})" if native
                              else f"dist.place_sharded over {world} ranks ({args.backend})")}

    cpu_baseline = None
    if full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import oracle  # CPU restatement, timed as the baseline only
        workers = min(16, os.cpu_count() or 1)
        k, med, ts = cpu_median(lambda k: oracle.eval_parallel(cfg, cl, np.arange(k), now, workers), P,
                                target_s=args.cpu_budget_s / 6)
        cpu_baseline = {"value": round(k * N / med, 1), "unit": "evals/s", "cores": workers, "kind": "port",
                        "sample": f"first {k} pods x {N} nodes of the same config-2 cluster, Filter+Score of every pair, "
                                  f"Parallelizer-faithful {workers}-thread node fan-out (oracle/koord_oracle.c "
                                  f"kgo_eval_parallel); median of {len(ts)} runs after a warm-up",
                        "runs_s": ts, "host": host_info(),
                        "sampling_note": "every node scored (percentageOfNodesToScore 100, INTEGRATION.md §2); "
                                         "the upstream default (adaptive: max(5, 50 - nodes/125) %) would stop "
                                         f"Filter after {max(100, N * max(5, 50 - N // 125) // 100)} feasible nodes "
                                         "per pod and Score only those"}
        if placement is not None:
            # placement baselines: the sequential cycle, single-threaded and with the 16-thread
            # Parallelizer fan-out over nodes per pod (kgo_schedule_parallel), on a pod prefix
            k1, m1, t1s = cpu_median(lambda k: oracle.schedule(cfg, cl, np.arange(k), now), P,
                                     target_s=args.cpu_budget_s / 6)
            k2, m2, t2s = cpu_median(lambda k: oracle.schedule_parallel(cfg, cl, np.arange(k), now, workers), P,
                                     target_s=args.cpu_budget_s / 6)
            placement["cpu_baseline"] = {
                "sequential": {"value": round(k1 / m1, 2), "unit": "pods placed/s", "cores": 1, "kind": "port",
                               "sample": f"first {k1} pods, sequential cycle over all {N} nodes (kgo_schedule); "
                                         f"median of {len(t1s)} runs", "runs_s": t1s},
                "parallel": {"value": round(k2 / m2, 2), "unit": "pods placed/s", "cores": workers, "kind": "port",
                             "sample": f"first {k2} pods, sequential cycle with a {workers}-thread Parallelizer fan-out "
                                       f"over nodes per pod (kgo_schedule_parallel); median of {len(t2s)} runs",
                             "runs_s": t2s},
                "host": host_info()}

    dropin = None
    if args.dropin_cycles > 0 and world == 1 and placement is not None:
        dropin = bench_dropin_cycle(args, engine, eng, node_rows, pod_rows, now, nodes)
        if placement.get("cpu_baseline"):
            seq = placement["cpu_baseline"]["sequential"]
            dropin["cpu_baseline"] = {"us_per_cycle": round(1e6 / seq["value"], 1), "kind": "port", "cores": 1,
                                      "sample": "the oracle's sequential cycle per pod (placement.cpu_baseline.sequential)"}

    distinct = None
    if full and not args.no_distinct and world == 1:
        distinct = bench_config2_distinct(args, engine, synth, cfg, node_rows, N, now, dev, stream)

    config3 = None
    if full and args.c3_pods > 0 and world == 1:
        config3 = bench_config3(args, engine, synth, shipped_profile, dev, stream, cpu_model)

    config5 = None
    if full and args.c5_pods > 0 and world == 1:
        config5 = bench_config5(args, engine, synth, shipped_profile, dev, stream, cpu_model)

    la_extra = None
    if full and args.la_extra_pods > 0 and world == 1:
        la_extra = bench_la_extra(args, engine, synth, shipped_profile, dev, stream)

    # the committed PMC passes profile the default workload (tools/profile.sh: config 2, one GPU)
    profiled = world == 1 and args.scaling == "strong" and P == 10_000 and total == 100_000
    traffic, prof_ms, traffic_src = pmc_traffic() if profiled else (None, None, None)
    if rank == 0:
        line = {
            "metric": "pod×node Filter+Score evals/sec (LoadAwareScheduling + NodeResourcesFit, matrix mode)",
            "value": round(evals_per_s, 1),
            "unit": "evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak" if args.scaling == "weak" else "strong",
            "vs_baseline": None,
            "dtype": "int64",
            "data": "synthetic",
            "config": {"workload": (f"{'config4' if args.scaling == 'config4' else 'config2'}: {P} pods x {total} nodes "
                                    f"({N} on rank 0 of {world}, {args.scaling} scaling), shipped-profile args, "
                                    "outputs: feasibility bits + Fit/LoadAware u8 scores + per-pod top-1"),
                       "pods": P, "nodes": total, "nodes_per_gpu": N, "parallelism": f"node-shard x{world}"},
            "roofline": {"bound": "hbm", "achieved": round(achieved / 1e9, 1), "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK, 4),
                         "frac_source": "this run's HIP-event kernel time (kernel_ms); frac_rocprof uses the committed "
                                        "rocprofv3 --kernel-trace --stats average of the same command (a different box: "
                                        "box-to-box spread ≈ 10 %)",
                         "kernel_ms_rocprof": None if prof_ms is None else round(prof_ms, 4),
                         "frac_rocprof": None if prof_ms is None else round(algo_bytes / (prof_ms * 1e-3) / HBM_PEAK, 4),
                         "traffic": None if traffic is None else int(traffic), "traffic_unit": "bytes per launch (PMC)",
                         "traffic_source": traffic_src,
                         "kernel": "k_eval3_dup (duplicate-row form of k_eval3: ~105 distinct pod rows over the 10k pods)",
                         "kernel_ms": round(k_ms, 4),
                         "kernel_ms_source": "HIP events on the engine stream around the k_eval3 launches of each "
                                             "timed step (kg_set_profiling), this run; rocprofv3 summaries of the "
                                             "same command are under profiles/",
                         "algorithmic_bytes_per_launch": int(algo_bytes)},
            "cpu_baseline": cpu_baseline,
            "placement": placement,
            "host_outputs": host_out,
            "dropin_cycle": dropin,
            "config2_distinct": distinct,
            "config3": config3,
            "config5": config5,
            "la_extra": la_extra,
            "pods_with_feasible_node": feasible_pods,
            "engine_counters": {**ctr, "source": "kg_counters_get over the timed steps of rank 0",
                                "evals_per_kernel_s": round(ctr["evals"] / (ctr["kernel_ns"] * 1e-9), 1)
                                if ctr["kernel_ns"] else None,
                                "out_GB_per_kernel_s": round(ctr["out_bytes"] / ctr["kernel_ns"], 1)
                                if ctr["kernel_ns"] else None},
        }
        print(json.dumps(line), flush=True)
    eng.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
