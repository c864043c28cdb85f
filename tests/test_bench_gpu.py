"""bench.py's plain run: --steps sets the timed steps, the other sections stay behind --full, and
--dump-outputs writes what the last timed step computed (checked against Engine.eval over the same rows)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from koordinator_amd import engine, synth
from koordinator_amd.config import shipped_profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
P, N = 200, 3000   # 47 mask words, the last one with 56 valid bits
FULL_SECTIONS = ("cpu_baseline", "placement", "host_outputs", "dropin_cycle", "config2_distinct", "config3",
                 "config5", "la_extra")


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--pods", str(P),
                        "--nodes", str(N), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["engine_counters"]["eval_calls"] == 3
    assert line["ms_per_step"] > 0 and line["unit"] == "evals/s" and line["dtype"] == "int64"
    assert line["higher_is_better"] is True
    # ms_per_step is printed to 1e-4 ms and a step takes at least 0.01 ms (one launch): 1 % covers the rounding
    assert line["value"] == pytest.approx(P * N / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert all(line[k] is None for k in FULL_SECTIONS)

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(got) == {"top1_node", "top1_score", "feasible_nodes", "score_sums", "sample_pods", "mask_sample",
                        "scores_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the same rows as bench.py builds them, through the host-array form of the same pass
    cfg = shipped_profile()
    pod_rows = engine.build_pod_rows(cfg, synth.make_cluster(1, P, seed=2), np.arange(P))
    cl = synth.make_cluster(N, P, seed=2)
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(engine.build_node_rows(cfg, cl))
        eng.set_pods(pod_rows)
        ref = eng.eval(cl.now_ns)
    bits = engine.unpack_mask(ref["mask"], N)
    node, total = engine.decode_top1(ref["top1"])
    assert bits.any() and not bits.all()
    np.testing.assert_array_equal(got["top1_node"], node)
    np.testing.assert_array_equal(got["top1_score"], total)
    np.testing.assert_array_equal(got["feasible_nodes"], bits.sum(axis=1))
    np.testing.assert_array_equal(got["score_sums"], ref["scores"][:, :N].astype(np.int64).sum(axis=1))
    pods = got["sample_pods"].astype(np.int64)
    assert len(pods) == P and (np.diff(pods) > 0).all()
    np.testing.assert_array_equal(got["mask_sample"], bits[pods])
    np.testing.assert_array_equal(got["scores_sample"], ref["scores"][pods][:, :N])
