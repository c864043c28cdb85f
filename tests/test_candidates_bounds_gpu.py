"""kg_candidates on the bounds-checked engine (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): sites 127-132 (k_cand,
k_cand_merge) report no violation and the answers are the same — the edited and the NodeNUMAResource case, with and
without the scores, in a child process that loads the bounds build."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import why_cases as wc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")
CASES = ("edited", "numa")
K = 16


def run_case(name):
    c = wc.case(name)
    with wc.engine_of(c) as eng:
        full = eng.candidates(c.pods, c.now_ns, K)
        bare = eng.candidates(c.pods, c.now_ns, 64, scores=False)
        eng.set_shard(0, 1_024 if len(c.rows) > 1_024 else 64)
        part = eng.candidates(c.pods, c.now_ns, K)
    return {"keys": full["keys"], "scores": full["scores"], "n_feasible": full["n_feasible"], "keys64": bare["keys"],
            "part_keys": part["keys"], "part_n_feasible": part["n_feasible"]}


def run_bounds(out_dir):
    """In the child (KG_ENGINE_SO = the bounds build); a violation raises EngineError "bounds check: ..." out of
    candidates."""
    for name in CASES:
        np.savez(os.path.join(out_dir, name + ".npz"), **run_case(name))


def test_candidates_bounds_build():
    assert os.path.exists(BOUNDS_SO), "libkoordgpu_bounds.so is built with the engine (koordinator_amd/build.py)"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_candidates_bounds_gpu as t\n"
            "t.run_bounds(sys.argv[1])\n"
            "print('RESULT ok')\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as out_dir:
        r = subprocess.run([sys.executable, "-c", code, out_dir], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO},
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, f"child exit {r.returncode}\n{r.stderr[-3000:]}"
        outs = {}
        for name in CASES:
            with np.load(os.path.join(out_dir, name + ".npz")) as z:
                outs[name] = {k: z[k] for k in z.files}
    for name in CASES:   # the product build, in this process
        want = run_case(name)
        assert want["keys"].any() and want["part_keys"].any()
        for k, v in want.items():
            np.testing.assert_array_equal(outs[name][k], v, err_msg=f"{name} {k}")
