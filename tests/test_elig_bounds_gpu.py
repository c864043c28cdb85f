"""Node eligibility classes on the bounds-checked engine (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): sites 106-112
(k_eval_elig) and the rest of the matrix and placement paths report no violation and give the same answers — the mixed
matrix case, the wide + restricted case and the chunk-16 placement, in a child process that loads the bounds build."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import elig_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")


def run_bounds(out_dir):
    """In the child (KG_ENGINE_SO = the bounds build); a violation raises EngineError "bounds check: ..." out of eval /
    place."""
    for name in ("mixed", "wide"):
        c = ec.case(name)
        with ec.engine_of(c) as eng:
            res = eng.eval(c.cl.now_ns)
            keys = eng.eval(c.cl.now_ns, mask=False, scores=False)["top1"]
        np.savez(os.path.join(out_dir, name + ".npz"), keys=keys, **res)
    c = ec.case("place16")
    with ec.engine_of(c) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
    np.savez(os.path.join(out_dir, "place.npz"), nodes=nodes, scores=scores)


def test_elig_bounds_build():
    assert os.path.exists(BOUNDS_SO), "libkoordgpu_bounds.so is built with the engine (koordinator_amd/build.py)"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_elig_bounds_gpu as t\n"
            "t.run_bounds(sys.argv[1])\n"
            "print('RESULT ok')\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as out_dir:
        r = subprocess.run([sys.executable, "-c", code, out_dir], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO},
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, f"child exit {r.returncode}\n{r.stderr[-3000:]}"
        outs = {}
        for name in ("mixed", "wide", "place"):
            with np.load(os.path.join(out_dir, name + ".npz")) as z:
                outs[name] = {k: z[k] for k in z.files}
    for name in ("mixed", "wide"):
        c = ec.case(name)
        ec.check_planes(c.cfg, outs[name], **c.planes())
        np.testing.assert_array_equal(outs[name]["keys"], outs[name]["top1"])
    ref_n, ref_s, _ = ec.case("place16").replayed
    np.testing.assert_array_equal(outs["place"]["nodes"], ref_n)
    np.testing.assert_array_equal(outs["place"]["scores"], ref_s)
