"""kg_diagnose on the bounds-checked engine (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): sites 113-118 (k_why,
k_why_reduce) report no violation and the answers are the same — the edited and the NodeNUMAResource case, with and
without the plane, in a child process that loads the bounds build."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import why_cases as wc
import why_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")
CASES = ("edited", "numa")


def run_bounds(out_dir):
    """In the child (KG_ENGINE_SO = the bounds build); a violation raises EngineError "bounds check: ..." out of
    diagnose."""
    for name in CASES:
        c = wc.case(name)
        with wc.engine_of(c) as eng:
            full = eng.diagnose(c.pods, c.now_ns, why=True)
            first = eng.diagnose(c.pods, c.now_ns, first_fail=True)
        np.savez(os.path.join(out_dir, name + ".npz"), first_counts=first["counts"], **full)


def test_why_bounds_build():
    assert os.path.exists(BOUNDS_SO), "libkoordgpu_bounds.so is built with the engine (koordinator_amd/build.py)"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_why_bounds_gpu as t\n"
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
    for name in CASES:
        n = len(wc.case(name).rows)
        ref = wc.reference(name)
        np.testing.assert_array_equal(outs[name]["why"][:, :n], ref)
        np.testing.assert_array_equal(outs[name]["counts"], why_ref.counts_ref(ref))
        np.testing.assert_array_equal(outs[name]["first_counts"], why_ref.counts_ref(wc.reference(name, True)))
        assert not outs[name]["pod_why"].any()
