"""The matrix-mode cases of tests/matrix_cases.py on the bounds-checked engine (libkoordgpu_bounds.so,
-DKG_BOUNDS_CHECK): every store, atomic and read-back of the matrix kernels into the mask, the score pairs, the NUMA
and Reservation planes, the per-(pod, tile) keys and top1 is checked on the device against its row and the row's width
(sites 60-100, the table in kg_engine.hip), a violation is skipped, recorded and reported by kg_eval as
EngineError "bounds check: ...".  One child process per family runs the family's whole case list with KG_ENGINE_SO
pointing at the bounds build (as test_bounds_gpu.py's _child_place); it raises on a violation and hands the planes
back, which must equal the oracle's exactly as in tests/test_matrix_guard_gpu.py.  The children run one after
another, each under its own timeout; once one aborts or times out no further child is started.

As in the guard tests, the small shapes do not reach k_eval_numa2's z < 8 grid splits (full-size tests only).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import matrix_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")
CHILD_TIMEOUT = 240   # seconds per family: its generators, one engine per case

_results = {}   # family → {case id: planes} | Exception
_stopped = []   # the family whose child aborted or timed out


def run_family(family, out_dir):
    """In the child: every case of the family through Engine.eval (the host path), the planes saved per case.
    A bounds violation raises EngineError out of eval."""
    for i, case in enumerate(mc.FAMILIES[family]):
        want = mc.planes_of(case)
        with mc.make_engine(case) as eng:
            res = eng.eval(mc.inputs(case).now_ns, numa_scores=want["numa"], rsv_scores=want["rsv"])
        np.savez(os.path.join(out_dir, f"{i}.npz"), **res)


def _child(family):
    if family in _results:
        return _results[family]
    if _stopped:
        raise RuntimeError(f"not started: the child of family {_stopped[0]!r} aborted or timed out")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_matrix_bounds_gpu as t\n"
            "t.run_family(sys.argv[1], sys.argv[2])\n"
            "print('RESULT ok')\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as out_dir:
        try:
            r = subprocess.run([sys.executable, "-c", code, family, out_dir], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO},
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            _stopped.append(family)
            _results[family] = RuntimeError(f"family {family}: the child timed out after {CHILD_TIMEOUT} s: {e}")
            raise _results[family]
        if r.returncode != 0 or "RESULT ok" not in r.stdout:
            if r.returncode < 0 or r.returncode in (134, 139):   # a signal: abort, segmentation fault
                _stopped.append(family)
            _results[family] = RuntimeError(f"family {family}: child exit {r.returncode}\n{r.stderr[-3000:]}")
            raise _results[family]
        out = {}
        for i, case in enumerate(mc.FAMILIES[family]):
            with np.load(os.path.join(out_dir, f"{i}.npz")) as z:
                out[case.id] = {k: z[k] for k in z.files}
    _results[family] = out
    return out


def _check(case):
    if not os.path.exists(BOUNDS_SO):
        pytest.skip("libkoordgpu_bounds.so not built (python koordinator_amd/build.py --bounds)")
    res = _child(case.family)
    if isinstance(res, Exception):
        raise res
    got = res[case.id]
    mc.check_against_reference(case, {"mask": got["mask"], "scores": got["scores"], "top1": got["top1"],
                                      "numa": got.get("numa_scores"), "rsv": got.get("rsv_scores")})


def _params(family):
    return pytest.mark.parametrize("case", mc.FAMILIES[family], ids=lambda c: c.id)


@_params("class")
def test_bounds_class_path(case):
    _check(case)


@_params("dup")
def test_bounds_duplicate_rows(case):
    _check(case)


@_params("slow")
def test_bounds_slow_nodes(case):
    _check(case)


@_params("la_extra")
def test_bounds_loadaware_extra_weights(case):
    _check(case)


@_params("numa")
def test_bounds_numa(case):
    _check(case)


@_params("bind")
def test_bounds_numa_cpuset_batch(case):
    _check(case)


@_params("rsv")
def test_bounds_reservation_quota(case):
    _check(case)
