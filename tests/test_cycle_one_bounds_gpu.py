"""k_cycle_one on the bounds-checked build (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): every plane index and the
committed node are checked on the device, and kg_cycle_one returns the build's verdict, so a violation fails the
call in the child process instead of being performed.  The shipped case with planes on 1,100 nodes (a ragged last
block) and the 257-node case (one column into the second block) must report none and answer like the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cycle_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")


def _child(n_nodes):
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import cycle_cases as cc\n"
            "from koordinator_amd import _native as nat\n"
            "assert nat.lib()._name.endswith('libkoordgpu_bounds.so')\n"
            "keys, masks, scores = cc.shipped_planes_keys(%r)\n"
            "print('RESULT ' + json.dumps([keys, masks.astype(int).tolist(), scores.astype(int).tolist()]))\n"
            ) % (ROOT, os.path.dirname(os.path.abspath(__file__)), n_nodes)
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO}, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]   # an EngineError "bounds check: ..." on a violation
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    keys, masks, scores = json.loads(line[len("RESULT "):])
    return keys, np.array(masks, bool), np.array(scores, np.uint8)


def test_cycle_one_bounds_build_reports_no_violation():
    assert os.path.exists(BOUNDS_SO), "build() makes the bounds-checked engine beside the product one"
    cfg, cl, rows, pods = cc.case("shipped")
    m, f, l, tot = cc.oracle_matrix("shipped")
    keys, masks, scores = _child(None)
    assert keys == [cc.key_of(t) for t in tot]
    np.testing.assert_array_equal(masks, m)
    np.testing.assert_array_equal(scores[:, :, 0], f)
    np.testing.assert_array_equal(scores[:, :, 1], l)
    keys, masks, scores = _child(257)
    for i in range(8):
        mi, fi, li, ti = cc.rows_totals(cfg, rows[:257], pods[i], cl.now_ns)
        assert keys[i] == cc.key_of(ti)
        np.testing.assert_array_equal(masks[i], mi)
        np.testing.assert_array_equal(scores[i, :, 0], fi)
        np.testing.assert_array_equal(scores[i, :, 1], li)
