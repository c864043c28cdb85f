"""k_unreserve / k_unreserve_quota on the bounds-checked build (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): every row,
plane, entry, slot and quota index is checked on the device and kg_unreserve returns the build's verdict, so a
violation fails the call in the child process instead of being performed.  The Fit + LoadAware case and the
Reservation + ElasticQuota case must report none and return what the product build returns."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import unreserve_cases as uc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest():
    """Both cases on the loaded library: checked against the host model, then reduced to what the builds must share."""
    a = uc.fit_la_rollback()
    assert a["released"].all() and a["rows"].tobytes() == a["model_rows"].tobytes()
    uc.same_eval(a["eval"], a["ref_eval"], "Fit + LoadAware")
    b = uc.rsv_quota_rollback()
    assert b["released"].all() and b["got"]["rows"].tobytes() == b["model"].rows.tobytes()
    np.testing.assert_array_equal(b["got"]["rsv"], b["model"].rsv)
    np.testing.assert_array_equal(b["got"]["quotas"], b["model"].quotas)
    np.testing.assert_array_equal(b["place"][0], b["ref_place"][0])
    return {"a_nodes": a["nodes"].tolist(), "a_rows": _sha(a["rows"]), "a_top1": a["eval"]["top1"].tolist(),
            "a_place": a["place"][0].tolist(), "b_nodes": b["nodes"].tolist(), "b_rows": _sha(b["got"]["rows"]),
            "b_rsv": _sha(b["got"]["rsv"]), "b_quotas": _sha(b["got"]["quotas"]), "b_place": b["place"][0].tolist()}


def _child():
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import test_unreserve_bounds_gpu as t\n"
            "from koordinator_amd import _native as nat\n"
            "assert nat.lib()._name.endswith('libkoordgpu_bounds.so')\n"
            "print('RESULT ' + json.dumps(t.digest()))\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO}, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]   # an EngineError "bounds check: ..." on a violation
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_unreserve_bounds_build_reports_no_violation():
    assert os.path.exists(BOUNDS_SO), "build() makes the bounds-checked engine beside the product one"
    assert _child() == digest()
