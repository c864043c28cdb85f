"""kg_place_gangs on the bounds-checked build (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): sites 145-149 (k_gang_settle:
group, gang, pod, node and quota-group indices) and the resolve's own sites report no violation, and the answers are
the product build's — the scarce-resource case and the ElasticQuota case, each checked against the twin model in the
child process as well."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gang_ref as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest():
    """Both cases on the loaded library (gang_ref.compare inside), reduced to what the builds must share."""
    a, b = gr.scarce_summary(), gr.quota_summary()
    assert len(a["rolled"]) >= 3 and len(b["rolled"]) == int(b["k"]) - 1   # both cases roll a gang back
    return {"a_nodes": a["nodes"].tolist(), "a_verdicts": a["verdicts"].tolist(), "a_rows": _sha(a["rows"]),
            "b_nodes": b["nodes"].tolist(), "b_verdicts": b["verdicts"].tolist(), "b_rows": _sha(b["rows"]),
            "b_quotas": _sha(b["quotas"])}


def _child():
    code = ("import sys, json; sys.path[:0] = [%r, %r]\n"
            "import test_gangs_bounds_gpu as t\n"
            "from koordinator_amd import _native as nat\n"
            "assert nat.lib()._name.endswith('libkoordgpu_bounds.so')\n"
            "print('RESULT ' + json.dumps(t.digest()))\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO}, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]   # an EngineError "bounds check: ..." on a violation
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_gangs_bounds_build_reports_no_violation():
    assert os.path.exists(BOUNDS_SO), "build() makes the bounds-checked engine beside the product one"
    assert _child() == digest()
