"""kg_preempt's PDB forms in guarded device buffers (nothing outside pick and plane is written, every in-range cell
is), and the seeded PDB case once on the bounds-checked engine (libkoordgpu_bounds.so, -DKG_BOUNDS_CHECK): the sites of
tests/test_preempt_bounds_gpu.py (133-141) and the new ones report no violation and the answers are the same.  New
sites: 142 (k_preempt's PDB forms: threshold plane slot and node), 143 (k_bound_pdb_fill: staged thresholds) and 144
(k_bound_pdb_fill: threshold plane slot and node)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import preempt_pdb_cases as ppc
from guarded_out import GuardedPlane
from koordinator_amd import _native as nat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")


@pytest.fixture(scope="module")
def dev():
    import torch   # torch's HIP context first: it does not initialise beside a live engine
    d = torch.device("cuda", 0)
    torch.zeros(1, device=d)
    torch.cuda.synchronize(d)
    return d


@pytest.mark.parametrize("prefill", [0x00, 0xFF])
def test_containment(dev, prefill):
    """Odd W (the first 1,025 nodes: W = 17, two tiles; the shard [1024, 1087): W = 1, a 63-node range that starts at
    the second tile), the pick pointer in the middle of a guarded allocation: guards intact, every in-range cell
    written whatever the buffers held."""
    import torch
    c = ppc.seeded()
    pods, prio = c.pods[:9], c.pod_prio[:9]
    ref = ppc.reference("seeded")[:9]
    for n_nodes, (lo, hi) in ((1_025, (0, 1_025)), (len(c.rows), (1_024, 1_087))):
        width = hi - lo
        stride = (width + 63) // 64 * 64
        want_pick, want_cells, _ = ppc.ref_arrays(ref, lo, hi)
        with ppc.engine_of(c, n_nodes) as eng:
            eng.set_shard(lo, hi)
            plane = GuardedPlane(len(pods) * stride * 4, prefill, dev)
            pick_b = len(pods) * nat.PREEMPT_PICK_WORDS * 8
            pick = GuardedPlane(4096 + 3 * pick_b, prefill, dev)   # the bytes before and after the picks are guards too
            torch.cuda.synchronize(dev)
            eng.preempt_device(pods, prio, c.now_ns, pick.ptr + 4096 + pick_b, plane_ptr=plane.ptr)
            assert plane.stray().size == 0 and pick.stray().size == 0
            payload = pick.read()[1]
            inner = payload[4096 + pick_b:4096 + 2 * pick_b]
            outer = np.concatenate([payload[:4096 + pick_b], payload[4096 + 2 * pick_b:]])
            assert (outer == prefill).all()
            np.testing.assert_array_equal(inner.view(np.int64).reshape(len(pods), nat.PREEMPT_PICK_WORDS), want_pick)
            cells = plane.read()[1].view(np.uint32).reshape(len(pods), stride)
            np.testing.assert_array_equal(cells[:, :width], want_cells)
            # picks alone (the PDB form without the plane)
            pick2 = GuardedPlane(pick_b, prefill, dev)
            torch.cuda.synchronize(dev)
            eng.preempt_device(pods, prio, c.now_ns, pick2.ptr)
            assert pick2.stray().size == 0
            np.testing.assert_array_equal(pick2.read()[1].view(np.int64).reshape(len(pods), nat.PREEMPT_PICK_WORDS), want_pick)


def run_bounds(out_dir):
    """In the child (KG_ENGINE_SO = the bounds build); a violation raises EngineError "bounds check: ..."."""
    c = ppc.seeded()
    th = ppc.thresholds("seeded")
    with ppc.engine_of(c) as eng:
        for j in (11, 16):   # k_bound_update's reset of a 1-pod and a 128-pod column, then k_bound_pdb_fill's values
            lo, hi = int(c.first[j]), int(c.first[j + 1])
            eng.update_bound_pods(j, c.b_rows[lo:hi], c.b_prio[lo:hi], c.b_start[lo:hi])
            eng.update_bound_pdb(j, th[lo:hi])
        full = eng.preempt(c.pods, c.pod_prio, c.now_ns, plane=True)
        alone = eng.preempt(c.pods, c.pod_prio, c.now_ns)
    np.savez(os.path.join(out_dir, "seeded.npz"), pick=full["pick"], plane=full["plane"], pick_alone=alone["pick"])


def test_preempt_pdb_bounds_build():
    assert os.path.exists(BOUNDS_SO), "libkoordgpu_bounds.so is built with the engine (koordinator_amd/build.py)"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_preempt_pdb_bounds_gpu as t\n"
            "t.run_bounds(sys.argv[1])\n"
            "print('RESULT ok')\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as out_dir:
        r = subprocess.run([sys.executable, "-c", code, out_dir], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO},
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, f"child exit {r.returncode}\n{r.stderr[-3000:]}"
        with np.load(os.path.join(out_dir, "seeded.npz")) as z:
            out = {k: z[k] for k in z.files}
    pick, cells, _ = ppc.ref_arrays(ppc.reference("seeded"))
    np.testing.assert_array_equal(out["pick"], pick)
    np.testing.assert_array_equal(out["pick_alone"], pick)
    np.testing.assert_array_equal(out["plane"][:, :cells.shape[1]], cells)
