"""Pod batches that compare or score more than 8 resources on the GPU (tests/wide_cases.py): kg_pods_set keeps the 8
most needed resources in the slot map and k_eval_spill evaluates the spill pods on the generic pair path, after every
slot-kernel launch — matrix mode (two tiles, the second partial; a shard; spill pods at either end of a batch that is
no multiple of the kernels' pod chunks; every pod a spill pod), the distinct-row NodeNUMAResource form (COMBINE reads
the repaired planes), placement through kg_place (sequential, pipelined, chunks of one), the chunk API and
kg_place_sharded, the bounds build, and one wide pod against kg_cycle_one.  Everything is compared with the oracle
exactly as tests/test_named_resources_gpu.py does; each test asserts its own preconditions (spill pods exist and have
feasible and infeasible nodes), so none passes on an easy batch."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import wide_cases as wc
from koordinator_amd import _native as nat
from koordinator_amd import engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_SO = os.path.join(ROOT, "koordinator_amd", "lib", "libkoordgpu_bounds.so")


def _engine(c, forms=0, shard=None):
    eng = engine.Engine(c.cfg)
    eng.set_forms(forms)
    eng.load_snapshot(c.node_rows)
    if shard:
        eng.set_shard(*shard)
    eng.set_pods(c.pod_rows)
    return eng


def _check_planes(c, out, m, f, l, begin=0, numa=None):
    """mask, both score planes where feasible, top-1 node (lowest index on ties) and total."""
    W = m.shape[1]
    np.testing.assert_array_equal(engine.unpack_mask(out["mask"], W), m)
    np.testing.assert_array_equal(out["scores"][:, :W, 0], np.where(m, f, out["scores"][:, :W, 0]))
    np.testing.assert_array_equal(out["scores"][:, :W, 1], np.where(m, l, out["scores"][:, :W, 1]))
    wf, wl, wn = int(c.cfg["weight_fit"]), int(c.cfg["weight_loadaware"]), int(c.cfg["weight_numa"])
    t = wf * f.astype(np.int64) + wl * l.astype(np.int64)
    if numa is not None:
        np.testing.assert_array_equal(out["numa_scores"][:, :W], np.where(m, numa, out["numa_scores"][:, :W]))
        t = t + wn * numa.astype(np.int64)
    t = np.where(m, t, -1)
    node, tot = engine.decode_top1(out["top1"])
    np.testing.assert_array_equal(node, np.where(t.max(axis=1) >= 0, t.argmax(axis=1) + begin, -1))
    np.testing.assert_array_equal(tot, t.max(axis=1))


@pytest.mark.parametrize("name", ["matrix_least9", "matrix_most4"])
def test_matrix_wide(name):
    c = wc.case(name)
    c.check_mixed()
    with _engine(c) as eng:
        assert eng.spill_count() == int(c.spill.sum())
        out = eng.eval(c.cl.now_ns)
    _check_planes(c, out, *c.matrix)


def test_matrix_wide_shard():
    c = wc.case("shard")
    begin, end = 1024, 2500
    m, f, l = (a[:, begin:end] for a in c.matrix)
    c.check_spill_rows(m)
    with _engine(c, shard=(begin, end)) as eng:
        out = eng.eval(c.cl.now_ns)
    assert out["mask"].shape[1] == (end - begin + 63) // 64   # planes cover the shard's columns only
    _check_planes(c, out, m, f, l, begin=begin)


@pytest.mark.parametrize("name", ["first", "last", "all"])
def test_matrix_spill_pod_positions(name):
    c = wc.case(name)
    want = {"first": [0], "last": [c.P - 1], "all": list(range(c.P))}[name]
    assert c.P == 37 and np.flatnonzero(c.spill).tolist() == want
    c.check_spill_rows()
    with _engine(c) as eng:
        assert eng.spill_count() == len(want)
        out = eng.eval(c.cl.now_ns)
        keys = eng.eval(c.cl.now_ns, mask=False, scores=False)["top1"]   # the keys-only form of the kernels
    _check_planes(c, out, *c.matrix)
    np.testing.assert_array_equal(keys, out["top1"])


def test_matrix_wide_distinct_rows_numa():
    """NodeNUMAResource on a batch of repeated rows: the distinct rows are evaluated (eq_on) by the Fit + LoadAware
    slot pass, the spill pass over it and k_eval_numa2's COMBINE form reading those planes back."""
    c = wc.case("numa_eq")
    assert c.P >= 64 and 4 * len({r.tobytes() for r in c.pod_rows}) <= 3 * c.P
    m, f, l, n = c.matrix3()
    assert c.n_slots == 8 and c.spill.any() and not c.spill.all()
    c.check_spill_rows(m)
    with _engine(c) as eng:
        assert eng.spill_count() == int(c.spill.sum())
        out = eng.eval(c.cl.now_ns)
    _check_planes(c, out, m, f, l, numa=n)


@pytest.mark.parametrize("name,forms", [("place", 0), ("place", nat.FORM_PLACE_PIPELINE), ("place1", 0)],
                         ids=["chunk16", "chunk16_pipeline", "chunk1"])
def test_place_wide(name, forms):
    c = wc.case(name)
    c.check_mixed()
    ref_n, ref_s = c.schedule
    assert (ref_n[c.spill] >= 0).any()
    with _engine(c, forms=forms) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
        after = eng.download()
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)
    np.testing.assert_array_equal(after, c.replay(nodes))


def test_place_wide_chunk_api_and_sharded():
    """The other routes to the chunk evaluation: kg_place_chunk_eval / kg_place_chunk_resolve_prev on their two
    streams (dist.place) and kg_place_sharded's own loop (one rank, loopback communicator)."""
    import torch
    from koordinator_amd import dist as kdist
    c = wc.case("place")
    ref_n, ref_s = c.schedule
    nodes, scores = kdist.place(c.cfg, c.node_rows, c.pod_rows, c.cl.now_ns, torch.device("cuda", 0))
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)
    eng = kdist.native_engine(c.cfg, c.node_rows, c.pod_rows, torch.device("cuda", 0), comm="loopback", rank=0,
                              world=1, shm_name=f"/kg_wide_{os.getpid()}")
    try:
        nodes, scores = eng.place_sharded(c.cl.now_ns)
    finally:
        eng.close()
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)


def run_bounds(out_dir):
    """In the child (KG_ENGINE_SO = the bounds build): the matrix case and the placement case; a violation raises
    EngineError "bounds check: ..." out of eval / place."""
    c = wc.case("matrix_least9")
    with _engine(c) as eng:
        res = eng.eval(c.cl.now_ns)
    np.savez(os.path.join(out_dir, "matrix.npz"), **res)
    c = wc.case("place")
    with _engine(c) as eng:
        nodes, scores = eng.place(c.cl.now_ns)
    np.savez(os.path.join(out_dir, "place.npz"), nodes=nodes, scores=scores)


def test_wide_bounds_build():
    """Sites 101-105 (k_eval_spill) and the rest of the matrix and placement paths on the bounds-checked engine: no
    verdict, the same answers."""
    assert os.path.exists(BOUNDS_SO), "libkoordgpu_bounds.so is built with the engine (koordinator_amd/build.py)"
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_wide_batch_gpu as t\n"
            "t.run_bounds(sys.argv[1])\n"
            "print('RESULT ok')\n") % (ROOT, os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as out_dir:
        r = subprocess.run([sys.executable, "-c", code, out_dir], env={**os.environ, "KG_ENGINE_SO": BOUNDS_SO},
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0 and "RESULT ok" in r.stdout, f"child exit {r.returncode}\n{r.stderr[-3000:]}"
        with np.load(os.path.join(out_dir, "matrix.npz")) as z:
            out = {k: z[k] for k in z.files}
        with np.load(os.path.join(out_dir, "place.npz")) as z:
            nodes, scores = z["nodes"], z["scores"]
    c = wc.case("matrix_least9")
    _check_planes(c, out, *c.matrix)
    ref_n, ref_s = wc.case("place").schedule
    np.testing.assert_array_equal(nodes, ref_n)
    np.testing.assert_array_equal(scores, ref_s)


def test_single_wide_pod_equals_cycle_one():
    """One pod that requests 10 resources: kg_pods_set + kg_eval (the slot kernel, then the spill kernel over it) picks
    what kg_cycle_one (the generic pair path alone) and the oracle pick."""
    c = wc.case("ten")
    p = 0
    assert (c.pod_rows["request"][p] > 0).sum() == 10 and bin(int(wc.pod_need(c.cfg, c.pod_rows)[p])).count("1") >= 10
    row = c.pod_rows[p:p + 1]
    m, f, l = (a[p] for a in c.matrix)
    assert m.any() and not m.all()
    t = np.where(m, int(c.cfg["weight_fit"]) * f.astype(np.int64) + int(c.cfg["weight_loadaware"]) * l, -1)
    with engine.Engine(c.cfg) as eng:
        eng.load_snapshot(c.node_rows)
        eng.set_pods(row)
        assert eng.spill_count() == 1
        key = int(eng.eval(c.cl.now_ns, mask=False, scores=False)["top1"][0])
        one = eng.cycle_one(row, c.cl.now_ns, commit=False)
    node, tot = engine.decode_top1(np.array([key], np.uint64))
    assert (int(node[0]), int(tot[0])) == (int(t.argmax()), int(t.max()))
    assert (one["key"], one["node"], one["score"]) == (key, int(t.argmax()), int(t.max()))
