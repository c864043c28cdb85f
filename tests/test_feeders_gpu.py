"""The informer-event feeders on the GPU: a seeded event stream drives an engine through
row deltas only (kg_snapshot_upsert of the rows each batch changed); the device snapshot then equals a fresh
build, and the ingest-built cluster's pending pods evaluate (kg_eval) and place (kg_place) exactly as the
oracle's matrix and sequential cycle over the same objects."""
import numpy as np
import pytest

from feeder_stream import Clock, pod_obj, run_stream
from koordinator_amd import _native as nat
from koordinator_amd import engine, feeders, ingest
from koordinator_amd.config import shipped_profile
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("numa", [False, True], ids=["shipped", "numa"])
def test_feeder_deltas_drive_engine_and_match_oracle(numa):
    rng = np.random.default_rng(11)
    cfg = shipped_profile()
    if numa:
        cfg["enabled_plugins"] |= nat.PLUGIN_NUMA
    clock = Clock(step=5 * 10**8)
    f = feeders.SnapshotFeeder(cfg, now_fn=clock)
    cap = 4096
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(np.zeros(cap, dtype=nat.NODE_ROW))        # capacity for every index the stream hands out
        written = []
        pods = run_stream(f, rng, clock, 40, numa=numa, allow_delete=False, nodes_per_step=(3, 8),
                          pods_per_step=(20, 40), on_step=lambda step: written.append(f.flush(eng)))
        got = eng.download(0, f.n_index)
        _, full = f.full_rows()
        np.testing.assert_array_equal(got, full)
        assert sum(written) > f.n_index                              # rows were rewritten by later events
        # the cluster as the objects describe it, with fresh pending pods
        cl = f.cluster()
        pend = [ingest.pod_from_object(p) for u, p in sorted(pods.items()) if not p["spec"]["nodeName"]]
        pend += [ingest.pod_from_object(pod_obj(f"q{i}", f"q{i}", cpu=["500m", "2", "4"][i % 3], mem=f"{1 + i % 5}Gi",
                                                phase="Pending")) for i in range(64)]
        view = cl.view(extra_pods=pend)
        idx = np.array([view.pod_index(p) for p in pend], dtype=np.int32)
        # the incrementally fed engine itself (capacity 4096, the planes the 40 steps of deltas left behind)
        eng.set_pods(engine.build_pod_rows(cfg, view, idx))
        fed = eng.eval(cl.now_ns)
        eng.load_snapshot(got)                                      # exactly the fed nodes, no spare capacity
        eng.set_pods(engine.build_pod_rows(cfg, view, idx))
        res = eng.eval(cl.now_ns)
        nodes, scores = eng.place(cl.now_ns)
    N = f.n_index
    if numa:
        m, fit, la, nm = oracle.eval_matrix3(cfg, view, idx, cl.now_ns)
        np.testing.assert_array_equal(res["numa_scores"][:, :N], nm)
        np.testing.assert_array_equal(fed["numa_scores"][:, :N], nm)
    else:
        m, fit, la = oracle.eval_matrix(cfg, view, idx, cl.now_ns)
    fed_mask = engine.unpack_mask(fed["mask"], cap)
    np.testing.assert_array_equal(fed_mask[:, :N], m)
    assert not fed_mask[:, N:].any()                                # never-fed capacity: no pod is feasible there
    np.testing.assert_array_equal(fed["scores"][:, :N, 0], fit)
    np.testing.assert_array_equal(fed["scores"][:, :N, 1], la)
    w = [int(cfg[k]) for k in ("weight_fit", "weight_loadaware", "weight_numa")]
    total = w[0] * fit.astype(np.int64) + w[1] * la.astype(np.int64) + (w[2] * nm.astype(np.int64) if numa else 0)
    total = np.where(m, total, -1)
    best_node, best_total = engine.decode_top1(fed["top1"])
    np.testing.assert_array_equal(best_total, total.max(axis=1))
    np.testing.assert_array_equal(best_node, np.where(total.max(axis=1) >= 0, total.argmax(axis=1), -1))
    np.testing.assert_array_equal(engine.unpack_mask(res["mask"], N), m)
    np.testing.assert_array_equal(res["scores"][:, :N, 0], fit)
    np.testing.assert_array_equal(res["scores"][:, :N, 1], la)
    assert m.any()
    ref_nodes, ref_scores = oracle.schedule(cfg, view, idx, cl.now_ns)
    np.testing.assert_array_equal(nodes, ref_nodes)
    np.testing.assert_array_equal(scores, ref_scores)
