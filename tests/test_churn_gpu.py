"""One engine that lives through a whole script (tests/churn_cases.py): row deltas, removed and returning nodes, batch
swaps of every shape, a moving shard, an advancing clock, reservations replaced, placements in between.  What a call
returns then depends on state earlier calls left behind — the derived planes k_upsert wrote, the lazily rebuilt slow
lists, kg_pods_set's per-batch lists and reused buffers, the class tables' layout — and every checkpoint compares it
with every reference that applies, never with the long-lived engine itself:

    oracle   the CPU oracle on the edited view (until the first commit),
    rows     the snapshot download equals the model rows after every step, and for Fit + LoadAware engines the planes
             equal rows_ref.rows_eval on them (exact numpy int64),
    twin     a fresh engine loaded with the model rows, the same tables, shard, forms and batch: every plane bit-equal.

tests/test_churn_cpu.py asserts that the scripts reach the transitions they are written for."""
import os

import numpy as np
import pytest

import churn_cases as cc
from koordinator_amd import _native as nat
from koordinator_amd import engine

pytestmark = pytest.mark.gpu


def _twin_eval(script, m, now_ns):
    """Reference 3: a fresh engine in the model's state."""
    with engine.Engine(script.cfg) as t:
        t.set_forms(script.forms)
        t.load_snapshot(m.rows)
        if m.rsv is not None:
            t.set_reservations(m.rsv)
        if m.masks is not None:
            t.set_eligibility(m.masks)
        t.set_shard(*m.shard)
        t.set_pods(m.pod_rows)
        return t.eval(now_ns), t.spill_count(), t.restricted_count()


def _checkpoint(script, m, eng, st):
    what = f"{script.name} / {st.label}"
    got = eng.eval(st.now_ns)
    b, e = m.shard
    used = []
    full = eng.spill_count() == 0 and eng.restricted_count() == 0
    if not m.committed:
        cc.compare(got, m.oracle_planes(st.now_ns), e - b, full, f"{what} vs oracle")
        used.append("oracle")
    if m.has_rows_eval:
        cc.compare(got, m.rows_planes(st.now_ns), e - b, full, f"{what} vs rows")
        used.append("rows")
    twin, spill, restricted = _twin_eval(script, m, st.now_ns)
    assert (eng.spill_count(), eng.restricted_count()) == (spill, restricted), what
    assert set(got) == set(twin)
    for k in got:
        np.testing.assert_array_equal(got[k], twin[k], err_msg=f"{what} vs twin: {k}")
    used.append("twin")
    print(f"{what}: P={len(m.pod_rows)} shard={m.shard} references: {', '.join(used)}")
    return used


def _run(name):
    script = cc.script(name)
    m = cc.Model(script)
    log = []
    with engine.Engine(script.cfg) as eng:
        eng.set_forms(script.forms)
        eng.load_snapshot(m.rows)
        for st in script.steps:
            if st.kind == "upsert":
                eng.upsert(st.idx, m.upsert(st))
            elif st.kind == "remove":
                m.remove(st)
                eng.remove(st.node)
            elif st.kind == "pods":
                eng.set_pods(m.pods(st))
            elif st.kind == "check":
                log.append((st.label, _checkpoint(script, m, eng, st)))
                continue
            elif st.kind == "place":
                if m.shard == (0, m.n):
                    nodes, scores = eng.place(st.now_ns)
                else:   # kg_place answers the whole snapshot; a shard is placed by kg_place_sharded (here one rank)
                    eng.comm_init_loopback(0, 1, f"/kg_churn_{os.getpid()}")
                    nodes, scores = eng.place_sharded(st.now_ns)
                ref_nodes, ref_scores, ref = m.place(st)
                np.testing.assert_array_equal(nodes, ref_nodes, err_msg=f"{name} / {st.label} vs {ref}")
                np.testing.assert_array_equal(scores, ref_scores, err_msg=f"{name} / {st.label} vs {ref}")
                print(f"{name} / {st.label}: reference: {ref}")
            else:
                m.apply(st)
                if st.kind == "shard":
                    eng.set_shard(*st.shard)
                elif st.kind == "elig":
                    eng.set_eligibility(st.masks)
                elif st.kind == "elig_update":
                    eng.update_eligibility(st.cls, st.nodes, st.eligible)
                elif st.kind == "rsv":
                    eng.set_reservations(st.rsv)
            # the snapshot equals the model rows after every step
            np.testing.assert_array_equal(eng.download(), m.rows, err_msg=f"{name} / {st.label}: snapshot rows")
    # no checkpoint rests on the long-lived engine alone, and the twin is never the only reference before a commit
    assert log and all("twin" in used for _, used in log)
    assert all(len(used) >= 2 for _, used in log) or name == "d_numa"
    return log


@pytest.mark.parametrize("name", ["a_class", "a_slot"])
def test_row_deltas(name):
    """Scenario A: row deltas on a shipped-profile engine — rows rewritten over and over, nodes out of the fp64 bounds
    and back (slow_list), a node removed and returning, metrics lost, regained and expiring by the clock alone, a
    place against the oracle, then committed rows overwritten and a second place against the replay on the rows.
    a_class: k_eval3 / k_eval3_dup; a_slot: a Fit weight sum of 3 sends the batch to k_eval2."""
    log = _run(name)
    assert any(used == ["oracle", "rows", "twin"] for _, used in log) and any(used == ["rows", "twin"] for _, used in log)


def test_batch_swaps():
    """Scenario B: eleven batches replace each other on one engine (slot profile 2 → 8 → 4 → 2, spill pods and none,
    restricted pods, none, restricted again after update_eligibility, la_prod on / off, class path / slot path,
    P = 96 → 8 → 1 → 65 → 96 with buffer reuse, duplicate rows then distinct ones), two row deltas in the middle."""
    log = _run("b_swaps")
    assert all(used == ["oracle", "rows", "twin"] for _, used in log)


def test_moving_shard():
    """Scenario C: one uploaded class-path batch evaluated at five shards (cls_layout's width / tile change), a delta
    in between, then a place on the upper shard; top-1 nodes stay global."""
    _run("c_shard")


def test_numa_engine():
    """Scenario D: NodeNUMAResource — zone amounts rewritten and policies toggled under a 96-pod batch of 70 rows
    (eq_on, eq_perm_on) and a distinct 65-pod one (numa_perm_on), a pipelined place (k_ncache_*), then placed nodes
    rewritten.  The oracle until the place, the twin after it."""
    log = _run("d_numa")
    assert [used for _, used in log] == [["oracle", "twin"]] * 3 + [["twin"]]


def test_la_extra_engine():
    """Scenario E: LoadAware extra resources — nodes' ephemeral-storage usage past the bound (KGD_XSLOW, xslow_list)
    and back between evaluations of one batch."""
    _run("e_la_extra")


def test_reservations():
    """Scenario F: set_reservations, rows of slot holders and of other nodes upserted, set_reservations with another
    slot set; oracle.eval_matrix5 and the twin, the rsv_scores plane included."""
    _run("f_rsv")


def test_duplicate_indices_in_one_upsert():
    """Scenario G: one kg_snapshot_upsert call of 600 entries that names 300 nodes twice.  The contract (koord_gpu.h):
    entries apply in order, the last entry of an index wins.  The snapshot then equals the last rows, and the planes
    derive from them: evaluation == oracle on the last rows == a fresh twin.

    The parent commit can pass this by luck of scheduling: k_upsert ran one thread per staged entry, each writing the
    row and then deriving the planes from whatever row was stored, so with both entries of a node in flight the result
    depended on the order the threads ran in.  The fix (kg_snapshot_upsert keeps the last entry per index on the host
    before staging; the kernel never sees a duplicate) is justified from the code, not from an observed failure.
    Also: an empty upsert is a no-op, and a single row at index N − 1 lands."""
    c = cc.dup_case()
    cfg, now = c.cfg, c.cl.now_ns
    pods = engine.build_pod_rows(cfg, c.cl, c.pod_idx)
    with engine.Engine(cfg) as eng:
        eng.load_snapshot(engine.build_node_rows(cfg, c.cl))
        eng.set_pods(pods)
        before = eng.eval(now)
        gen = eng.generation()
        eng.upsert(np.zeros(0, np.int32), np.zeros(0, nat.NODE_ROW))
        assert eng.generation() == gen
        np.testing.assert_array_equal(eng.download(), engine.build_node_rows(cfg, c.cl))
        eng.upsert(c.idx, c.rows)
        np.testing.assert_array_equal(eng.download(), c.expect)
        got = eng.eval(now)
        # a single row at the last index
        last = c.expect[cc.N - 1:].copy()
        last["requested"][0, cc.CPU] += 1000
        last["nonzero_requested"][0, 0] += 1000
        eng.upsert([cc.N - 1], last)
        np.testing.assert_array_equal(eng.download(cc.N - 1, 1), last)
        np.testing.assert_array_equal(eng.download(0, cc.N - 1), c.expect[:cc.N - 1])
        one = eng.eval(now)
    m, f, l = cc.oracle.eval_matrix(cfg, c.view_last, c.pod_idx, now)
    ref = dict(mask=m, fit=f, la=l, top1=cc._keys(m, cc.elig_cases.totals(cfg, f, l), 0))
    cc.compare(got, ref, cc.N, True, "duplicates vs oracle on the last rows")
    assert not np.array_equal(before["scores"], got["scores"])
    with engine.Engine(cfg) as twin:
        twin.load_snapshot(c.expect)
        twin.set_pods(pods)
        fresh = twin.eval(now)
        rows = c.expect.copy()
        rows[cc.N - 1:] = last
        twin.load_snapshot(rows)
        twin.set_pods(pods)
        fresh_one = twin.eval(now)
    for k in got:
        np.testing.assert_array_equal(got[k], fresh[k], err_msg=f"duplicates vs twin: {k}")
        np.testing.assert_array_equal(one[k], fresh_one[k], err_msg=f"single row vs twin: {k}")
    mr, fr, lr = cc.rows_ref.rows_eval(cfg, rows, pods, now)
    np.testing.assert_array_equal(engine.unpack_mask(one["mask"], cc.N), mr)
    np.testing.assert_array_equal(one["scores"][:, :cc.N, 0], fr)
    np.testing.assert_array_equal(one["scores"][:, :cc.N, 1], lr)
