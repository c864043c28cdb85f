"""The churn scripts of tests/churn_cases.py reach what tests/test_churn_gpu.py relies on (no GPU): every step kind and
every listed transition occurs — counted from the model rows' flags, the bounds predicates restated in numpy,
engine.batch_slot_map and the expiry rule of rows_eval — the two host references agree wherever both apply, every
checkpoint has feasible pairs and every place schedules at least half of its pods.  A GPU test that silently stopped
covering a transition fails here."""
import functools

import numpy as np
import pytest

import churn_cases as cc
from koordinator_amd import _native as nat
from koordinator_amd import engine

N = cc.N


class Trace:
    pass


@functools.lru_cache(maxsize=None)
def walk(name):
    """The script on the model alone: per upsert the rows before / after, per batch its rows and slot map, per
    checkpoint the host references (asserted equal where both apply), per place the placements."""
    s = cc.script(name)
    m = cc.Model(s)
    t = Trace()
    t.s, t.ups, t.batches, t.cps, t.places, t.order = s, [], [], [], [], []
    for st in s.steps:
        t.order.append(st.kind)
        if st.kind == "upsert":
            before = m.rows.copy()
            m.upsert(st)
            if not m.committed:   # the delta names every row it changed: the model equals a fresh build of the view
                keep = np.ones(N, bool)
                keep[list(m.removed)] = False
                full = engine.build_node_rows(s.cfg, st.view)
                assert (m.rows[keep] == full[keep]).all(), st.label
            t.ups.append(dict(step=st, before=before, after=m.rows.copy(), at=len(t.cps), committed=m.committed))
        elif st.kind == "remove":
            m.remove(st)
            t.ups.append(dict(step=st, before=None, after=m.rows.copy(), at=len(t.cps), committed=m.committed))
        elif st.kind == "pods":
            rows = m.pods(st)
            n_slots, slot_res, spill = engine.batch_slot_map(s.cfg, rows)
            t.batches.append(dict(step=st, rows=rows, n_slots=n_slots, spill=int(spill.sum()), at=len(t.cps),
                                  restricted=int((rows["elig_class"] != 0).sum()),
                                  la_prod=bool((rows["flags"] & nat.POD_LA_PROD_SCORE).any()),
                                  pow2=bool(cc.is_pow2(cc.pod_fit_w(s.cfg, rows)).all()),
                                  distinct=cc.distinct_rows(rows)))
        elif st.kind == "check":
            rec = dict(step=st, shard=m.shard, committed=m.committed, refs=[])
            if not m.committed:
                rec["oracle"] = m.oracle_planes(st.now_ns)
                rec["refs"].append("oracle")
            if m.has_rows_eval:
                rec["rows"] = m.rows_planes(st.now_ns)
                rec["refs"].append("rows")
            if len(rec["refs"]) == 2:
                cc.same_planes(rec["oracle"], rec["rows"], f"{name} / {st.label}")
            for k in rec["refs"]:
                assert rec[k]["mask"].any(), (name, st.label)
                assert rec[k]["mask"].shape == (len(m.pod_rows), m.shard[1] - m.shard[0])
            rec["expired"] = cc.rows_expired(s.cfg, m.rows, st.now_ns) & ((m.rows["flags"] & nat.NODE_HAS_METRIC) != 0)
            rec["n_ups"] = len(t.ups)
            t.cps.append(rec)
        elif st.kind == "place":
            nodes, scores, ref = m.place(st)
            assert 2 * int((nodes >= 0).sum()) >= len(nodes), (name, st.label)
            t.places.append(dict(step=st, nodes=nodes, scores=scores, ref=ref, shard=m.shard))
        else:
            m.apply(st)
    t.model = m
    return t


def _moves(t, pred):
    """Nodes for which pred(rows) turns on, and off, across the script's upserts."""
    on, off = set(), set()
    for u in t.ups:
        if u["before"] is None:
            continue
        a, b = pred(u["before"]), pred(u["after"])
        on |= set(np.flatnonzero(~a & b).tolist())
        off |= set(np.flatnonzero(a & ~b).tolist())
    return on, off


def _best(ref):
    return engine.decode_top1(ref["top1"])[0]


@pytest.mark.parametrize("name", list(cc.SCENARIOS))
def test_every_checkpoint_has_a_host_reference_or_follows_a_place(name):
    t = walk(name)
    assert t.cps and "pods" in t.order
    for c in t.cps:
        # the NUMA engine after its place has no host row evaluation: that checkpoint is the twin's alone
        assert c["refs"] or (name == "d_numa" and c["committed"]), c["step"].label


@pytest.mark.parametrize("name,deltas", [("a_class", 12), ("a_slot", 6)])
def test_scenario_a_reaches_its_transitions(name, deltas):
    t = walk(name)
    s, cfg = t.s, t.s.cfg
    ups = [u for u in t.ups if u["step"].kind == "upsert"]
    assert len(ups) == deltas and all(1 <= len(u["step"].idx) <= 40 for u in ups)
    assert {"upsert", "remove", "pods", "check", "place"} <= set(t.order)
    # the path: every pod specialisable (class path) or none of the cpu / memory pods (k_eval2)
    w = cc.pod_fit_w(cfg, t.batches[0]["rows"])
    assert cc.is_pow2(int(cfg["la_resource_weight"][:2].sum()))
    assert cc.is_pow2(w).all() if name == "a_class" else not cc.is_pow2(w).any()
    assert sum(1 for k in s.touched.values() if k >= 3) >= 5
    # out of the fp64 bounds and back, the tile corners and the ragged tile among them, by both predicates
    on, off = _moves(t, lambda r: cc.rows_slow(cfg, r)[0])
    for moved in (on, off):
        assert len(moved) >= 8 and set(cc.CORNERS) <= moved and any(cc.RAGGED <= j < N - 1 for j in moved)
    by_alloc, _ = _moves(t, lambda r: r["alloc"][:, cc.MEM] >= cc.CAP_LIMIT)
    by_base, _ = _moves(t, lambda r: cc.val_out(r["nonzero_requested"][:, 0]))
    assert len(by_alloc) >= 4 and len(by_base) >= 4
    # a node removed and later upserted valid again at the same index
    gone = [k for k, u in enumerate(t.ups) if u["step"].kind == "remove"]
    assert len(gone) == 1 and t.ups[gone[0]]["step"].node == cc.A_GONE
    back = [u for u in t.ups[gone[0] + 1:] if u["step"].kind == "upsert" and cc.A_GONE in u["step"].idx]
    assert back and back[0]["after"]["flags"][cc.A_GONE] & nat.NODE_VALID
    assert back[0]["at"] > t.ups[gone[0]]["at"]             # a checkpoint sees the node gone
    # metrics lost and regained, LoadAware-pass flags flipping both ways
    for bit, least in ((nat.NODE_HAS_METRIC, 8), (nat.NODE_LA_PASS_NONPROD, 4)):
        on, off = _moves(t, lambda r: (r["flags"] & bit) != 0)
        assert len(on) >= least and len(off) >= least, (bit, len(on), len(off))
    # a node that is some pod's best node only after a delta
    labels = [c["step"].label for c in t.cps]
    k = labels.index("star")
    ref = lambda c: c.get("oracle") or c["rows"]
    assert (_best(ref(t.cps[k])) == cc.A_STAR).any() and not (_best(ref(t.cps[k - 1])) == cc.A_STAR).any()
    # the places: the first against the oracle with checkpoints on both sides, whole rows overwritten afterwards
    assert int(cfg["place_chunk"]) == 16
    assert t.places[0]["ref"].startswith("oracle") and t.order.index("place") < len(t.order) - 2
    placed = set(t.places[0]["nodes"][t.places[0]["nodes"] >= 0].tolist())
    later = [u for u in t.ups if u["committed"] and u["step"].kind == "upsert"]
    assert later and placed & set(np.concatenate([u["step"].idx for u in later]).tolist())
    assert any(c["committed"] and c["refs"] == ["rows"] for c in t.cps)
    if name == "a_class":
        # the clock alone: two consecutive checkpoints, no delta between, at least 20 metrics expire
        assert cfg["la_has_expiration"]
        pairs = [(a, b) for a, b in zip(t.cps, t.cps[1:]) if a["n_ups"] == b["n_ups"]
                 and a["step"].now_ns != b["step"].now_ns and not a["committed"]]
        assert pairs and int((pairs[0][1]["expired"] & ~pairs[0][0]["expired"]).sum()) >= 20
        assert not np.array_equal(pairs[0][0]["oracle"]["la"], pairs[0][1]["oracle"]["la"])
        # the second place: the replay on the model rows, with an unschedulable pod
        assert len(t.places) == 2 and t.places[1]["ref"].startswith("replay")
        assert (t.places[1]["nodes"] < 0).any()
        on, _ = _moves(Trace_after(t), lambda r: cc.rows_slow(cfg, r)[0])
        assert len(on) >= 8                                  # out of the bounds again on committed rows


def Trace_after(t):
    """The upserts after the first commit."""
    x = Trace()
    x.ups = [u for u in t.ups if u["committed"]]
    return x


def test_scenario_b_reaches_its_transitions():
    t = walk("b_swaps")
    b = t.batches

    def seq(key, want):
        got = [x[key] if not callable(key) else key(x) for x in b]
        return any(got[i:i + len(want)] == list(want) for i in range(len(got)))

    assert seq("n_slots", (2, 8, 4, 2))
    assert seq(lambda x: len(x["rows"]), (96, 8, 1, 65, 96))
    assert max(len(x["rows"]) for x in b) == 96 and len(b[0]["rows"]) == 96          # the growth step comes first
    assert {len(x["rows"]) for x in b} >= {1, 8, 63, 64, 65, 96}
    assert seq(lambda x: x["spill"] > 0, (True, False)) and seq(lambda x: x["n_slots"] == 8 and x["spill"] == 0, (True,))
    assert seq(lambda x: x["restricted"] > 0, (True, False, True))
    assert seq("la_prod", (True, False, True))
    assert seq("pow2", (True, False, True))
    assert seq(lambda x: (len(x["rows"]), x["distinct"] <= 6, x["pow2"]), ((96, True, True),))
    assert b[-1]["distinct"] == len(b[-1]["rows"]) == 96 and b[-1]["pow2"] and not b[-1]["restricted"]
    # restricted classes 1..3 of elig_cases.class_masks; the table is updated between the two restricted batches
    r = [x for x in b if x["restricted"]]
    assert all(set(np.unique(x["rows"]["elig_class"]).tolist()) == {0, 1, 2, 3} for x in r)
    o = t.order
    assert o.index("elig") < o.index("pods") and "elig_update" in o
    assert sum(1 for u in t.ups if u["step"].kind == "upsert") == 2
    assert all(0 < u["at"] < len(t.cps) for u in t.ups)                              # in the middle
    assert all(c["shard"] == (0, N) and c["refs"] == ["oracle", "rows"] for c in t.cps)
    assert len(t.cps) == len(b)


def test_scenario_c_reaches_its_transitions():
    t = walk("c_shard")
    assert tuple(c["shard"] for c in t.cps[:5]) == cc.C_SHARDS
    assert [u["at"] for u in t.ups] == [3]                   # the delta lies between the third and fourth evaluation
    assert t.batches[0]["pow2"] and len(t.batches) == 1 and len(t.batches[0]["rows"]) == 65
    for c in t.cps[:5]:
        node = _best(c["oracle"])
        assert ((node == -1) | ((node >= c["shard"][0]) & (node < c["shard"][1]))).all() and (node >= 0).any()
    assert (_best(t.cps[3]["oracle"]) == 2090).any()         # the delta moves the small shard's best node
    p = t.places[0]
    assert p["shard"] == (1024, N) and (p["nodes"][p["nodes"] >= 0] >= 1024).all()


def test_scenario_d_reaches_its_transitions():
    t = walk("d_numa")
    s = t.s
    assert int(s.cfg["enabled_plugins"]) & nat.PLUGIN_NUMA and s.forms == nat.FORM_PLACE_PIPELINE
    b = t.batches
    assert len(b[0]["rows"]) == 96 and 64 < b[0]["distinct"] <= 72           # eq_on (≤ 3/4 distinct), eq_perm_on (> 64)
    assert len(b[1]["rows"]) == 65 and b[1]["distinct"] == 65                # eq_on off, numa_perm_on (> 64 pods)
    assert t.order == ["pods", "check", "upsert", "check", "pods", "check", "place", "upsert", "check"]
    for u in t.ups:
        ch = u["step"].idx
        assert (u["before"]["zone_allocated"][ch] != u["after"]["zone_allocated"][ch]).any()
        assert int((u["before"]["numa_policy"][ch] != u["after"]["numa_policy"][ch]).sum()) >= 5
    placed = set(t.places[0]["nodes"].tolist()) - {-1}
    assert len(placed & set(t.ups[1]["step"].idx.tolist())) >= 5             # the last delta rewrites placed nodes
    assert not (b[1]["rows"]["flags"] & nat.POD_NUMA_CPU_BIND).any()
    assert (t.cps[0]["oracle"]["numa"] != 0).any()


def test_scenario_e_reaches_its_transitions():
    t = walk("e_la_extra")
    cfg = t.s.cfg
    assert cfg["la_resource_weight"][2:].any()
    on, off = _moves(t, lambda r: cc.rows_slow(cfg, r)[1])
    assert len(on) >= 8 and len(off) >= 8 and set(cc.CORNERS) <= on and on == off
    slow_only, _ = _moves(t, lambda r: cc.rows_slow(cfg, r)[0])
    assert not slow_only                                     # the extra resource's plane alone sends them off
    assert t.order.count("pods") == 1 and len(t.cps) == 4
    x = cc.rows_slow(cfg, t.ups[1]["after"])[1]
    assert 4 <= int(x.sum()) and int(cc.rows_slow(cfg, t.ups[2]["after"])[1].sum()) == 0
    assert all(c["refs"] == ["oracle"] for c in t.cps)


def test_scenario_f_reaches_its_transitions():
    t = walk("f_rsv")
    s = t.s
    rsv = [st for st in s.steps if st.kind == "rsv"]
    assert len(rsv) == 2 and t.order == ["rsv", "pods", "check", "upsert", "check", "rsv", "check"]
    h0, h1 = set(rsv[0].rsv["node"].tolist()), set(rsv[1].rsv["node"].tolist())
    assert len(h0 - h1) >= 10 and len(h1 - h0) >= 10          # nodes that lose every slot, nodes that gain their first
    assert set(s.losers.tolist()) == h0 - h1 and set(s.gainers.tolist()) == h1 - h0
    # nodes outside the fp64 bounds on every side of the swap: the exact path under reservation slots coming and going
    slow = set(np.flatnonzero(cc.rows_slow(s.cfg, t.model.rows)[0]).tolist())
    assert slow == set(s.slow_nodes.tolist()) and len(slow & (h0 - h1)) == 2 and len(slow & (h1 - h0)) == 2
    assert len(slow - h0 - h1) == 2
    ch = set(t.ups[0]["step"].idx.tolist())
    assert len(ch & h0) >= 10 and len(ch - h0) >= 10
    for c in t.cps:
        assert c["refs"] == ["oracle"] and c["oracle"]["rsv"].max() == 100
    best0, best2 = _best(t.cps[1]["oracle"]), _best(t.cps[2]["oracle"])
    assert np.isin(best0, list(h0 - h1)).any() and (best0 != best2).any()   # a lost slot moves some pod's best node


def test_duplicate_upsert_case():
    c = cc.dup_case()
    assert len(c.idx) == 600 and len(np.unique(c.idx)) == 300 and (np.bincount(c.idx)[c.sel] == 2).all()
    assert set(cc.CORNERS) <= set(c.sel.tolist())
    first_pos = {int(n): k for k, n in reversed(list(enumerate(c.idx.tolist())))}
    last_pos = {int(n): k for k, n in enumerate(c.idx.tolist())}
    for k, n in enumerate(c.sel.tolist()):
        assert first_pos[n] < last_pos[n]
        assert c.rows[first_pos[n]] == c.rows_first[k] and c.rows[last_pos[n]] == c.rows_last[k]
    a, b = c.rows_first, c.rows_last
    assert ((a["alloc"] != b["alloc"]).any(axis=1) & (a["requested"] != b["requested"]).any(axis=1)).all()
    assert (a["la_used"].reshape(300, -1) != b["la_used"].reshape(300, -1)).any(axis=1).mean() > 0.9
    sa, sb = cc.rows_slow(c.cfg, a)[0], cc.rows_slow(c.cfg, b)[0]
    assert int((sa ^ sb).sum()) == 150 and sa.sum() >= 70 and sb.sum() >= 70 and not (sa & sb).any()
    assert (c.expect[c.sel] == b).all()
