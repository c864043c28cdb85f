"""The designed Reservation / ElasticQuota clusters (tests/rsv_edge_cases.py) do what they claim, judged by the
oracle alone — otherwise the GPU tests of tests/test_rsv_edges_gpu.py could pass vacuously — and the engine's host
code agrees with the oracle on them: the host-row mirror of the per-pod reduction (rsv_cases.rows_matrix5) and
kg_row_eval_rsv against kgo_rsv_pair for every (pod, reservation node) pair."""
import functools
import json
import os

import numpy as np
import pytest

import rsv_edge_cases as rc
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import make_config, shipped_profile
from oracle import oracle
from rsv_cases import rows_matrix5

RSV = ("NodeResourcesFit", "LoadAwareScheduling", "Reservation")
RSV_EQ = RSV + ("ElasticQuota",)
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _one_copy():
    ec = rc.make_rsv_edge_cluster(1)
    out = {}
    for cp in (0, 1):
        cfg = shipped_profile(plugins=RSV_EQ, eq_check_parent_quota=cp)
        out[cp] = oracle.eval_matrix5(cfg, ec.view, np.arange(ec.n_pods), ec.view.now_ns)
    return ec, out


def _plane(ec, res, pod, tags):
    m, _, _, _, rsv, _ = res
    p = ec.pod(pod)
    return [(bool(m[p, ec.node(t)]), int(rsv[p, ec.node(t)])) for t in tags]


def _pair(ec, pod, node_tag):
    """oracle.rsv_pair of (pod tag, unit tag)."""
    return oracle.rsv_pair(make_config(plugins=("Reservation",)), ec.view, ec.pod(pod), ec.node(node_tag))


def test_normalize_score_without_a_preferred_node():
    """mx = mraw: the classes' planes hold exactly floor(100·raw / mraw); over the cluster at least 20 distinct values
    lie strictly between 10 and 100, and every class's maximum is 100."""
    ec, res = _one_copy()
    m, _, _, _, rsv, _ = res[0]
    seen = set()
    for name, raws in rc.MRAWS.items():
        p = ec.pod(name)
        got = {r: int(rsv[p, ec.node(f"{name}:{r}")]) for r in raws}
        assert got == {r: 100 * r // max(raws) for r in raws}, name
        assert all(m[p, ec.node(f"{name}:{r}")] for r in raws)
        assert rsv[p].max() == 100
        assert not any(int(ec.view.rsv_arr["order"][i]) for i in np.flatnonzero(
            ec.view.rsv_arr["owner_classes"] & np.uint32(1 << rc.CLS[name])))
        seen |= set(got.values())
    for p in range(ec.n_pods):
        seen |= set(rsv[p][m[p]].tolist())
    assert len({s for s in seen if 10 < s < 100}) >= 20
    # floor steps: 1/3, 2/3, 1/7 .. 6/7, 16/33 | 17/33 around one half, 98/99, 49/50
    p = ec.pod("M33")
    assert (int(rsv[p, ec.node("M33:16")]), int(rsv[p, ec.node("M33:17")])) == (48, 51)
    assert int(rsv[ec.pod("M99"), ec.node("M99:98")]) == 98 and int(rsv[ec.pod("M50"), ec.node("M50:49")]) == 98


def test_zero_maximum_and_preferred_node():
    ec, res = _one_copy()
    m, _, _, _, rsv, _ = res[0]
    # feasible nominated entries, all of raw 0: an all-zero plane
    z = ec.pod("Z")
    for t in ("Z:0", "Z:1"):
        ok, raw, nom = _pair(ec, "Z", t)
        assert ok and raw == 0 and nom == 0 and m[z, ec.node(t)]
    assert m[z].any() and rsv[z].max() == 0
    # the preferred node holds the class's largest raw: the override wins and the others scale by 1000
    assert _pair(ec, "P", "P:pref")[1] == 80
    assert _plane(ec, res[0], "P", ["P:pref", "P:40", "P:60"]) == [(True, 100), (True, 4), (True, 6)]
    # the minimal order tied across three nodes: the lowest node
    assert _plane(ec, res[0], "T", ["T:0", "T:1", "T:2"]) == [(True, 100), (True, 3), (True, 4)]
    assert ec.node("T:0") < ec.node("T:1") < ec.node("T:2")
    # the two smallest orders sit on infeasible nodes (Fit; Reservation.Filter) and are skipped
    assert _plane(ec, res[0], "I", ["I:fit", "I:rsv", "I:pref", "I:next"]) == [(False, 0), (False, 0), (True, 100), (True, 5)]
    assert _pair(ec, "I", "I:fit")[0] and not _pair(ec, "I", "I:rsv")[0]   # the first by Fit alone, the second by Reservation
    # order magnitudes: the smallest non-zero int64 wins; INT64_MAX never does
    for pod, want in (("OA", "OA:1"), ("OB", "OB:1"), ("OC", "OC:1"), ("OD", "OD:1"), ("OE", "OE:1")):
        p = ec.pod(pod)
        cols = ec.nodes_of(pod + ":")
        assert [j for j in cols if rsv[p, j] == 100] == [ec.node(want)], pod
    # the node order comes from the matched set (a Restricted reservation that does not fit), the nomination from
    # the fitting set
    ok, raw, nom = _pair(ec, "R", "R:two")
    assert ok and nom == 1 and raw == 50
    assert _plane(ec, res[0], "R", ["R:two", "R:other"]) == [(True, 100), (True, 3)]
    # equal nomination scores: the first of them, behind a slot that shares no resource with the pod
    assert _pair(ec, "Q", "Q:eq") == (True, 50, 1)


def test_filter_boundaries_flip():
    ec, res = _one_copy()
    m = res[0][0]

    def feas(pod, node):
        return bool(m[ec.pod(pod), ec.node(node)])
    for a, b, node in (("F1:pass", "F1:fail", "F1:r"), ("F1B:pass", "F1B:fail", "F1B:r"), ("F2:pass", "F2:fail", "F2:r"),
                       ("F2A:pass", "F2A:fail", "F2A:r"), ("F2n:pass", "F2n:fail", "F2:r")):
        assert feas(a, node) and not feas(b, node), (a, b)
    # Restricted without the affinity: the node stays feasible and the nomination flips
    assert _pair(ec, "F1n:pass", "F1:r") == (True, 100, 0) and _pair(ec, "F1n:fail", "F1:r") == (True, 0, -1)
    # the pod fits only because of the restore: its request exceeds Allocatable − Requested of the node as uploaded
    n = ec.view.nodes[ec.node("F2:r")]
    assert 3000 > int(n["allocatable"]["v"][rc.BCPU] - n["requested"]["v"][rc.BCPU]) == 1000
    # pod count
    assert feas("F3", "F3:at") and not feas("F3", "F3:over")
    # flags: allocate-once with an assigned pod, unschedulable with assigned pods, not available: no match on the node
    assert not feas("F4", "F4:flags") and feas("F4n", "F4:flags")
    r = oracle.rsv_restore(make_config(plugins=("Reservation",)), ec.view, ec.pod("F4n"), ec.node("F4:flags"))
    assert int(r["n_matched"]) == 0 and int(r["has_state"]) == 1   # the unschedulable one is restored as unmatched
    # affinity: a required affinity with no match is infeasible on reservation nodes and on plain nodes alike
    assert not m[ec.pod("NONE")].any() and not m[ec.pod("OUT32:aff")].any()
    assert m[ec.pod("NONEn"), ec.node("plain:0")] and m[ec.pod("NONEn"), ec.node("P:pref")]
    # owner classes outside 0..31 match nothing
    for pod in ("OUT32", "OUT40"):
        assert m[ec.pod(pod)].any() and res[0][4][ec.pod(pod)].max() == 0
        assert all(_pair(ec, pod, u["tag"])[2] == -1 for u in ec.units if u["rsv"])
    # an all-zero request passes fitsNode on a node with nothing left and is nominated
    assert _pair(ec, "ZR", "ZR:full") == (True, 0, 0)


def test_score_quotients():
    ec, res = _one_copy()
    rsv = res[0][4]
    p = ec.pod("S")
    for cap in rc.S_CAPS:
        for k in rc.S_STEPS:
            assert _pair(ec, "S", f"S:{cap}:{k}:at")[1] == k and _pair(ec, "S", f"S:{cap}:{k}:below")[1] == k - 1
            assert int(rsv[p, ec.node(f"S:{cap}:{k}:at")]) == k   # the class maximum is 100
        assert _pair(ec, "S", f"S:{cap}:over") == (True, 0, 0)
    assert min(rc.S_CAPS) * 1000 < 1 << 40 < rc.S_CAPS[1] * 1000 and rc.S_CAPS[2] * 1000 < 1 << 46 < rc.S_CAPS[3] * 1000
    assert [_pair(ec, "S2", t)[1] for t in ("S2:over", "S2:zero", "S2:three", "S2:one")] == [25, 50, 55, 30]


def test_quota_boundaries_flip():
    ec, res = _one_copy()
    any0 = res[0][0].any(axis=1)
    any1 = res[1][0].any(axis=1)

    def open_(tag):
        return bool(any0[ec.pod(tag)]), bool(any1[ec.pod(tag)])
    assert open_("Q0:pass") == (True, True) and open_("Q0:fail") == (False, False)
    assert open_("Q1:absent") == (True, True)
    assert open_("Q2:np:pass") == (True, True) and open_("Q2:np:fail") == (False, False)
    assert open_("Q2:preemptible") == (True, True)
    assert open_("Q3:pass") == (True, True) and open_("Q3:parent") == (True, False)
    assert open_("Q5:pass") == (True, True) and open_("Q5:last") == (True, False)
    assert open_("plain") == (True, True) and int(ec.view.pods["quota"][ec.pod("plain")]) == -1
    q = ec.view.quota_arr
    depth, a = 0, int(q["parent"][5])
    while a >= 0:
        depth, a = depth + 1, int(q["parent"][a])
    assert depth == rc.QUOTA_MAX_DEPTH


def test_host_rows_equal_the_oracle():
    ec, _ = _one_copy()
    idx = np.arange(ec.n_pods)
    for cfg in (shipped_profile(plugins=RSV), make_config(plugins=("Reservation",), weight_reservation=7)):
        got = rows_matrix5(cfg, ec.view, idx, ec.view.now_ns)
        ref = oracle.eval_matrix5(cfg, ec.view, idx, ec.view.now_ns)
        for g, r, name in zip(got, ref, ("mask", "fit", "la", "numa", "rsv", "top1")):
            np.testing.assert_array_equal(g, r, err_msg=name)


def test_row_eval_rsv_equals_rsv_pair_for_every_pair():
    ec, _ = _one_copy()
    cfg = make_config(plugins=("Reservation",))
    rows = engine.build_node_rows(cfg, ec.view)
    prow = engine.build_pod_rows(cfg, ec.view, np.arange(ec.n_pods))
    by_node = {}
    for r in ec.view.rsv_arr:
        by_node.setdefault(int(r["node"]), []).append(r)
    nominated = 0
    for p in range(ec.n_pods):
        for j, slots in by_node.items():
            f, _, _, _, raw, _, nom = engine.row_eval_rsv(cfg, rows[j:j + 1], np.array(slots), prow[p:p + 1], ec.view.now_ns)
            ok, oraw, onom = oracle.rsv_pair(cfg, ec.view, p, j)
            assert f == ok, (ec.pod_tags[p], ec.units[j]["tag"])
            if ok:
                assert (raw, nom) == (oraw, onom), (ec.pod_tags[p], ec.units[j]["tag"])
                nominated += nom >= 0
    assert nominated > 100


@pytest.mark.parametrize("n_rn", rc.GPU_SHAPES)
def test_shapes_keep_the_decisive_entries_decisive(n_rn):
    """The clusters of the GPU shape cases: trimmed to n_rn reservation nodes, the decisive units at the wanted ranks
    decide the preferred node of P, the maximum of M99 and the best key of an unowned pod."""
    for variant in (0, 1):
        at = rc.decisive_ranks(n_rn, variant)
        ec = rc.make_rsv_edge_cluster(-(-n_rn // 100) + 1, n_rn=n_rn, at=at)
        assert len(ec.rn) == n_rn and len(ec.view.nodes) - n_rn <= 400
        assert (np.diff(ec.rn) > 1).any() or n_rn == 1
        if at is None:
            continue
        assert tuple(ec.rank(t) for t in rc.DECISIVE) == at
        cfg = shipped_profile(plugins=RSV)
        idx = [ec.pod("P"), ec.pod("M99"), ec.pod("OUT32"), ec.pod("T")]
        m, _, _, _, rsv, top1 = oracle.eval_matrix5(cfg, ec.view, idx, ec.view.now_ns)
        assert rsv[0, ec.node("P:pref")] == 100 and (rsv[0] == 100).sum() == 1
        assert rsv[1, ec.node("M99:99")] == 100 and (rsv[1] == 100).sum() == 1
        assert engine.decode_top1(top1)[0][2] == ec.node("BK")
        ties = [k for k, u in enumerate(u for u in ec.units if u["rsv"]) if u["tag"].startswith("T:")]
        if len(ties) > 1:
            assert rsv[3, ec.rn[ties[0]]] == 100 and (rsv[3] == 100).sum() == 1   # the lowest of the tied nodes
        if n_rn >= 2047:   # tied minimal orders where lane order and rank order disagree (the 256-thread reduce, and
            # the 512-thread one of the resolve's fallback), in one wave, in other waves, in other blocks
            assert rc.lane_order_disagrees(ties, 256) and rc.lane_order_disagrees(ties, 512)
            assert {k // 64 for k in ties} > {ties[0] // 64} and {k // 256 for k in ties} > {ties[0] // 256}
            assert ties[1] // 64 == ties[0] // 64
        if n_rn == 2305:
            assert min(ties) < 2048 <= max(ties)


def test_queue_transitions_happen_in_the_reference_cycle():
    qc = rc.make_queue_cluster()
    v = qc.view
    out = {}
    for cp in (0, 1):
        cfg = shipped_profile(plugins=RSV_EQ, eq_check_parent_quota=cp)
        out[cp] = oracle.schedule2(cfg, v, np.arange(qc.n_pods), v.now_ns)
    nodes, scores, rsv, q = out[0]
    where = {t: (qc.units[nodes[p]]["tag"] if nodes[p] >= 0 else None) for p, t in enumerate(qc.pod_tags)}
    score = dict(zip(qc.pod_tags, scores.tolist()))
    wr = 5000
    for a, first in (("A", 2), ("A2", 15)):
        assert qc.pod(f"{a}:0") == first
        # the allocate-once reservation (the class's only order) is taken, then mx falls from 1000 to mraw: the next
        # pod's best reservation scores 100 · 60 / 60, not 100 · 60 / 1000
        assert where[f"{a}:0"] == f"{a}:once" and where[f"{a}:1"] == f"{a}:60"
        assert score[f"{a}:0"] >= 100 * wr and score[f"{a}:1"] >= 100 * wr
    # one triple inside a chunk of 16, one across its boundary
    assert qc.pod("A:0") // 16 == qc.pod("A:2") // 16 and qc.pod("A2:0") // 16 != qc.pod("A2:1") // 16
    assert [where[f"B:{i}"] for i in range(4)] == ["B:r"] * 3 + [None]
    r = rsv[[i for i, x in enumerate(v.rsv_arr) if x["node"] == qc.node("B:r")][0]]
    assert int(r["allocated"]["v"][rc.BCPU]) == int(r["allocatable"]["v"][rc.BCPU])
    assert [where[f"QL:{i}"] is not None for i in range(4)] == [True] * 3 + [False]
    assert int(q["used"]["v"][0, rc.BCPU]) == int(v.quota_arr["used_limit"]["v"][0, rc.BCPU])
    assert where["QP:2"] is not None and out[1][0][qc.pod("QP:2")] == -1
    assert int(out[1][3]["used"]["v"][2, rc.BCPU]) == int(v.quota_arr["used_limit"]["v"][2, rc.BCPU])
    # X holds the best base key for the unowned pod until the commits on it; then its group has another best
    assert where["free:0"] == "X" and where["X:big"] == "X" and where["free:1"] not in ("X", None)
    assert qc.rank("X") // 64 == qc.rank("A:once") // 64 == qc.rank("A:60") // 64
    assert where["cpu:0"].startswith("plain") and qc.pod("free:1") < qc.pod("cpu:0") < qc.pod("B:0")


@pytest.mark.parametrize("variant", ["order", "raw", "far"])
def test_wide_classes_count_their_scored_entries(variant):
    wc = rc.make_wide_class_cluster(variant)
    cfg = shipped_profile(plugins=RSV, weight_reservation=1 if variant == "far" else 5000)
    idx = np.arange(len(rc.WIDE_COUNTS))
    m, _, _, _, rsv, top1 = oracle.eval_matrix5(cfg, wc.view, idx, wc.view.now_ns)
    owners = np.zeros(len(wc.view.nodes), np.uint32)
    owners[wc.view.rsv_arr["node"]] = wc.view.rsv_arr["owner_classes"]
    last = wc.node(f"w:{len(wc.rn) - 1}")
    for i, want in enumerate(rc.WIDE_COUNTS):
        scored = m[i] & ((owners >> np.uint32(i)) & 1).astype(bool)
        assert int(scored.sum()) == want
        assert all(oracle.rsv_pair(cfg, wc.view, i, j)[2] == 0 for j in np.flatnonzero(scored)[::97])
        assert rsv[i, last] == 100 and (rsv[i] == 100).sum() == 1       # the last rank's entry decides
        assert (engine.decode_top1(top1)[0][i] == last) == (variant != "far")
    assert [int((wc.view.pods["rsv_owner_class"] == i).sum()) for i in range(4)] == [rc.WIDE_PODS[m] for m in rc.WIDE_COUNTS]
    if variant == "far":
        # no pod of the cycle is placed on the deciding node, and each one's chosen node carries a reservation score
        # that the deciding entry scales by 1000: every pod's score depends on it, whatever the chunk
        nodes, scores, _, _ = oracle.schedule2(cfg, wc.view, np.arange(wc.n_pods), wc.view.now_ns)
        assert (nodes >= 0).all() and (nodes != last).all()
        m, fit, la, _, rsv, _ = oracle.eval_matrix5(cfg, wc.view, np.arange(wc.n_pods), wc.view.now_ns)
        first = int(nodes[0])
        assert m[:, last].all() and (rsv[:, last] == 100).all() and 0 < rsv[0, first] < 10
        assert scores[0] == int(fit[0, first]) + int(la[0, first]) + int(rsv[0, first])


def test_fallback_cluster_is_past_the_group_flags():
    fv = rc.make_fallback_cluster()
    assert len(np.unique(fv.rsv_arr["node"])) == rc.FALLBACK_RN > 2048 * 64
    cfg = shipped_profile(plugins=RSV, place_chunk=4)
    nodes, scores, _, _ = oracle.schedule2(cfg, fv, np.arange(6), fv.now_ns)
    assert (nodes[:5] >= rc.FALLBACK_RN - 5).all() and 0 <= nodes[5]


def test_oracle_known_answers():
    """The two oracle corrections this cluster brought: an owner / affinity class outside 0..31 matches nothing (the
    shift by the class was undefined there), and a quota group may have KG_QUOTA_MAX_DEPTH ancestors, as kg_quota_set
    admits (the oracle's input check counted the group itself)."""
    with open(os.path.join(HERE, "golden", "rsv_edge_kat.json")) as f:
        doc = json.load(f)
    ec, res = _one_copy()
    for c in doc["class_match"]:
        pods = [dict(tag="k", req={rc.BCPU: 10}, cls=c["owner_class"], aff=c["affinity_class"], quota=-1, npre=False)]
        units = [rc._unit("n", [rc._rsv(tuple(c["reservation_classes"]), {rc.BCPU: 100}, {rc.BCPU: 40})])]
        v = rc.build_view(units, pods)
        ok, raw, nom = oracle.rsv_pair(make_config(plugins=("Reservation",)), v, 0, 0)
        assert [ok, raw, nom] == c["want"], c
    for c in doc["quota_chain"]:
        n = c["ancestors"] + 1
        q = np.zeros(n, dtype=nat.QUOTA)
        q["parent"] = np.arange(1, n + 1)
        q["parent"][-1] = -1
        pods = [dict(tag="k", req={rc.BCPU: 10}, cls=-1, aff=-1, quota=0, npre=False)]
        v = rc.build_view([rc._unit("n", [])], pods, q)
        cfg = shipped_profile(plugins=RSV_EQ, eq_check_parent_quota=1)
        if c["valid"]:
            assert oracle.eval_matrix5(cfg, v, [0], v.now_ns)[0].all()
        else:
            with pytest.raises(RuntimeError):
                oracle.eval_matrix5(cfg, v, [0], v.now_ns)
