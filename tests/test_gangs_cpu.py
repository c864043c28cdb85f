"""Gang-aware placement without a device: the ABI additions, kg_gang_plan's cuts and argument checks, and the rules
of kg_place_gangs (tests/gang_ref.run_model) on an 8-node hand case through the host driver."""
import numpy as np
import pytest

import gang_ref as gr
from koordinator_amd import _native as nat
from koordinator_amd import engine
from koordinator_amd.config import shipped_profile
from koordinator_amd.engine import EngineError

S = nat.GANG_STRICT


def test_abi_unchanged_and_symbols_present():
    L = nat.lib()
    assert L.kg_abi_version() == 13 and nat.ABI_VERSION == 13
    assert len(nat.STRUCT_IDS) == 19 and nat.SID_CYCLE_OUT == 18   # KG_SID_COUNT: no struct id added
    for name in ("kg_place_gangs", "kg_gang_plan"):
        assert name in nat.EXPORTED and getattr(L, name) is not None
    assert (nat.GANG_STRICT, nat.PLACE_GANG_RELEASE_WAITING) == (1, 1)
    assert (nat.GANG_ALLOWED, nat.GANG_WAITING, nat.GANG_REJECTED) == (0, 1, 2)


def _chunks(cut):
    """The chunk lengths a cut array describes."""
    ends = np.flatnonzero(cut) + 1
    assert len(cut) == 0 or ends[-1] == len(cut)
    return np.diff(np.concatenate([[0], ends])).tolist()


def test_plan_plain_batch_is_place_chunks():
    for P, chunk in ((0, 16), (1, 16), (16, 16), (40, 16), (40, 1), (40, 64), (130, 64)):
        want = [chunk] * (P // chunk) + ([P % chunk] if P % chunk else [])
        assert _chunks(engine.gang_plan(np.full(P, -1), np.zeros(0, np.uint8), chunk=chunk)) == want
    assert _chunks(engine.gang_plan(np.full(40, -1), [], chunk=0)) == [16, 16, 8]          # the default chunk
    assert _chunks(engine.gang_plan(np.full(2000, -1), [], chunk=5000)) == [1024, 976]      # clamped


def test_plan_contiguous_gangs():
    # plain 5, strict gang of 3, strict gang of 17 (straddles a chunk of 16), plain 4, a non-strict gang of 6 with them
    pg = np.array([-1] * 5 + [0] * 3 + [1] * 17 + [-1] * 4 + [2] * 6)
    flags = [S, S, 0]
    assert _chunks(engine.gang_plan(pg, flags, chunk=16)) == [5, 3, 16, 1, 10]
    assert _chunks(engine.gang_plan(pg, flags, chunk=64)) == [5, 3, 17, 10]
    assert _chunks(engine.gang_plan(pg, flags, chunk=1)) == [1] * len(pg)
    # the two strict gangs in one group: one run of 20, cut by the chunk size alone
    assert _chunks(engine.gang_plan(pg, flags, gang_group=[0, 0, 2], chunk=16)) == [5, 16, 4, 10]
    assert _chunks(engine.gang_plan(pg, flags, gang_group=[1, 1, 0], chunk=64)) == [5, 20, 10]


def test_plan_interleaved_gangs():
    pg = np.array([0, 1, 0, 1, -1, 0, 0, 2, -1, 1])
    assert _chunks(engine.gang_plan(pg, [S, S, 0], chunk=16)) == [1, 1, 1, 1, 1, 2, 2, 1]
    assert _chunks(engine.gang_plan(pg, [S, S, 0], gang_group=[0, 0, 2], chunk=16)) == [4, 1, 2, 2, 1]
    assert _chunks(engine.gang_plan(pg, [0, 0, 0], chunk=16)) == [10]   # no strict gang: no cut
    # every chunk is all pods of one strict group, or holds no strict pod
    cut = engine.gang_plan(pg, [S, S, 0], chunk=16)
    b = 0
    for n in _chunks(cut):
        kinds = {int(g) if g >= 0 and [S, S, 0][g] else -1 for g in pg[b:b + n]}
        assert len(kinds) == 1
        b += n


def _plan_status(pg, gg, gf, ng, chunk=16, cut=True, n_pods=None):
    pg = None if pg is None else np.ascontiguousarray(pg, np.int32)
    gg = None if gg is None else np.ascontiguousarray(gg, np.int32)
    gf = None if gf is None else np.ascontiguousarray(gf, np.uint8)
    P = (0 if pg is None else len(pg)) if n_pods is None else n_pods
    out = np.full(max(P, 1), 7, np.uint8)
    st = nat.lib().kg_gang_plan(nat.ptr(pg), P, nat.ptr(gg), nat.ptr(gf), ng, chunk, nat.ptr(out) if cut else None)
    return st, out


INVALID, RANGE = -1, -4   # KG_ERR_INVALID_ARG, KG_ERR_RANGE


def test_plan_validation():
    ok = ([0, 0, -1, 1], None, [S, 0], 2)
    assert _plan_status(*ok)[0] == 0
    assert _plan_status(None, None, [S], 1, n_pods=3)[0] == INVALID          # null pod_gang with pods
    assert _plan_status([0, 0], None, [S], 1, cut=False)[0] == INVALID       # null cut with pods
    assert _plan_status([0, 0], None, None, 1)[0] == INVALID                 # null gang_flags with gangs
    assert _plan_status([-1], None, None, -1)[0] == INVALID                  # n_gangs < 0
    assert _plan_status([-1], None, None, 0, n_pods=-1)[0] == INVALID        # n_pods < 0
    assert _plan_status([0], None, [2], 1)[0] == INVALID                     # unknown gang_flags bit
    assert _plan_status([0, 1], [0, 0], [S, 0], 2)[0] == INVALID             # a group that disagrees on strict
    assert _plan_status([0, 1, 2], [2, 1, 2], [S, 0, 0], 3)[0] == INVALID
    assert _plan_status([0, 2], None, [S, 0], 2)[0] == RANGE                 # pod_gang >= n_gangs
    assert _plan_status([-2], None, [S], 1)[0] == RANGE                      # pod_gang < -1
    assert _plan_status([0], None, None, 0)[0] == RANGE                      # any gang without gangs
    assert _plan_status([0, 1], [0, 2], [S, S], 2)[0] == RANGE               # gang_group >= n_gangs
    assert _plan_status([0, 1], [-1, 0], [S, S], 2)[0] == RANGE              # gang_group < 0
    for bad in (([0, 2], None, [S, 0], 2), ([0, 1], [0, 0], [S, 0], 2)):      # an error leaves cut untouched
        st, out = _plan_status(*bad)
        assert st != 0 and (out == 7).all()
    with pytest.raises(EngineError):
        engine.gang_plan([0, 3], [S])
    assert _plan_status(None, None, None, 0)[0] == 0                         # the empty batch


# ---- the hand case ---------------------------------------------------------------------------------------------------
def hand_case():
    """8 nodes of 4000m cpu under NodeResourcesFit (LeastAllocated): nodes 2 and 5 are empty, node 7 has 2000m free,
    the others 1000m.  Pods 0-2 ask 3000m each (a gang of 3), pod 3 is plain and asks 2000m."""
    cfg = shipped_profile(plugins=("NodeResourcesFit",))
    rows = np.zeros(8, nat.NODE_ROW)
    rows["flags"] = nat.NODE_VALID
    rows["alloc"][:, nat.RES_CPU] = 4000
    rows["alloc"][:, nat.RES_MEMORY] = 8 << 30
    rows["allowed_pods"] = 110
    used = np.array([3000, 3000, 0, 3000, 3000, 0, 3000, 2000])
    rows["requested"][:, nat.RES_CPU] = used
    rows["nonzero_requested"][:, 0] = used
    pods = np.zeros(4, nat.POD_ROW)
    for p, cpu in enumerate((3000, 3000, 3000, 2000)):
        pods["request"][p, nat.RES_CPU] = cpu
        pods["fit_score_request"][p, nat.RES_CPU] = cpu
        pods["nonzero_request"][p] = (cpu, 200 << 20)
    pods["request_present"] = 1 << nat.RES_CPU
    pods["flags"] = nat.POD_VALID | nat.POD_HAS_REQUEST
    pods["quota"] = pods["rsv_owner_class"] = pods["rsv_affinity_class"] = -1
    return cfg, rows, pods


def _hand(strict, **kw):
    cfg, rows, pods = hand_case()
    g = gr.gangs_of(4, [(0, 3)], strict=strict)
    d = gr.HostDriver(cfg, rows, pods)
    nodes, scores, verdicts, rolled = gr.run_model(d, 4, g["pod_gang"], g["gang_min"], g["gang_flags"], **kw)
    return nodes.tolist(), scores, verdicts.tolist(), rolled, d.rows, rows


def test_hand_case_strict_gang_hands_its_nodes_back():
    # members 0 and 1 take the empty nodes 2 and 5 (the lower index first), member 2 fits nowhere: the group is
    # rejected, both are released, and the plain pod takes node 2 — the best node again now that it is empty
    nodes, scores, verdicts, rolled, after, before = _hand(True)
    assert nodes == [-1, -1, -1, 2] and verdicts == [gr.REJECTED] and rolled == [0, 1]
    assert scores[:3].tolist() == [-1, -1, -1] and scores[3] >= 0
    want = before.copy()
    want["requested"][2, nat.RES_CPU] = want["nonzero_requested"][2, 0] = 2000
    want["nonzero_requested"][2, 1] = 200 << 20
    want["pod_count"][2] = 1
    assert after.tobytes() == want.tobytes()   # nodes 2 and 5 carry no trace of the gang


def test_hand_case_non_strict_gang_keeps_its_nodes():
    # the same queue with a non-strict gang: nothing is released, the plain pod finds 2000m only on node 7, and the
    # gang (2 of 3 placed) waits in Permit
    nodes, _, verdicts, rolled, after, _ = _hand(False)
    assert nodes == [2, 5, -1, 7] and verdicts == [gr.WAITING] and rolled == []
    assert after["pod_count"].tolist() == [0, 0, 1, 0, 0, 1, 0, 1]


def test_hand_case_release_waiting_and_allowed():
    nodes, _, verdicts, rolled, after, before = _hand(False, release_waiting=True)   # the Permit timeout
    assert nodes == [-1, -1, -1, 7] and verdicts == [gr.WAITING] and rolled == [0, 1]
    assert after[:7].tobytes() == before[:7].tobytes()
    cfg, rows, pods = hand_case()
    g = gr.gangs_of(4, [(0, 3)], gang_min=[2])   # two members are enough
    for strict in (0, S):
        n, _, v, _ = gr.run_model(gr.HostDriver(cfg, rows, pods), 4, g["pod_gang"], g["gang_min"], [strict])
        assert v.tolist() == ([gr.REJECTED] if strict else [gr.ALLOWED])


def test_host_quota_gate_matches_the_reserved_usage():
    """The host driver's ElasticQuota restatement: a strict gang whose k-th member fails the gate leaves `used` of the
    group and its ancestors where it started (on a 16-node cut of the GPU case)."""
    case, gangs, members, k = gr.quota_gang(gr.quota_case())
    rows = case["rows"][:16]
    last = members[k - 1] + 1
    d = gr.HostDriver(case["cfg"], rows, case["pods"][:last], case["quotas"])
    pg = gangs["pod_gang"][:last]
    only = np.where(pg >= 0)[0]
    d.pods = case["pods"][:last]
    nodes, _, verdicts, rolled = gr.run_model(_Only(d, set(only.tolist())), last, pg, gangs["gang_min"], gangs["gang_flags"])
    assert verdicts.tolist() == [gr.REJECTED] and rolled == members[:k - 1] and (nodes < 0).all()
    np.testing.assert_array_equal(d.quotas["used"]["v"], case["quotas"]["used"]["v"])
    np.testing.assert_array_equal(d.quotas["non_preemptible_used"]["v"], case["quotas"]["non_preemptible_used"]["v"])
    assert d.rows.tobytes() == rows.tobytes()


class _Only:
    """A driver that schedules the listed pods only (the others are unschedulable): keeps the host case small."""

    def __init__(self, driver, which):
        self.d, self.which = driver, which

    def cycle(self, p):
        return self.d.cycle(p) if p in self.which else (-1, -1)

    def release(self, p, node):
        self.d.release(p, node)
