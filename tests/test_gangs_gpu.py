"""kg_place_gangs on the device against the rules of tests/gang_ref.py run over a twin engine (merged entry points
only, one pod at a time).  gang_ref.compare checks every case four ways: out_node / out_score / verdicts, the
downloaded rows byte for byte, the downloaded quota groups, and a second batch's eval against a fresh engine loaded
from the model's final state.  N = 2100 nodes (two full tiles and a ragged third), batches of 64-128 pods."""
import numpy as np
import pytest

import gang_ref as gr
import unreserve_cases as uc
from koordinator_amd import _native as nat
from koordinator_amd.engine import EngineError

pytestmark = pytest.mark.gpu

NOW = gr.NOW


def _case(unfit=(), most=False):
    base = gr.fit_la_case(most)
    return dict(base, pods=gr.unfit(base["pods"], unfit)) if len(unfit) else base


@pytest.mark.parametrize("size", [1, 3, 16, 17, 40])
def test_shapes(size):
    """Two strict gangs of `size` pods behind 5 plain pods (place_chunk = 16): the first completes, the second loses
    its middle member and is rolled back."""
    a, b = (5, 5 + size), (5 + size + 2, 5 + 2 * size + 2)
    fail = b[0] + size // 2
    got, ref = gr.compare(_case([fail]), gr.gangs_of(128, [a, b]))
    assert got["verdicts"].tolist() == [gr.ALLOWED, gr.REJECTED]
    assert (got["nodes"][a[0]:a[1]] >= 0).all() and (got["nodes"][b[0]:b[1]] == -1).all()
    assert ref[3] == list(range(b[0], fail))


@pytest.mark.parametrize("pos", ["first", "middle", "last"])
def test_failure_position(pos):
    """A strict gang of 17 pods from pod 10 on (it straddles the chunks 0-15 and 16-31) failing at its first, a middle
    and its last member."""
    begin, end = 10, 27
    fail = {"first": begin, "middle": 21, "last": end - 1}[pos]
    got, ref = gr.compare(_case([fail]), gr.gangs_of(128, [(begin, end)]))
    assert got["verdicts"].tolist() == [gr.REJECTED] and (got["nodes"][begin:end] == -1).all()
    assert ref[3] == list(range(begin, fail))
    assert got["generations"][1] > got["generations"][0]


def test_scarce_resource_goes_to_the_pods_behind_the_gang():
    s = gr.scarce_summary()
    members = list(range(8, 16))
    took = len(s["rolled"])                               # the gpu nodes these pods fit on: at most six, then none
    assert s["verdicts"].tolist() == [gr.REJECTED] and 3 <= took <= 6 and s["rolled"].tolist() == members[:took]
    later = [p for p in s["gpu_pods"].tolist() if p >= 16]
    assert (s["nodes"][later] >= 0).sum() == took         # they take the nodes the gang gave back
    assert (s["nodes"][later] != s["plain"][later]).any() and (s["plain"][later] == -1).all()
    assert (s["plain"][members[:took]] >= 0).all()        # plain place leaves the partial gang on the snapshot


def test_several_members_on_one_node():
    """MostAllocated piles the members of a gang on few nodes: the rollback releases one node several times."""
    members = list(range(6, 30))
    case = _case([members[-1]], most=True)
    with gr.make_engine(case["cfg"], case["rows"]) as eng:
        eng.set_pods(case["pods"])
        plain = eng.place(NOW)[0]
    placed = plain[members[:-1]]
    assert (placed >= 0).all() and np.bincount(placed).max() >= 3, "the case needs a node with several members"
    got, ref = gr.compare(case, gr.gangs_of(128, [members]))
    assert got["verdicts"].tolist() == [gr.REJECTED] and ref[3] == members[:-1]


def test_non_contiguous_gang():
    members = [3, 9, 10, 25, 40, 41, 77, 100]
    got, ref = gr.compare(_case([41]), gr.gangs_of(128, [members]))
    assert got["verdicts"].tolist() == [gr.REJECTED] and ref[3] == members[:5]
    assert (got["nodes"][members] == -1).all()            # 77 and 100 were never scheduled
    others = np.setdiff1d(np.arange(128), members)
    assert (got["nodes"][others] >= 0).sum() > 100


def test_group_of_two_gangs():
    """Gangs 0 and 1 form one group, gang 2 is alone: gang 1 fails, so gang 0's pods are rolled back too."""
    spans = [(4, 12), (20, 30), (40, 50)]
    got, ref = gr.compare(_case([26]), gr.gangs_of(128, spans, groups=[0, 0, 2]))
    assert got["verdicts"].tolist() == [gr.REJECTED, gr.REJECTED, gr.ALLOWED]
    assert ref[3] == list(range(4, 12)) + list(range(20, 26))
    assert (got["nodes"][4:12] == -1).all() and (got["nodes"][20:30] == -1).all() and (got["nodes"][40:50] >= 0).all()


def test_non_strict_failing_gang_releases_nothing():
    got, ref = gr.compare(_case([15]), gr.gangs_of(128, [(8, 24)], strict=False))
    assert got["verdicts"].tolist() == [gr.WAITING] and ref[3] == []
    assert got["nodes"][15] == -1 and (np.delete(got["nodes"][8:24], 7) >= 0).all()


@pytest.mark.parametrize("release", [False, True])
def test_waiting_groups(release):
    """gang_min above the members of the batch: strict gang 0 and non-strict gang 1 wait, gang 2 is allowed; the
    release rolls both waiting groups back and keeps their verdict."""
    gangs = gr.gangs_of(128, [(2, 12), (30, 36), (50, 70)], strict=[gr.STRICT, 0, gr.STRICT], gang_min=[11, 9, 20])
    got, ref = gr.compare(_case(), gangs, release_waiting=release)
    assert got["verdicts"].tolist() == [gr.WAITING, gr.WAITING, gr.ALLOWED]
    assert ref[3] == (list(range(2, 12)) + list(range(30, 36)) if release else [])
    assert ((got["nodes"][2:12] >= 0).all() and (got["nodes"][30:36] >= 0).all()) != release
    assert (got["nodes"][50:70] >= 0).all()


def test_quota_gate_rejects_the_gang():
    s = gr.quota_summary()
    members, k = s["members"].tolist(), int(s["k"])
    assert s["verdicts"].tolist() == [gr.REJECTED] and s["rolled"].tolist() == members[:k - 1]
    assert (s["nodes"][members] == -1).all()
    # the leaf and its ancestors: no batch-cpu of the gang is left in `used`
    leaf = int(gr.quota_case()["pods"]["quota"][members[0]])
    others = [p for p in np.flatnonzero(s["nodes"] >= 0).tolist()]
    pods = gr.quota_case()["pods"]
    g = leaf
    while g >= 0:
        below = [p for p in others if _under(s["quotas0"], int(pods["quota"][p]), g)]
        want = int(s["quotas0"]["used"]["v"][g, nat.RES_BATCH_CPU]) + sum(int(pods["numa_request"][p, nat.RES_BATCH_CPU]) for p in below)
        assert int(s["quotas"]["used"]["v"][g, nat.RES_BATCH_CPU]) == want, g
        g = int(s["quotas0"]["parent"][g])


def _under(quotas, g, top):
    while g >= 0:
        if g == top:
            return True
        g = int(quotas["parent"][g])
    return False


def test_eligibility_classes_on_a_gang():
    """The gang's members may only run on class 1's nodes (every third node), a few plain pods on class 2's (the ragged
    tile); the member after the last eligible capacity... fails by construction (unfit)."""
    base = gr.fit_la_case()
    elig = np.zeros((2, gr.N), bool)
    elig[0, ::3] = True
    elig[1, 2048:] = True
    pods = gr.unfit(base["pods"], [31])
    members = list(range(12, 36))
    pods["elig_class"][members] = 1
    pods["elig_class"][[40, 41, 60]] = 2
    case = dict(base, pods=pods, elig=elig)
    with gr.make_engine(case["cfg"], case["rows"], elig=elig) as eng:
        eng.set_pods(pods)
        plain = eng.place(NOW)[0]
    assert (plain[members[:19]] % 3 == 0).all() and (plain[[40, 41, 60]] >= 2048).all()
    got, ref = gr.compare(case, gr.gangs_of(128, [members]))
    assert got["verdicts"].tolist() == [gr.REJECTED] and ref[3] == members[:19]


def test_forms_give_the_same_answer():
    """place_chunk 1 / 16 / 64 and the forced placement pipeline: a gang batch takes the sequential loop with
    kg_gang_plan's cuts either way."""
    case = _case([26, 70])
    gangs = gr.gangs_of(128, [(4, 12), (20, 30), (40, 57), (60, 75)], strict=[gr.STRICT, gr.STRICT, 0, gr.STRICT],
                        groups=[0, 0, 2, 3])
    got, _ = gr.compare(case, gangs)
    for kw in (dict(place_chunk=1), dict(place_chunk=64), dict(forms=nat.FORM_PLACE_PIPELINE),
               dict(place_chunk=64, forms=nat.FORM_PLACE_PIPELINE)):
        other = gr.engine_run(case, gangs, **kw)
        for k in ("nodes", "scores", "verdicts"):
            np.testing.assert_array_equal(other[k], got[k], err_msg=f"{kw}: {k}")
        assert other["rows"].tobytes() == got["rows"].tobytes(), kw


@pytest.mark.parametrize("how", ["no_gangs", "all_minus_one"])
def test_without_gang_members_it_is_place(how):
    case = _case([7, 50])
    gangs = dict(pod_gang=np.full(128, -1, np.int32), gang_min=np.zeros(0, np.int32), gang_flags=np.zeros(0, np.uint8)) \
        if how == "no_gangs" else dict(pod_gang=np.full(128, -1, np.int32), gang_min=np.array([0, 3], np.int32),
                                       gang_flags=np.array([gr.STRICT, 0], np.uint8))
    got = gr.engine_run(case, gangs)
    with gr.make_engine(case["cfg"], case["rows"]) as twin:
        twin.set_pods(case["pods"])
        g0 = twin.generation()
        nodes, scores = twin.place(NOW)
        np.testing.assert_array_equal(got["nodes"], nodes)
        np.testing.assert_array_equal(got["scores"], scores)
        assert got["rows"].tobytes() == twin.download().tobytes()
        assert got["generations"][1] - got["generations"][0] == twin.generation() - g0
    assert got["verdicts"].tolist() == ([] if how == "no_gangs" else [gr.ALLOWED, gr.WAITING])
    assert got["placed"] == int((nodes >= 0).sum())


def _refused(eng, pods, code):
    eng.set_pods(pods)
    rows0, g0, placed0 = eng.download(), eng.generation(), eng.counters()["placed"]
    g = gr.gangs_of(len(pods), [(0, 4)])
    with pytest.raises(EngineError) as e:
        eng.place_gangs(NOW, g["pod_gang"], g["gang_min"], g["gang_flags"])
    assert f"status {code}:" in str(e.value)
    assert eng.download().tobytes() == rows0.tobytes() and eng.generation() == g0
    assert eng.counters()["placed"] == placed0


def test_refusals_change_nothing():
    cfg, rows, first, _ = uc.numa_cluster()
    with uc.make_engine(cfg, rows) as eng:
        _refused(eng, first, -3)                                   # KG_ERR_UNSUPPORTED: NodeNUMAResource enabled
    cfg, rows, first, _, rsv, quotas = uc.rsv_quota_cluster()
    with uc.make_engine(cfg, rows, rsv, quotas) as eng:
        rsv0 = eng.download_reservations()
        _refused(eng, first, -3)                                   # reservation slots loaded
        np.testing.assert_array_equal(rsv0, eng.download_reservations())
    case = gr.fit_la_case()
    with gr.make_engine(case["cfg"], case["rows"]) as eng:         # argument errors on a live engine
        eng.set_pods(case["pods"])
        rows0, g0 = eng.download(), eng.generation()
        pg = np.full(128, -1, np.int32)
        pg[:4] = 0
        for bad, code in ((dict(pod_gang=pg, gang_min=[-1], gang_flags=[1]), -1),
                          (dict(pod_gang=pg, gang_min=[4], gang_flags=[2]), -1),
                          (dict(pod_gang=np.where(pg == 0, 1, pg), gang_min=[4], gang_flags=[1]), -4),
                          (dict(pod_gang=pg, gang_min=[4], gang_flags=[1], gang_group=[1]), -4)):
            with pytest.raises(EngineError) as e:
                eng.place_gangs(NOW, **bad)
            assert f"status {code}:" in str(e.value), bad
        assert eng.download().tobytes() == rows0.tobytes() and eng.generation() == g0
        eng.set_shard(0, 1024)
        with pytest.raises(EngineError) as e:
            eng.place_gangs(NOW, pg, [4], [1])
        assert "status -5:" in str(e.value)                        # KG_ERR_STATE: a shard is set
