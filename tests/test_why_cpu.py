"""kg_row_why (the host entry of the rejection reasons) against tests/why_ref.py, why_ref itself against the oracle at
object level, the unchanged ABI, and the reason strings.  No GPU."""
import ctypes

import numpy as np
import pytest

import why_cases as wc
import why_ref
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import shipped_profile

# kg_struct_size of every kg_struct_id at ABI 13, before kg_row_why / kg_diagnose (functions and macros only)
STRUCT_SIZES_ABI13 = [104, 1120, 208, 184, 632, 120, 16, 840, 160, 432, 992, 48, 1776, 240, 424, 320, 24, 64, 24]


def row_why_all(c, first_fail):
    """kg_row_why over every pair of a case → [P][N] uint32."""
    L = nat.lib()
    rows, pods = np.ascontiguousarray(c.ref_rows), np.ascontiguousarray(c.pods)
    out = np.zeros((len(pods), len(rows)), np.uint32)
    w = ctypes.c_uint32(0)
    cfg_p, wp = nat.ptr(c.cfg), ctypes.byref(w)
    flags = nat.DIAG_FIRST_FAIL if first_fail else 0
    nb, ns, pb, ps = rows.ctypes.data, rows.dtype.itemsize, pods.ctypes.data, pods.dtype.itemsize
    for i in range(len(pods)):
        for j in range(len(rows)):
            st = L.kg_row_why(cfg_p, nb + j * ns, pb + i * ps, int(c.now_ns), flags, wp)
            assert st == 0, (i, j, st)
            out[i, j] = w.value
    return out


@pytest.mark.parametrize("first_fail", [False, True])
@pytest.mark.parametrize("name", wc.NAMES)
def test_row_why_matches_reference(name, first_fail):
    c = wc.case(name)
    ref = wc.reference(name, first_fail)
    assert (ref != 0).any() and (ref == 0).any()
    np.testing.assert_array_equal(row_why_all(c, first_fail), ref)


def test_row_why_rejects_unknown_flags():
    c = wc.case("edited")
    w = ctypes.c_uint32(0)
    st = nat.lib().kg_row_why(nat.ptr(c.cfg), nat.ptr(c.ref_rows[:1]), nat.ptr(c.pods[:1]), int(c.now_ns), 0x2, ctypes.byref(w))
    assert st == -1   # KG_ERR_INVALID_ARG


def test_edited_reference_totals():
    """The `edited` reference is not vacuous: every reason occurs, exactly one pod fits nowhere, zero cpu requests fail
    on over-requested nodes and the nodes beyond the fp64 bounds carry reasons."""
    import cycle_cases as cc
    c = wc.case("edited")
    pods = c.pods.copy()   # the totals before the daemonset / no-request pod edits
    _, _, _, base_pods = wc.base("edited")
    for k in (wc.DAEMON_POD, wc.EMPTY_POD):
        pods[k] = base_pods[k]
    why = why_ref.why_ref(c.cfg, c.ref_rows, pods, c.now_ns)
    tot = wc.bit_totals(why)
    print("bit totals", tot, "feasible", int((why == 0).sum()))
    want = {0: 5_568, 2: 9_024, 3: 16_627, 16: 8_642, 17: 4_774, 18: 7_488, 19: 48, 20: 678, 23: 16_305}
    assert tot == want
    assert int((why == 0).sum()) == 50_976
    assert int(((why == 0).sum(axis=1) == 0).sum()) == 1
    zero_cpu = (pods["request"][:, nat.RES_CPU] == 0) & ((pods["flags"] & nat.POD_HAS_REQUEST) != 0)
    assert int(((why[zero_cpu] & nat.WHY_FIT_RES(nat.RES_CPU)) != 0).sum()) == 1_520
    assert int((why[:, cc.BIG] != 0).sum()) == 636   # the canonical-row path of k_why has reasons to report
    # the two remaining pod edits change their rows
    full = wc.reference("edited")
    assert not (full[wc.DAEMON_POD] & nat.WHY_LOADAWARE).any() and (why[wc.DAEMON_POD] & nat.WHY_LOADAWARE).any()
    assert not (full[wc.EMPTY_POD] >> nat.WHY_FIT_RES_SHIFT).any() and (why[wc.EMPTY_POD] >> nat.WHY_FIT_RES_SHIFT).any()


def test_scalar_and_numa_references_are_not_vacuous():
    tot = wc.bit_totals(wc.reference("scalar"))
    print("scalar", tot)
    assert (tot[16 + 8], tot[16 + 9], tot[16 + 10]) == (9_094, 3_996, 7_815)
    why = wc.reference("numa")
    numa = (why & nat.WHY_NUMA) != 0
    print("numa", int(numa.sum()), int((why == nat.WHY_NUMA).sum()))
    assert int(numa.sum()) == 2_401 and int((why == nat.WHY_NUMA).sum()) == 632
    assert not ((wc.case("numa").pods["flags"] & nat.POD_NUMA_CPU_BIND) != 0).any()


@pytest.mark.parametrize("name", wc.NAMES)
def test_reference_matches_oracle(name):
    """why_ref on the unedited rows against the oracle's object-level plugins: the Fit group ⇔ fit_filter, the LoadAware
    bit ⇔ la_filter, the NUMA bit ⇔ numa_eval, a zero word ⇔ the oracle's mask."""
    from oracle import oracle
    cfg, cl, rows, pods = wc.base(name)
    nb = wc.numa_bad() if name == "numa" else None
    why = why_ref.why_ref(cfg, rows, pods, cl.now_ns, numa_bad=nb)
    idx = np.arange(len(pods))
    if name == "numa":
        mask = oracle.eval_matrix3(cfg, cl, idx, cl.now_ns)[0]
    else:
        mask = oracle.eval_matrix(cfg, cl, idx, cl.now_ns)[0]
    np.testing.assert_array_equal(why == 0, mask)
    fit = np.zeros(why.shape, bool)
    la = np.zeros(why.shape, bool)
    for i in range(len(pods)):
        for j in range(len(rows)):
            fit[i, j] = oracle.fit_filter(cl, i, j) != 0
            la[i, j] = oracle.la_filter(cfg, cl, i, j, cl.now_ns) != 0
    assert fit.any() and la.any()
    np.testing.assert_array_equal((why & nat.WHY_FIT_MASK) != 0, fit)
    np.testing.assert_array_equal((why & nat.WHY_LOADAWARE) != 0, la)
    if name == "numa":
        skip = (pods["flags"] & nat.POD_NUMA_SKIP) != 0
        np.testing.assert_array_equal(((why & nat.WHY_NUMA) != 0)[~skip], nb[~skip])


def test_first_fail_keeps_one_group():
    for name in wc.NAMES:
        full, first = wc.reference(name), wc.reference(name, True)
        np.testing.assert_array_equal(first != 0, full != 0)
        groups = [first & g != 0 for g in (nat.WHY_ABSENT, nat.WHY_ELIG, nat.WHY_FIT_MASK, nat.WHY_LOADAWARE, nat.WHY_NUMA)]
        assert (np.sum(groups, axis=0) <= 1).all()
        assert ((first & ~full) == 0).all()


def test_abi_is_unchanged():
    L = nat.lib()
    for fn in ("kg_row_why", "kg_diagnose"):
        assert fn in nat.EXPORTED and hasattr(L, fn)
    assert L.kg_abi_version() == 13 and nat.ABI_VERSION == 13
    assert len(nat.STRUCT_IDS) == len(STRUCT_SIZES_ABI13)   # KG_SID_COUNT: no new ABI struct
    assert [L.kg_struct_size(sid) for sid in range(len(STRUCT_SIZES_ABI13) + 1)] == STRUCT_SIZES_ABI13 + [-1]
    assert (nat.WHY_SLOTS, nat.WHY_SLOT_REJECTED, nat.WHY_SLOT_FEASIBLE, nat.DIAG_MAX_PODS) == (32, 30, 31, 256)
    assert nat.WHY_FIT_RES(0) == 1 << 16 and nat.WHY_FIT_RES(nat.NUM_RES - 1) == 1 << 27


def test_debug_dump_logs_the_reason_histogram(caplog):
    import logging
    from koordinator_amd import debug
    cfg = shipped_profile()
    res = {"mask": np.array([[0], [0b101]], np.uint64), "scores": np.zeros((2, 64, 2), np.uint8)}
    asked = []

    def reasons(p):
        asked.append(p)
        return "3 Too many pods"

    with caplog.at_level(logging.INFO, logger="koordinator_amd.debug"):
        tables = debug.dump_eval(cfg, res, 3, 2, reasons=reasons)
    assert len(tables) == 2 and asked == [0]   # only the pod without a feasible node
    assert "0/3 nodes are available for Pod: pod-0: 3 Too many pods" in caplog.text


def test_why_names():
    cfg = shipped_profile(extended_resources=synth.SCALAR_NAMES)
    word = nat.WHY_FIT_PODS | nat.WHY_FIT_RES(nat.RES_CPU) | nat.WHY_FIT_RES(nat.RES_BATCH_MEMORY) | \
        nat.WHY_FIT_RES(nat.RES_EXT0) | nat.WHY_FIT_RES(nat.RES_EXT2) | nat.WHY_LOADAWARE
    assert engine.why_names(cfg, word) == [
        "Too many pods", "Insufficient cpu", "Insufficient kubernetes.io/batch-memory", "Insufficient nvidia.com/gpu",
        "Insufficient koordinator.sh/rdma", "node(s) usage exceed threshold"]
    assert engine.why_names(cfg, 0) == []
    assert engine.why_names(cfg, nat.WHY_ELIG | nat.WHY_NUMA) == [
        "node(s) didn't match the pod's eligibility class", "node(s) NUMA Topology affinity error"]
    counts = np.zeros(nat.WHY_SLOTS, np.uint32)
    counts[2], counts[16], counts[nat.WHY_SLOT_REJECTED] = 97, 312, 400
    assert engine.why_histogram(cfg, counts) == "97 Too many pods, 312 Insufficient cpu"
