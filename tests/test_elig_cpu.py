"""Node eligibility classes without a GPU: the ABI (three new exports, unchanged struct sizes, elig_class at _pad2's old
offset, ABI 13, kg_build_pod_rows writes 0), the Python packing, and the preconditions of tests/test_elig_gpu.py
proved from the oracle, so that the GPU tests cannot pass vacuously (tests/elig_cases.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import elig_cases as ec
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import shipped_profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "koord_gpu.h")


def test_library_exports_the_three_functions():
    L = nat.lib()
    for name in ("kg_elig_set", "kg_elig_update", "kg_pods_restricted_count"):
        assert hasattr(L, name), name
        assert name in nat.EXPORTED


# sizeof() of every ABI struct before the eligibility classes, by kg_struct_id (ABI 13): none may change
SIZES_ABI13 = {0: 104, 1: 1120, 2: 208, 3: 184, 4: 632, 5: 120, 6: 16, 7: 840, 9: 432, 10: 992, 12: 1776, 13: 240,
               14: 424, 15: 320, 16: 24, 17: 64, 18: 24}


def test_struct_sizes_unchanged_and_field_offset():
    L = nat.lib()
    L.kg_struct_size.restype = ctypes.c_int64
    for sid, dt in enumerate(nat.STRUCT_IDS):
        if dt is not None:
            assert int(L.kg_struct_size(sid)) == dt.itemsize == SIZES_ABI13[sid], sid
    sid = nat.STRUCT_IDS.index(nat.POD_ROW)
    assert int(L.kg_struct_size(sid)) == nat.POD_ROW.itemsize == 432
    # the field sits where _pad2 sat: after quota, before la_estimate_x, in the dtype and in the header
    f = nat.POD_ROW.fields
    assert "_pad2" not in f and f["elig_class"][0] == np.dtype("<i4")
    assert f["elig_class"][1] == f["quota"][1] + 4 == f["la_estimate_x"][1] - 4 == 348   # _pad2's offset
    text = open(HEADER).read()
    body = text[text.index("typedef struct kg_pod_row {"):text.index("} kg_pod_row;")]
    names = re.findall(r"^\s*(?:u?int\d+_t)\s+(\w+)", body, flags=re.M)
    assert "_pad2" not in names
    assert names[names.index("quota") + 1] == "elig_class" and names[names.index("elig_class") + 1] == "la_estimate_x"
    assert re.search(r"^\s*int32_t\s+elig_class;", body, flags=re.M)


def test_header_still_says_abi_13():
    text = open(HEADER).read()
    assert re.search(r"#define\s+KG_ABI_VERSION\s+13\b", text)
    assert nat.ABI_VERSION == 13 and int(nat.lib().kg_abi_version()) == 13
    for name in ("kg_elig_set", "kg_elig_update", "kg_pods_restricted_count"):
        assert re.search(r"\b%s\(" % name, text), name
    # both non-checks are stated in the header
    assert "kg_commit(pod, node) does not check eligibility" in text
    assert "ignore kg_pod_row.elig_class" in text


def test_build_pod_rows_writes_zero():
    cl = synth.make_cluster(64, 16, seed=5)
    cfg = shipped_profile()
    idx = np.arange(16, dtype=np.int32)
    out = np.zeros(16, dtype=nat.POD_ROW)
    out["elig_class"] = 7   # whatever the buffer held
    engine._check(nat.lib().kg_build_pod_rows(nat.ptr(cfg), ctypes.byref(cl.c_view), nat.ptr(idx), 16, nat.ptr(out)))
    assert not out["elig_class"].any()


def test_row_eval_ignores_the_class():
    cl = synth.make_cluster(64, 4, seed=5)
    cfg = shipped_profile()
    nodes = engine.build_node_rows(cfg, cl)
    pods = engine.build_pod_rows(cfg, cl, np.arange(4))
    other = pods.copy()
    other["elig_class"] = 3
    for j in range(0, 64, 7):
        for p in range(4):
            assert engine.row_eval(cfg, nodes[j:j + 1], pods[p:p + 1], cl.now_ns) == \
                engine.row_eval(cfg, nodes[j:j + 1], other[p:p + 1], cl.now_ns)


def test_pack_eligibility():
    masks = ec.class_masks()
    packed = engine.pack_eligibility(masks)
    assert packed.shape == (len(ec.CLASSES), 40) and packed.dtype == np.uint64
    np.testing.assert_array_equal(engine.unpack_mask(packed, ec.N), masks)
    assert not (packed[:, -1] >> np.uint64(ec.N % 64)).any()   # pad bits 0


def test_classes_are_what_the_names_say():
    m = ec.class_masks()
    cls = dict(zip(ec.CLASSES, m))
    assert 0.45 < cls["half"].mean() < 0.55
    assert np.flatnonzero(cls["pool"]).tolist() == list(range(1024, 2048))
    assert np.flatnonzero(cls["tailword"]).tolist() == [2496, 2497, 2498, 2499]
    assert np.flatnonzero(cls["edges"]).tolist() == [0, 63, 64, 1023, 1024, ec.N - 1]
    assert cls["one"].sum() == 1 and not cls["none"].any() and cls["all"].all()
    np.testing.assert_array_equal(m, ec.class_masks())   # fixed by seed


@pytest.mark.parametrize("name", ["mixed", "wide", "slow", "lax", "exact"])
def test_mixed_batch_preconditions(name):
    c = ec.case(name)
    assert (c.P, c.N) == (ec.P, ec.N)
    c.check_preconditions()
    if name == "wide":
        assert (c.spill & c.restricted).any() and (c.spill & ~c.restricted).any() and (~c.spill & c.restricted).any()
    if name == "slow":   # slow nodes on both sides of a class, feasible for some restricted pod on each side
        slow = np.array(ec.SLOW_NODES)
        assert (c.node_rows["alloc"][slow, nat.RES_MEMORY] > (1 << 42)).all()
        half = c.of_class("half")
        free = c.free[0][half][:, slow]
        inside = c.masks[ec.CLS["half"] - 1][slow]
        assert free[:, inside].any() and free[:, ~inside].any()


def test_twin_preconditions():
    c, view = ec.twin()
    c.check_preconditions()
    assert len(c.masks) <= 5
    # the restricted pods of the twin have a non-zero request of their class's resource, the others none
    rows = engine.build_pod_rows(c.cfg, view, c.idx)
    for p in range(c.P):
        k = int(c.elig_class[p])
        ext = rows["request"][p, nat.RES_EXT0:nat.RES_EXT0 + 5]
        assert ext.tolist() == [1 if k and r == k - 1 else 0 for r in range(5)]
    # unweighted: no score reads the named scalars
    assert not c.cfg["fit_resource_weight"][nat.RES_EXT0:].any() and not c.cfg["la_resource_weight"][nat.RES_EXT0:].any()
    # the twin's oracle mask is the restricted mask
    from oracle import oracle
    m, f, l = oracle.eval_matrix(c.cfg, view, c.idx, c.cl.now_ns)
    np.testing.assert_array_equal(m, c.matrix[0])
    np.testing.assert_array_equal(f, c.matrix[1])
    np.testing.assert_array_equal(l, c.matrix[2])


def test_rsv_case_preconditions():
    c = ec.rsv_case()
    (m, f, l, plane, top1), moved = ec.rsv_reference(c)
    m0 = c.free5[0]
    rn = np.unique(c.cl.rsv_arr["node"])
    r = np.flatnonzero(c.restricted)
    assert 0.25 <= c.restricted.mean() <= 0.75
    # reservation nodes both eligible and ineligible for restricted pods, feasible on each side
    elig = np.stack([c.masks[c.elig_class[p] - 1] for p in r])
    assert (m0[r][:, rn] & elig[:, rn]).any() and (m0[r][:, rn] & ~elig[:, rn]).any()
    assert moved >= 1, "no restricted pod whose preferred reservation node is ineligible"
    # some restricted pod's restricted best node is a reservation node, and the restriction changes some top1
    node = (np.uint64(0xFFFFFFFF) - (top1 & np.uint64(0xFFFFFFFF))).astype(np.int64)
    assert ((top1[r] != 0) & np.isin(node[r], rn)).any()
    assert (top1[r] != c.free5[5][r]).any()
    # the unrestricted pods' re-reduction is the oracle's own
    u = np.flatnonzero(~c.restricted)
    np.testing.assert_array_equal(top1[u], c.free5[5][u])
    np.testing.assert_array_equal(plane[u], c.free5[4][u])
