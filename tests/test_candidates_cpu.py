"""kg_candidates / kg_candidates_merge without a GPU: the boundary (macros, symbols, ABI 13 unchanged), the NumPy
reference tests/cand_ref.py on a hand-written example, and the host merge against that reference."""
import os
import re

import numpy as np
import pytest

import cand_ref as cr
import cycle_cases as cc
from koordinator_amd import _native as nat
from koordinator_amd import engine

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "koord_gpu.h")
STRUCT_SIZES_ABI13 = [104, 1120, 208, 184, 632, 120, 16, 840, 160, 432, 992, 48, 1776, 240, 424, 320, 24, 64, 24]
ERR_INVALID_ARG = -1


def key(total, node):
    return ((total + 1) << 32) | (0xFFFFFFFF - node)


def test_boundary_is_abi_13():
    text = open(HEADER).read()
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (KG_\w+) (\d+)\b", text)}
    assert consts["KG_CAND_MAX_K"] == nat.CAND_MAX_K == 64
    assert consts["KG_CAND_MAX_PODS"] == nat.CAND_MAX_PODS == 256
    L = nat.lib()
    for fn in ("kg_candidates", "kg_candidates_merge"):
        assert fn in nat.EXPORTED and getattr(L, fn) is not None
    assert consts["KG_ABI_VERSION"] == 13 and L.kg_abi_version() == 13 and nat.ABI_VERSION == 13
    assert len(nat.STRUCT_IDS) == len(STRUCT_SIZES_ABI13)   # KG_SID_COUNT: no new ABI struct
    assert [L.kg_struct_size(sid) for sid in range(len(STRUCT_SIZES_ABI13) + 1)] == STRUCT_SIZES_ABI13 + [-1]
    assert nat.SID_CYCLE_OUT == len(STRUCT_SIZES_ABI13) - 1


def test_cand_ref_by_hand():
    #            node: 0   1   2   3   4   5   6   7   8   9
    tot = np.array([[5, -1, 9, 5, 9, 0, -1, 5, 9, 2],      # three 9s, three 5s: ties to the lower node
                    [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1],
                    [-1, 7, -1, -1, -1, -1, -1, 7, -1, -1]])
    fit = np.arange(30).reshape(3, 10)
    la = 100 - fit
    keys, scores, nf = cr.cand_ref(tot, 4, fit, la)
    np.testing.assert_array_equal(nf, [8, 0, 2])
    want = np.array([[key(9, 2), key(9, 4), key(9, 8), key(5, 0)], [0, 0, 0, 0], [key(7, 1), key(7, 7), 0, 0]], np.uint64)
    np.testing.assert_array_equal(keys, want)
    np.testing.assert_array_equal(scores[0, :, 0], [2, 4, 8, 0])
    np.testing.assert_array_equal(scores[0, :, 1], [98, 96, 92, 100])
    np.testing.assert_array_equal(scores[2, :, 0], [21, 27, 0, 0])
    assert not scores[1].any() and not scores[..., 2:].any() and not scores[2, 2:].any()
    assert cr.tie_at_cut(tot, 4) and cr.tie_at_cut(tot, 1) and not cr.tie_at_cut(tot, 3)   # 5 | 5, 9 | 9, 9 | 5
    # k past the node count: zero padding; a node offset: the keys carry global indices
    keys12, scores12, _ = cr.cand_ref(tot, 12, fit)
    np.testing.assert_array_equal(keys12[:, :4], want)
    assert not keys12[0, 8:].any() and keys12[0, 7] == key(0, 5) and not scores12[0, 8:].any()
    np.testing.assert_array_equal(cr.cand_ref(tot, 4, node0=1024)[0][2], [key(7, 1025), key(7, 1031), 0, 0])
    node, total = engine.decode_top1(keys)
    np.testing.assert_array_equal(node[0], [2, 4, 8, 0])
    np.testing.assert_array_equal(total[2], [7, 7, -1, -1])


def merge(keys, scores, n_lists, n, k, prefill=0xAB):
    """(status, out_keys, out_scores) of kg_candidates_merge over prefilled outputs."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out_k = np.full((max(n, 1), max(k, 1)), prefill * 0x0101010101010101, dtype=np.uint64)
    out_s = None if scores is None else np.full((max(n, 1), max(k, 1), 4), prefill, dtype=np.uint8)
    sc = None if scores is None else np.ascontiguousarray(scores, dtype=np.uint8)
    st = nat.lib().kg_candidates_merge(nat.ptr(keys), nat.ptr(sc), n_lists, n, k, nat.ptr(out_k), nat.ptr(out_s))
    return st, out_k, out_s


def split_lists(tot, fit, la, k, bounds):
    parts = [cr.cand_ref(tot[:, lo:hi], k, fit[:, lo:hi], la[:, lo:hi], node0=lo) for lo, hi in bounds]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


@pytest.mark.parametrize("n_lists", [2, 8])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_merge_matches_reference(n_lists, k):
    rng = np.random.default_rng(100 * n_lists + k)
    P, N = 7, 200
    tot = rng.integers(-1, 6, size=(P, N))      # few distinct totals: ties within and across the lists
    tot[1] = -1                                  # every list of this pod is empty
    tot[2, 3:] = -1                              # lists shorter than k
    tot[3, :] = 4                                # one total everywhere: the node index decides alone
    fit, la = rng.integers(0, 101, size=(2, P, N))
    edges = np.linspace(0, N, n_lists + 1).astype(int)
    bounds = list(zip(edges[:-1], edges[1:]))
    keys, scores = split_lists(tot, fit, la, k, bounds)
    want_k, want_s, _ = cr.cand_ref(tot, k, fit, la)
    st, out_k, out_s = merge(keys, scores, n_lists, P, k)
    assert st == 0
    np.testing.assert_array_equal(out_k, want_k)
    np.testing.assert_array_equal(out_s, want_s)
    st, out_k, out_s = merge(keys, None, n_lists, P, k)     # scores = NULL
    assert st == 0 and out_s is None
    np.testing.assert_array_equal(out_k, want_k)
    # the Python wrapper, n_feasible summed over the disjoint shards
    res = engine.merge_candidates([{"keys": keys[i], "scores": scores[i],
                                    "n_feasible": (tot[:, lo:hi] >= 0).sum(axis=1)} for i, (lo, hi) in enumerate(bounds)])
    np.testing.assert_array_equal(res["keys"], want_k)
    np.testing.assert_array_equal(res["scores"], want_s)
    np.testing.assert_array_equal(res["n_feasible"], (tot >= 0).sum(axis=1))
    np.testing.assert_array_equal(res["nodes"][1], np.full(k, -1))


def test_merge_tie_across_lists_takes_the_lower_node():
    a = np.array([[key(50, 900), key(40, 901)]], np.uint64)
    b = np.array([[key(50, 17), key(50, 899)]], np.uint64)
    st, out_k, _ = merge(np.stack([a, b]), None, 2, 1, 2)
    assert st == 0
    np.testing.assert_array_equal(out_k, [[key(50, 17), key(50, 899)]])
    st, out_k, _ = merge(np.stack([b, a]), None, 2, 1, 2)     # the order of the lists does not matter
    assert st == 0
    np.testing.assert_array_equal(out_k, [[key(50, 17), key(50, 899)]])


def test_merge_refuses_malformed_input():
    good = np.array([[[key(9, 1), key(8, 2), key(8, 5), 0]], [[key(9, 0), key(3, 7), 0, 0]]], np.uint64)
    sc = np.arange(2 * 1 * 4 * 4, dtype=np.uint8).reshape(2, 1, 4, 4)
    assert merge(good, sc, 2, 1, 4)[0] == 0

    def refused(keys, scores=sc, n_lists=2, n=1, k=4):
        st, out_k, out_s = merge(keys, scores, n_lists, n, k)
        assert st == ERR_INVALID_ARG
        assert (out_k == np.uint64(0xABABABABABABABAB)).all() and (out_s is None or (out_s == 0xAB).all())

    for cell, value, what in (((0, 0, 2), key(8, 2), "an equal neighbour: not strictly descending"),
                              ((0, 0, 2), key(8, 1), "ascending"),
                              ((1, 0, 3), key(1, 9), "a key after a 0"),
                              ((1, 0, 1), key(8, 5), "the same key in two lists: the shards overlap")):
        bad = good.copy()
        bad[cell] = value
        refused(bad)
    refused(good, n_lists=0)
    refused(good, k=0)
    L = nat.lib()
    out = np.full((1, 4), 0xABABABABABABABAB, dtype=np.uint64)
    out_s = np.full((1, 4, 4), 0xAB, dtype=np.uint8)
    flat = np.ascontiguousarray(good)
    assert L.kg_candidates_merge(nat.ptr(flat), nat.ptr(sc), 2, -1, 4, nat.ptr(out), nat.ptr(out_s)) == ERR_INVALID_ARG
    assert L.kg_candidates_merge(nat.ptr(flat), nat.ptr(sc), 2, 1, 65, nat.ptr(out), nat.ptr(out_s)) == ERR_INVALID_ARG
    assert L.kg_candidates_merge(None, nat.ptr(sc), 2, 1, 4, nat.ptr(out), nat.ptr(out_s)) == ERR_INVALID_ARG
    assert L.kg_candidates_merge(nat.ptr(flat), nat.ptr(sc), 2, 1, 4, None, nat.ptr(out_s)) == ERR_INVALID_ARG
    assert L.kg_candidates_merge(nat.ptr(flat), nat.ptr(sc), 2, 1, 4, nat.ptr(out), None) == ERR_INVALID_ARG   # scores without out_scores
    assert L.kg_candidates_merge(nat.ptr(flat), None, 2, 1, 4, nat.ptr(out), nat.ptr(out_s)) == ERR_INVALID_ARG   # and the reverse
    assert (out == np.uint64(0xABABABABABABABAB)).all() and (out_s == 0xAB).all()
    with pytest.raises(engine.EngineError):
        bad = good.copy()
        bad[1, 0, 1] = key(8, 5)
        engine.merge_candidates([{"keys": bad[0], "n_feasible": [3]}, {"keys": bad[1], "n_feasible": [2]}])


@pytest.mark.parametrize("k", [1, 16, 64])
def test_merge_of_the_tile_split_equals_the_whole(k):
    """The shipped oracle matrix (96 × 1,100) split at the tile boundary, as two shards would return it."""
    _, fit, la, tot = cc.oracle_matrix("shipped")
    keys, scores = split_lists(tot, fit, la, k, [(0, 1024), (1024, cc.N_NODES)])
    want_k, want_s, nf = cr.cand_ref(tot, k, fit, la)
    st, out_k, out_s = merge(keys, scores, 2, cc.N_PODS, k)
    assert st == 0
    np.testing.assert_array_equal(out_k, want_k)
    np.testing.assert_array_equal(out_s, want_s)
    assert nf.min() > k   # every list is full: the merge cuts, it does not merely concatenate


def test_reference_has_a_tie_at_every_k():
    """What tests/test_candidates_gpu.py::test_oracle_parity relies on: a tie in total straddling the cut at k = 16 and
    k = 64 in every profile, at k = 1 in some profile, and a node beyond the fp64 bounds in some pod's list."""
    assert any(cr.tie_at_cut(cc.oracle_matrix(p)[3], 1) for p in cc.PROFILES)
    for p in cc.PROFILES:
        _, fit, la, tot = cc.oracle_matrix(p)
        assert cr.tie_at_cut(tot, 16) and cr.tie_at_cut(tot, 64)
        keys = cr.cand_ref(tot, 64, fit, la)[0]
        assert np.isin(engine.decode_top1(keys)[0][keys != 0], cc.BIG).any()
