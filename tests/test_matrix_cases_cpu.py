"""The inputs of the matrix containment tests (tests/matrix_cases.py), checked from the oracle alone, and the guard
helper's layout arithmetic (tests/guarded_out.py) on CPU tensors: what the GPU tests rely on is proved here first."""
import numpy as np
import pytest

import guarded_out as go
import matrix_cases as mc
from koordinator_amd import _native as nat
from koordinator_amd import engine

ALL = mc.all_cases()
SHAPED = [f for f in mc.FAMILIES if f != "bind"]   # (the cpuset batch is one extra writer of the numa family)


@pytest.mark.parametrize("family", SHAPED)
def test_every_family_covers_the_mandatory_shapes(family):
    cases = mc.FAMILIES[family]
    sizes = {c.n_nodes for c in cases if c.full}
    shards = {(c.begin, c.end) for c in cases if not c.full and c.n_nodes == mc.SHARD_SNAPSHOT}
    assert set(mc.MANDATORY_SIZES) <= sizes
    assert set(mc.MANDATORY_SHARDS) <= shards
    assert set(mc.MANDATORY_PODS) <= {c.n_pods for c in cases}
    assert len({(c.id, c.family) for c in cases}) == len(cases)


def test_the_class_family_runs_every_listed_shape():
    cases = mc.FAMILIES["class"]
    assert set(mc.SNAPSHOT_SIZES) <= {c.n_nodes for c in cases if c.full}
    assert set(mc.SHARDS) <= {(c.begin, c.end) for c in cases if c.n_nodes == mc.SHARD_SNAPSHOT and not c.full}
    assert set(mc.POD_COUNTS) <= {c.n_pods for c in cases}
    words = {(c.width + 63) // 64 for c in cases}
    assert 3 in words and 17 in words   # odd mask_words: 8-byte-aligned 16-byte mask stores, k_eq_rows<8>
    numa_words = {((c.width + 63) // 64, c.eq) for c in mc.FAMILIES["numa"]}
    assert (3, True) in numa_words and (17, True) in numa_words and (16, True) in numa_words


@pytest.mark.parametrize("case", ALL, ids=lambda c: f"{c.family}-{c.id}")
def test_input_conditions(case):
    ref = mc.reference(case)
    inp = mc.inputs(case)
    m = ref["mask"]
    W, P = case.width, case.n_pods
    assert m.shape == (P, W) and len(inp.idx) == P and len(inp.view.nodes) == case.n_nodes
    if W >= 64:
        assert 0.05 <= m.mean() <= 0.95, f"feasible fraction {m.mean():.3f}"
    if W > 0:
        # the last mask word: each 32-column half that has in-range columns holds a feasible one for some pod (a
        # width of at most 32 columns in the last word leaves its high half without any)
        last = (W - 1) // 64 * 64
        col_any = m.any(axis=0)
        assert col_any[last:min(last + 32, W)].any(), "low half of the last word has no feasible column"
        if W > last + 32:
            assert col_any[last + 32:W].any(), "high half of the last word has no feasible column"
    if case.family in ("slow", "la_extra") and case.variant != "exact":
        inside, outside = inp.special
        rows = engine.build_node_rows(inp.cfg, inp.view)
        # (what the engine will call slow: the row builder's own verdict is not visible here, so the inputs are
        # pinned instead — allocatable beyond 2^41 bytes is outside the fp64 bounds, test_matrix_slow_path_huge_nodes)
        huge = (rows["alloc"][:, nat.RES_MEMORY] >= 1 << 41) | (rows["alloc"][:, nat.RES_EPHEMERAL_STORAGE] >= 1 << 41)
        assert set(np.flatnonzero(huge)) == set(inside) | set(outside)
        if W > 0:
            assert len(inside) >= 1 and all(case.begin <= j < case.end for j in inside)
            assert case.begin in inside and case.end - 1 in inside
            assert (W <= 63 or case.begin + 63 in inside) and (W <= 64 or case.begin + 64 in inside)
            assert m[:, [j - case.begin for j in inside]].any(), "no slow node is feasible for any pod"
        if not case.full:   # (a whole-snapshot range has no node outside it)
            assert len(outside) >= 1 and not any(case.begin <= j < case.end for j in outside)
    if case.family == "dup" and P >= 65:
        pods, counts = np.unique(inp.idx, return_counts=True)
        straddle = [p for p, c in zip(pods, counts)
                    if c >= 2 and (np.flatnonzero(inp.idx == p) < 64).any() and (np.flatnonzero(inp.idx == p) >= 64).any()]
        assert straddle, "no repeated row straddles a 64-pod boundary"
        assert counts.min() == 1 and counts.max() == (70 if P >= 130 else 40) and 2 in counts
    if case.family == "numa":
        rows = engine.build_pod_rows(inp.cfg, inp.view, inp.idx)
        distinct = len({r.tobytes() for r in rows})
        if case.eq:
            assert P >= 64 and 4 * distinct <= 3 * P   # kg_pods_set turns the equivalent-pod path on
        elif P >= 64:
            assert 4 * distinct > 3 * P
    if case.family == "rsv":
        rsv_nodes = ref["rsv_nodes"]
        node = (np.uint64(0xFFFFFFFF) - (ref["top1"] & np.uint64(0xFFFFFFFF))).astype(np.int64)
        best_is_rsv = (ref["top1"] != 0) & np.isin(node, rsv_nodes)
        assert best_is_rsv.any(), "no pod's best node is a reservation node"
        if case.full:   # the reference's own top1 rule against the oracle's keys
            np.testing.assert_array_equal(ref["top1"], ref["top1_whole"])
        if case.n_nodes == mc.SHARD_SNAPSHOT and W > 0:
            assert ((rsv_nodes >= case.begin) & (rsv_nodes < case.end)).any()
            assert ((rsv_nodes < case.begin) | (rsv_nodes >= case.end)).any()
        if P >= 65:
            from oracle import oracle
            pods = inp.view.pods[inp.idx]
            assert (pods["rsv_affinity_class"] >= 0).any(), "no pod requires a reservation"
            cfg_open = inp.cfg.copy()
            cfg_open["enabled_plugins"] = int(cfg_open["enabled_plugins"]) & ~nat.PLUGIN_ELASTICQUOTA
            open_mask = oracle.eval_matrix5(cfg_open, inp.view, inp.idx, inp.now_ns)[0]
            gated = open_mask.any(axis=1) & ~ref["mask_whole"].any(axis=1)
            assert gated.any(), "no pod fails the quota gate"


def test_guard_layout_on_cpu_tensors():
    import torch
    for nbytes in (0, 8, 520, 130 * 17 * 8, 130 * 1088 * 2):
        for prefill in (0x00, 0xFF):
            g = go.GuardedPlane(nbytes, prefill, torch.device("cpu"))
            assert g.off >= go.GUARD and g.ptr % go.ALIGN == 0
            front, payload, back = g.read()
            assert len(front) >= go.GUARD and len(back) >= go.GUARD and len(payload) == nbytes
            assert g.stray(payload_too=True).size == 0
            if nbytes:   # a write inside the payload is no stray; one byte either side of it is
                g.buf[g.off] = prefill ^ 0x5A
                g.buf[g.off + nbytes - 1] = prefill ^ 0x5A
                assert g.stray().size == 0 and list(g.stray(payload_too=True)) == [0, nbytes - 1]
            g.buf[g.off - 1] = prefill ^ 0x5A
            g.buf[g.off + nbytes] = prefill ^ 0x5A
            assert list(g.stray()) == [-1, nbytes]
    for base in (0, 1, 255, 256, 4096 + 16, (1 << 40) + 200):
        off = go.payload_offset(base)
        assert go.GUARD <= off < go.GUARD + go.ALIGN and (base + off) % go.ALIGN == 0
        assert go.total_bytes(100) - off - 100 >= go.GUARD
    b = go.plane_bytes(65, 1076)   # the shard [1024, 2100): 17 words, a 52-bit last word
    assert b == {"mask": 65 * 17 * 8, "scores": 65 * 1088 * 2, "top1": 65 * 8, "numa": 65 * 1088, "rsv": 65 * 1088}
    assert go.plane_bytes(65, 0) == {"mask": 0, "scores": 0, "top1": 520, "numa": 0, "rsv": 0}
    payload = np.arange(2 * 128 * 2, dtype=np.uint8)
    assert go.shape_payload("scores", payload, 2, 2).shape == (2, 128, 2)
    assert go.shape_payload("mask", np.zeros(0, np.uint8), 65, 0).shape == (65, 0)


def test_check_against_reference_sees_pad_bits_and_wrong_cells():
    case = mc.Case("class", "shipped", 33, 0, 33, 130)
    ref = mc.reference(case)
    mask = np.packbits(np.pad(ref["mask"], ((0, 0), (0, 31))), axis=1, bitorder="little").view(np.uint64)
    scores = np.zeros((130, 64, 2), np.uint8)
    scores[:, :33, 0], scores[:, :33, 1] = ref["fit"], ref["la"]
    scores[:, 33:] = 0xFF   # unspecified pad columns
    good = {"mask": mask, "scores": scores, "top1": ref["top1"]}
    mc.check_against_reference(case, good)
    with pytest.raises(AssertionError, match="pad bits"):
        mc.check_against_reference(case, dict(good, mask=mask | np.uint64(1 << 33)))
    bad = scores.copy()
    bad[129, 32, 1] ^= 1
    with pytest.raises(AssertionError, match="LoadAware"):
        mc.check_against_reference(case, dict(good, scores=bad))
    with pytest.raises(AssertionError, match="top1"):
        mc.check_against_reference(case, dict(good, top1=ref["top1"] + np.uint64(1)))
