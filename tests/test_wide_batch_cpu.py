"""kg_batch_slot_map on the host (no GPU): the slot map kg_pods_set chooses and the spill pods of batches that
compare or score more than 8 resources (tests/wide_cases.py), against a Python restatement of the rule; the three
legacy maps on batches of at most 8 resources; and the wide fixture itself against the oracle."""
import numpy as np

import wide_cases as wc
from koordinator_amd import _native as nat
from koordinator_amd import engine, synth
from koordinator_amd.config import make_config, shipped_profile
from rows_ref import rows_eval


def test_slot_map_matches_the_rule_on_the_wide_batch():
    for name in ("matrix_least9", "matrix_most4", "place"):
        c = wc.case(name)
        need = wc.pod_need(c.cfg, c.pod_rows)
        assert bin(int(np.bitwise_or.reduce(need))).count("1") > 8   # the union does not fit 8 slots
        n_slots, slot_res, spill = wc.slot_map_rule(need)
        assert (c.n_slots, c.slot_res.tolist()) == (n_slots, slot_res)
        np.testing.assert_array_equal(c.spill, spill)
        assert slot_res[:2] == [nat.RES_CPU, nat.RES_MEMORY] and slot_res[2:] == sorted(slot_res[2:])
        assert 0.25 <= c.spill.mean() <= 0.75, c.spill.mean()
        # a spill pod needs a resource outside the map, the others none
        held = sum(1 << r for r in slot_res)
        np.testing.assert_array_equal((need & ~held) != 0, c.spill)


def test_slot_map_is_deterministic_and_optional_spill():
    import ctypes
    c = wc.case("matrix_least9")
    again = engine.batch_slot_map(c.cfg, c.pod_rows)
    assert again[0] == c.n_slots and again[1].tolist() == c.slot_res.tolist()
    np.testing.assert_array_equal(again[2], c.spill)
    ns, sr = ctypes.c_int32(), np.zeros(8, np.int32)
    rows = np.ascontiguousarray(c.pod_rows)
    assert nat.lib().kg_batch_slot_map(nat.ptr(c.cfg), nat.ptr(rows), len(rows), ctypes.addressof(ns), nat.ptr(sr),
                                       None) == 0   # spill may be NULL
    assert ns.value == 8 and sr.tolist() == c.slot_res.tolist()
    assert nat.lib().kg_batch_slot_map(nat.ptr(c.cfg), None, 3, ctypes.addressof(ns), nat.ptr(sr), None) != 0
    assert engine.batch_slot_map(c.cfg, rows[:0])[0] == 2   # the empty batch: cpu, memory


def test_legacy_maps_unchanged():
    """Batches of at most 8 resources: exactly the 2-, 4- and 8-slot maps kg_pods_set always built, no spill pods."""
    P = 200
    native = make_config()                       # scores cpu, memory
    cl = synth.make_cluster(500, P, seed=5)
    rows = engine.build_pod_rows(native, cl, np.arange(P))
    ls = rows[(rows["request_present"] & 0xFF8) == 0]          # pods without batch requests
    n, sr, sp = engine.batch_slot_map(native, ls)
    assert (n, sr.tolist(), sp.any()) == (2, [0, 1, -1, -1, -1, -1, -1, -1], False) and len(ls) > P // 2
    n, sr, sp = engine.batch_slot_map(shipped_profile(), engine.build_pod_rows(shipped_profile(), cl, np.arange(P)))
    assert (n, sr.tolist(), sp.any()) == (4, [0, 1, nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY, -1, -1, -1, -1], False)
    cfg = shipped_profile(extended_resources=synth.SCALAR_NAMES)
    sc = synth.make_scalar_cluster(500, P, seed=5)
    rows = engine.build_pod_rows(cfg, sc, np.arange(P))
    n, sr, sp = engine.batch_slot_map(cfg, rows)
    want = [0, 1, nat.RES_BATCH_CPU, nat.RES_BATCH_MEMORY, nat.RES_EXT0, nat.RES_EXT1, nat.RES_EXT2, nat.RES_EXT3]
    assert (n, sr.tolist(), sp.any()) == (8, want, False)
    # an ephemeral-storage request alone leaves the 4-slot map for the 8-slot one (unused slots −1)
    one = rows[:1].copy()
    one["request_present"] = 0
    one["request"][:] = 0
    one["fit_score_request"][0, 3:] = 0
    one["request"][0, nat.RES_EPHEMERAL_STORAGE] = 1 << 30
    one["flags"] |= nat.POD_HAS_REQUEST
    n, sr, sp = engine.batch_slot_map(cfg, one)
    assert (n, sr.tolist(), sp.any()) == (8, [0, 1, nat.RES_EPHEMERAL_STORAGE, -1, -1, -1, -1, -1], False)


def test_one_pod_needing_nine_resources_is_the_spill_pod():
    cfg = wc.wide_config("least9")
    rows = np.zeros(3, dtype=nat.POD_ROW)
    rows["flags"] = nat.POD_HAS_REQUEST | nat.POD_VALID
    rows["request"][:, nat.RES_CPU] = 500
    rows["request"][:, nat.RES_MEMORY] = 1 << 30
    rows["fit_score_request"][:, :2] = rows["request"][:, :2]
    rows["request_present"] = 0x3
    # pod 1: cpu, memory, ephemeral-storage (scored by every pod) and six scalar keys of its own: 9 resources
    for r in (nat.RES_BATCH_CPU, nat.RES_MID_CPU, nat.RES_EXT0, nat.RES_EXT2, nat.RES_EXT3, nat.RES_EXT4):
        rows["request"][1, r] = 1
        rows["request_present"][1] |= 1 << r
    rows["request"][2, nat.RES_EXT0] = 2
    rows["request_present"][2] |= 1 << nat.RES_EXT0
    need = wc.pod_need(cfg, rows)
    assert [bin(int(x)).count("1") for x in need] == [3, 9, 4]
    n, sr, sp = engine.batch_slot_map(cfg, rows)
    assert n == 8 and sp.tolist() == [False, True, False]
    # ephemeral-storage (3 pods) and nvidia.com/gpu (2) first, then the lowest ids among the resources of one pod
    assert sr.tolist() == [0, 1, nat.RES_EPHEMERAL_STORAGE, nat.RES_BATCH_CPU, nat.RES_MID_CPU, nat.RES_EXT0,
                           nat.RES_EXT2, nat.RES_EXT3]
    assert (wc.slot_map_rule(need)[1], wc.slot_map_rule(need)[2].tolist()) == (sr.tolist(), sp.tolist())


def test_wide_fixture_rows_match_oracle():
    """The fixture: the exact row evaluation equals the oracle's object-level matrices on the wide cluster, every
    spill pod has a feasible and an infeasible node, and the oracle's cycle places the placement batch."""
    for name in ("matrix_least9", "matrix_most4"):
        c = wc.case(name)
        m, f, l = rows_eval(c.cfg, c.node_rows, c.pod_rows, c.cl.now_ns)
        m_ref, f_ref, l_ref = c.matrix
        np.testing.assert_array_equal(m, m_ref)
        np.testing.assert_array_equal(f, f_ref)
        np.testing.assert_array_equal(l, l_ref)
        c.check_mixed()
    for name in ("shard", "first", "last", "all"):
        wc.case(name).check_spill_rows()
    assert wc.case("first").spill.tolist() == [True] + [False] * 36
    assert wc.case("last").spill.tolist() == [False] * 36 + [True]
    assert wc.case("all").spill.all()
    nodes, _ = wc.case("place").schedule
    assert (nodes >= 0).all() and wc.case("place").spill[nodes >= 0].any()


def test_slot_map_under_sanitizers(tmp_path):
    """kg_batch_slot_map under AddressSanitizer + UndefinedBehaviorSanitizer: tests/wide_slot_map_san.cpp (its own
    main) compiled with the host sources and run as a program of its own."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "koordinator_amd", "csrc")
    exe = str(tmp_path / "wide_slot_map_san")
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host objects of the engine too"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "wide_slot_map_san.cpp"), os.path.join(csrc, "kg_host.cpp"),
                    os.path.join(csrc, "kg_cpuset.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout + r.stderr[-3000:]
