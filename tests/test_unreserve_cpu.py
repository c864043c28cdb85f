"""kg_row_unreserve / kg_row_numa_alloc on host rows (no GPU): the exact inverse of kg_row_commit, the clamped zone
release of NodeAllocation.release, the transitions a release takes a row through, and the argument errors."""
import os
import re

import numpy as np
import pytest

import churn_cases as ch
import unreserve_cases as uc
from koordinator_amd import _native as nat
from koordinator_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_STATE = -1, -5


def _status(cfg, row, pod, zones=None):
    return nat.lib().kg_row_unreserve(nat.ptr(cfg), nat.ptr(row), nat.ptr(pod), nat.ptr(zones))


def test_header_abi_and_symbols():
    with open(os.path.join(ROOT, "include", "koord_gpu.h")) as f:
        text = f.read()
    assert re.search(r"#define KG_ABI_VERSION 13\b", text) and nat.lib().kg_abi_version() == 13
    m = re.search(r"#define KG_UNRESERVE_MAX (\d+)", text)
    assert m and int(m.group(1)) == nat.UNRESERVE_MAX == 4096
    for name in ("kg_row_unreserve", "kg_row_numa_alloc", "kg_unreserve"):
        assert name in nat.EXPORTED and getattr(nat.lib(), name) is not None
        assert re.search(r"kg_status %s\(" % name, text)


@pytest.mark.parametrize("extra", [False, True], ids=["shipped", "la_extra"])
def test_commit_then_unreserve_restores_the_row_bytes(extra):
    cfg, rows, first, second = uc.fit_la_cluster(extra)
    pods = np.concatenate([first, second])
    rng = np.random.default_rng(5)
    valid = np.flatnonzero((rows["flags"] & nat.NODE_VALID) != 0)
    changed = 0
    for _ in range(200):
        j, p = int(rng.choice(valid)), int(rng.integers(len(pods)))
        row, pod = rows[j:j + 1].copy(), pods[p:p + 1]
        engine.row_commit(cfg, row, pod)
        changed += row.tobytes() != rows[j:j + 1].tobytes()
        committed = row.copy()
        engine.row_unreserve(cfg, row, pod)
        assert row.tobytes() == rows[j:j + 1].tobytes(), (j, p)
        # and the restatement of the rules gives the same row
        assert uc.restate_row_unreserve(cfg, committed[0], pod[0]).tobytes() == row[0].tobytes()
    assert changed == 200
    if extra:
        assert (pods["la_estimate_x"] != 0).any(), "the extra-weights profile moves la_used_x"


def test_middle_rollback_equals_never_reserved():
    """S0 + A + B − A = S0 + B by bytes (NodeNUMAResource off: plain subtraction commutes with B's Reserve)."""
    cfg, rows, first, second = uc.fit_la_cluster()
    rng = np.random.default_rng(6)
    valid = np.flatnonzero((rows["flags"] & nat.NODE_VALID) != 0)
    for _ in range(100):
        j = int(rng.choice(valid))
        a, b = first[int(rng.integers(len(first)))][None], second[int(rng.integers(len(second)))][None]
        x, y = rows[j:j + 1].copy(), rows[j:j + 1].copy()
        engine.row_commit(cfg, x, a)
        engine.row_commit(cfg, x, b)
        engine.row_unreserve(cfg, x, a)
        engine.row_commit(cfg, y, b)
        assert x.tobytes() == y.tobytes()


def _numa_pairs(n):
    """(row index, pod a, pod b) whose Reserves both record a zone allocation."""
    cfg, rows, first, second = uc.numa_cluster()
    out = []
    rng = np.random.default_rng(7)
    while len(out) < n:
        j = int(rng.integers(len(rows)))
        a, b = first[int(rng.integers(len(first)))][None], second[int(rng.integers(len(second)))][None]
        if not engine.row_eval(cfg, rows[j:j + 1], a, uc.NOW)[0]:
            continue
        rec = engine.row_numa_alloc(cfg, rows[j:j + 1], a)
        if not rec.any():
            continue
        mid = rows[j:j + 1].copy()
        engine.row_commit(cfg, mid, a)
        if engine.row_eval(cfg, mid, b, uc.NOW)[0] and engine.row_numa_alloc(cfg, mid, b).any():
            out.append((j, a, b))
    return cfg, rows, out


def test_numa_alloc_is_what_the_commit_records():
    cfg, rows, pairs = _numa_pairs(40)
    for j, a, _ in pairs:
        before = rows[j:j + 1].copy()
        rec = engine.row_numa_alloc(cfg, before, a)
        assert before.tobytes() == rows[j:j + 1].tobytes(), "the row is not modified"
        after = before.copy()
        engine.row_commit(cfg, after, a)
        np.testing.assert_array_equal(rec, after["zone_allocated"][0] - before["zone_allocated"][0])
        assert (rec >= 0).all()


def test_numa_release_follows_node_allocation_release():
    cfg, rows, pairs = _numa_pairs(40)
    for j, a, b in pairs:
        row = rows[j:j + 1].copy()
        rec_a = engine.row_numa_alloc(cfg, row, a)
        engine.row_commit(cfg, row, a)
        engine.row_commit(cfg, row, b)
        keys_ab = int(row["zone_alloc_keys"][0])
        want = uc.restate_row_unreserve(cfg, row[0], a[0], rec_a)
        engine.row_unreserve(cfg, row, a, rec_a)
        np.testing.assert_array_equal(row["zone_allocated"][0], want["zone_allocated"])
        assert row[0].tobytes() == want.tobytes()
        assert int(row["zone_alloc_keys"][0]) & keys_ab == keys_ab, "no key bit is cleared"


def test_numa_over_release_clamps_and_zones_without_entry_stay():
    cfg, rows, pairs = _numa_pairs(8)
    j, a, _ = pairs[0]
    row = rows[j:j + 1].copy()
    rec = engine.row_numa_alloc(cfg, row, a)
    engine.row_commit(cfg, row, a)
    z = int(np.flatnonzero(rec.any(axis=1))[0])
    big = rec.copy()
    big[z] = row["zone_allocated"][0][z] + 10**9           # more than the zone holds
    keys = int(row["zone_alloc_keys"][0])
    engine.row_unreserve(cfg, row, a, big)
    assert (row["zone_allocated"][0][z] == 0).all() and int(row["zone_alloc_keys"][0]) & keys == keys
    assert (int(row["zone_alloc_keys"][0]) >> (2 * z)) & 3 == 3, "both released resources keep their key"
    # a zone without an allocation entry: a release names it, nothing changes there
    rows_w = np.flatnonzero(((rows["flags"] & nat.NODE_VALID) != 0) & (rows["n_zones"] >= 2) & (rows["pod_count"] >= 1))
    row = rows[rows_w[:1]].copy()
    row["zone_alloc_keys"] &= ~np.uint32(3 << 2)          # zone 1 loses its entry
    row["zone_allocated"][0][1] = (777, 888)
    rel = np.zeros((nat.MAX_ZONES, 2), np.int64)
    rel[1] = (500, 500)
    keys = int(row["zone_alloc_keys"][0])
    engine.row_unreserve(cfg, row, a, rel)
    assert tuple(row["zone_allocated"][0][1]) == (777, 888) and int(row["zone_alloc_keys"][0]) == keys


@pytest.mark.parametrize("name", ["pods_full", "over_cpu", "val_limit"])
def test_release_leaves_the_transition(name):
    cfg, cases = uc.transition_rows()
    row0, pod = cases[name]
    flag = uc.TRANSITION_FLAG[name]
    row = np.array([row0])
    assert not flag(cfg, row[0]), "not before the Reserve"
    engine.row_commit(cfg, row, pod)
    assert flag(cfg, row[0]), "while the pod is on the row"
    engine.row_unreserve(cfg, row, pod)
    assert not flag(cfg, row[0]) and row[0].tobytes() == row0.tobytes()
    if name == "val_limit":
        assert int(row0["nonzero_requested"][0]) + int(pod["nonzero_request"][0, 0]) == ch.VAL_LIMIT


def test_argument_errors_leave_the_row_unchanged():
    cfg, rows, first, _ = uc.fit_la_cluster()
    ncfg, nrows, nfirst, _ = uc.numa_cluster()
    pod = first[:1]
    zeros = np.zeros((nat.MAX_ZONES, 2), np.int64)

    def refused(cfg_, row, pod_, zones, status):
        keep = row.copy()
        assert _status(cfg_, row, pod_, zones) == status
        assert row.tobytes() == keep.tobytes()

    valid = np.flatnonzero((rows["flags"] & nat.NODE_VALID) != 0)
    empty = rows[valid[:1]].copy()
    empty["pod_count"] = 0
    refused(cfg, empty, pod, None, ERR_STATE)                       # no pod to release
    gone = np.zeros(1, nat.NODE_ROW)
    gone["pod_count"] = 5
    refused(cfg, gone, pod, None, ERR_STATE)                        # not KG_NODE_VALID
    refused(cfg, rows[valid[:1]].copy(), pod, zeros, ERR_INVALID_ARG)   # zone_release with NodeNUMAResource disabled
    nv = np.flatnonzero(((nrows["flags"] & nat.NODE_VALID) != 0) & (nrows["n_zones"] >= 1) & (nrows["n_zones"] < nat.MAX_ZONES)
                        & (nrows["pod_count"] >= 1))
    nrow = nrows[nv[:1]].copy()
    neg = zeros.copy()
    neg[0, 1] = -1
    refused(ncfg, nrow, nfirst[:1], neg, ERR_INVALID_ARG)           # a negative amount
    past = zeros.copy()
    past[int(nrow["n_zones"][0]), 0] = 1
    refused(ncfg, nrow, nfirst[:1], past, ERR_INVALID_ARG)          # a non-zero amount at z >= n_zones
    assert _status(ncfg, nrow, nfirst[:1], zeros) == 0              # all zero: fine
    for args in ((None, nat.ptr(nrow), nat.ptr(pod), None), (nat.ptr(cfg), None, nat.ptr(pod), None),
                 (nat.ptr(cfg), nat.ptr(nrow), None, None)):
        assert nat.lib().kg_row_unreserve(*args) == ERR_INVALID_ARG
    assert nat.lib().kg_row_numa_alloc(nat.ptr(ncfg), nat.ptr(nrow), nat.ptr(pod), None) == ERR_INVALID_ARG
