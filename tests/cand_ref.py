"""Reference of kg_candidates / kg_candidates_merge (tests/test_candidates_*.py): pure NumPy.

TEST INFRASTRUCTURE: no engine code runs here.  A pod's list is its feasible nodes in a stable sort by
(−total, node): higher total first, among equal totals the lower node index first, which is the descending order
of the keys (total + 1) << 32 | (0xFFFFFFFF − node).
"""
import numpy as np


def keys_of(totals, node0=0):
    """uint64 [P][N]: the key of every pair (0 where totals < 0); column c is node node0 + c."""
    totals = np.asarray(totals, dtype=np.int64)
    node = np.arange(totals.shape[1], dtype=np.uint64) + np.uint64(node0)
    key = ((totals + 1).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - node)[None, :]
    return np.where(totals >= 0, key, np.uint64(0))


def cand_ref(totals, k, fit=None, la=None, numa=None, node0=0):
    """(keys [P][k] u64, scores [P][k][4] u8, n_feasible [P] u32) from totals [P][N] (−1 where infeasible) and the
    optional plugin-score matrices [P][N] (a missing one: 0, as a disabled plugin)."""
    totals = np.asarray(totals, dtype=np.int64)
    P, N = totals.shape
    order = np.argsort(-totals, axis=1, kind="stable")[:, :k]     # infeasible pairs (−1 → +1) sort last
    rows = np.arange(P)[:, None]
    keys = np.zeros((P, k), dtype=np.uint64)
    scores = np.zeros((P, k, 4), dtype=np.uint8)
    m = min(k, N)
    picked = keys_of(totals, node0)[rows, order]
    keys[:, :m] = picked
    for b, plane in enumerate((fit, la, numa)):
        if plane is not None:
            scores[:, :m, b] = np.where(picked != 0, np.asarray(plane)[rows, order], 0)
    return keys, scores, (totals >= 0).sum(axis=1).astype(np.uint32)


def tie_at_cut(totals, k):
    """True when some pod's (k)-th and (k + 1)-th best feasible totals are equal: a tie straddling the cut."""
    totals = np.asarray(totals, dtype=np.int64)
    if totals.shape[1] <= k:
        return False
    s = -np.sort(-totals, axis=1)
    return bool(((s[:, k - 1] == s[:, k]) & (s[:, k] >= 0)).any())


def from_planes(cfg, res, n_nodes):
    """(totals, fit, la, numa) [P][n_nodes] from an Engine.eval() result (mask, scores and, under NodeNUMAResource,
    numa_scores): totals −1 where the mask bit is clear."""
    from koordinator_amd import engine
    mask = engine.unpack_mask(res["mask"], n_nodes)
    fit = res["scores"][:, :n_nodes, 0].astype(np.int64)
    la = res["scores"][:, :n_nodes, 1].astype(np.int64)
    numa = res["numa_scores"][:, :n_nodes].astype(np.int64) if "numa_scores" in res else np.zeros_like(fit)
    tot = int(cfg["weight_fit"]) * fit + int(cfg["weight_loadaware"]) * la + int(cfg["weight_numa"]) * numa
    return np.where(mask, tot, -1), fit, la, numa
