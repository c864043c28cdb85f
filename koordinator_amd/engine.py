"""Python handle on the HIP engine (``libkoordgpu.so``), used by the plugin mirror, tests and bench."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _native as nat
from . import debug


class EngineError(RuntimeError):
    pass


def _check(st: int, eng: Optional["Engine"] = None, what: str = "") -> None:
    if st != 0:
        msg = nat.lib().kg_last_error(eng._h).decode() if eng is not None and eng._h else ""
        raise EngineError(f"{what} failed with status {st}: {msg}")


def build_pod_rows(cfg: np.ndarray, view, pod_index: Sequence[int]) -> np.ndarray:
    idx = np.ascontiguousarray(pod_index, dtype=np.int32)
    out = np.zeros(len(idx), dtype=nat.POD_ROW)
    _check(nat.lib().kg_build_pod_rows(nat.ptr(cfg), ctypes.byref(view.c_view), nat.ptr(idx), len(idx), nat.ptr(out)),
           what="kg_build_pod_rows")
    return out


def build_node_rows(cfg: np.ndarray, view, node_index: Optional[Sequence[int]] = None) -> np.ndarray:
    n = len(view.nodes)
    idx = np.arange(n, dtype=np.int32) if node_index is None else np.ascontiguousarray(node_index, dtype=np.int32)
    out = np.zeros(len(idx), dtype=nat.NODE_ROW)
    _check(nat.lib().kg_build_node_rows(nat.ptr(cfg), ctypes.byref(view.c_view), nat.ptr(idx), len(idx), nat.ptr(out)),
           what="kg_build_node_rows")
    return out


def row_commit(cfg: np.ndarray, node_row: np.ndarray, pod_row: np.ndarray) -> None:
    _check(nat.lib().kg_row_commit(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(pod_row)), what="kg_row_commit")


def row_unreserve(cfg: np.ndarray, node_row: np.ndarray, pod_row: np.ndarray, zone_release=None) -> None:
    """kg_row_unreserve: the inverse of row_commit on a host row (in place).  `zone_release`: the pod's recorded zone
    allocation, int64 [MAX_ZONES][2] by zone slot (row_numa_alloc at Reserve time), or None."""
    zr = None if zone_release is None else np.ascontiguousarray(zone_release, dtype=np.int64).reshape(nat.MAX_ZONES, 2)
    _check(nat.lib().kg_row_unreserve(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(pod_row), nat.ptr(zr)),
           what="kg_row_unreserve")


def gang_plan(pod_gang, gang_flags, gang_group=None, chunk: int = 0) -> np.ndarray:
    """kg_gang_plan: the argument checks of Engine.place_gangs that need no engine and the chunk cuts it will use for
    place_chunk = `chunk` (0: the default 16).  Returns uint8 [P]: 1 where a placement chunk ends after the pod."""
    pg = np.ascontiguousarray(pod_gang, dtype=np.int32).reshape(-1)
    gf = np.ascontiguousarray(gang_flags, dtype=np.uint8).reshape(-1)
    gg = None if gang_group is None else np.ascontiguousarray(gang_group, dtype=np.int32).reshape(-1)
    if gg is not None and len(gg) != len(gf):
        raise ValueError("gang_flags and gang_group describe the same gangs")
    cut = np.zeros(len(pg), dtype=np.uint8)
    _check(nat.lib().kg_gang_plan(nat.ptr(pg) if len(pg) else None, len(pg), nat.ptr(gg) if len(gf) else None,
                                  nat.ptr(gf) if len(gf) else None, len(gf), int(chunk), nat.ptr(cut) if len(pg) else None),
           what="kg_gang_plan")
    return cut


def row_numa_alloc(cfg: np.ndarray, node_row: np.ndarray, pod_row: np.ndarray) -> np.ndarray:
    """kg_row_numa_alloc: the zone amounts row_commit would record for the pod on this (pre-Reserve) row, int64
    [MAX_ZONES][2] by zone slot; all zero where the commit records nothing.  The row is not modified."""
    out = np.zeros((nat.MAX_ZONES, 2), dtype=np.int64)
    _check(nat.lib().kg_row_numa_alloc(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(pod_row), nat.ptr(out)),
           what="kg_row_numa_alloc")
    return out


def row_reserve(cfg: np.ndarray, node_row: np.ndarray, pod_row: np.ndarray, cpus: np.ndarray, max_ref_count: int = 1,
                numa_allocate_strategy: int = 0):
    """kg_row_reserve: the Reserve of one pair on a host row and the node's CPU_INFO array (both updated in
    place).  Returns the taken cpuset (bool per cpu), or None when the Reserve fails (KG_NOT_FOUND)."""
    taken = np.zeros(len(cpus), dtype=np.uint8)
    st = nat.lib().kg_row_reserve(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(pod_row), nat.ptr(cpus) if len(cpus) else None,
                                  len(cpus), int(max_ref_count), int(numa_allocate_strategy),
                                  nat.ptr(taken) if len(cpus) else None)
    if st == nat.NOT_FOUND:
        return None
    _check(st, what="kg_row_reserve")
    return taken.astype(bool)


def row_eval(cfg: np.ndarray, node_row: np.ndarray, pod_row: np.ndarray, now_ns: int):
    """(feasible, fit, la, numa) of one pair on host rows (the kernels' per-pair code, run on the CPU)."""
    f, a, b, c = (ctypes.c_int32() for _ in range(4))
    _check(nat.lib().kg_row_eval(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(pod_row), int(now_ns), ctypes.byref(f),
                                 ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), what="kg_row_eval")
    return bool(f.value), a.value, b.value, c.value


def row_why(cfg: np.ndarray, node_row: np.ndarray, pod_row: np.ndarray, now_ns: int, first_fail: bool = False) -> int:
    """kg_row_why: the reason word (nat.WHY_*) of one pair on host rows; 0 ⇔ feasible.  Ignores elig_class."""
    w = ctypes.c_uint32(0)
    _check(nat.lib().kg_row_why(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(pod_row), int(now_ns),
                                nat.DIAG_FIRST_FAIL if first_fail else 0, ctypes.byref(w)), what="kg_row_why")
    return int(w.value)


def row_preempt(cfg: np.ndarray, node_row: np.ndarray, bound_rows: np.ndarray, bound_priority, bound_start_ns,
                pod_row: np.ndarray, pod_priority: int, now_ns: int, quotas: Optional[np.ndarray] = None) -> dict:
    """kg_row_preempt: the preemption dry run of one (preemptor, node) pair on host rows (SelectVictimsOnNode without
    PodDisruptionBudgets).  `bound_rows` / `bound_priority` / `bound_start_ns`: the node's bound pods in the caller's
    order.  Returns status (nat.PRE_*), victims (bool [nat.BOUND_MAX_PER_NODE], caller positions), n_victims, hi_prio,
    prio_sum and earliest_ns; everything but the status is zero unless the status is nat.PRE_CANDIDATE.  Ignores
    elig_class."""
    rows = np.ascontiguousarray(bound_rows, dtype=nat.POD_ROW).reshape(-1)
    n = len(rows)
    pr = np.ascontiguousarray(bound_priority, dtype=np.int32).reshape(-1)
    ts = np.ascontiguousarray(bound_start_ns, dtype=np.int64).reshape(-1)
    if len(pr) != n or len(ts) != n:
        raise ValueError("row_preempt takes one priority and one start time per bound row")
    q = None if quotas is None else np.ascontiguousarray(quotas, dtype=nat.QUOTA).reshape(-1)
    status = ctypes.c_int32(0)
    mask = np.zeros(2, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.int64)
    _check(nat.lib().kg_row_preempt(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(rows) if n else None, nat.ptr(pr) if n else None,
                                    nat.ptr(ts) if n else None, n, nat.ptr(pod_row), int(pod_priority),
                                    nat.ptr(q) if q is not None and len(q) else None, 0 if q is None else len(q),
                                    int(now_ns), ctypes.byref(status), nat.ptr(mask), nat.ptr(stats)), what="kg_row_preempt")
    return {"status": int(status.value), "victims": unpack_victims(mask), "n_victims": int(stats[0]),
            "hi_prio": int(stats[1]), "prio_sum": int(stats[2]), "earliest_ns": int(stats[3])}


def row_preempt_pdb(cfg: np.ndarray, node_row: np.ndarray, bound_rows: np.ndarray, bound_priority, bound_start_ns,
                    bound_pdb_prio, pod_row: np.ndarray, pod_priority: int, now_ns: int,
                    quotas: Optional[np.ndarray] = None) -> dict:
    """kg_row_preempt_pdb: row_preempt with one PDB threshold per bound pod (pdb_thresholds; None: the plain form).
    Adds n_violating (numViolatingVictim) to row_preempt's result."""
    rows = np.ascontiguousarray(bound_rows, dtype=nat.POD_ROW).reshape(-1)
    n = len(rows)
    pr = np.ascontiguousarray(bound_priority, dtype=np.int32).reshape(-1)
    ts = np.ascontiguousarray(bound_start_ns, dtype=np.int64).reshape(-1)
    th = None if bound_pdb_prio is None else np.ascontiguousarray(bound_pdb_prio, dtype=np.int32).reshape(-1)
    if len(pr) != n or len(ts) != n or (th is not None and len(th) != n):
        raise ValueError("row_preempt_pdb takes one priority, one start time and one threshold per bound row")
    q = None if quotas is None else np.ascontiguousarray(quotas, dtype=nat.QUOTA).reshape(-1)
    status = ctypes.c_int32(0)
    mask = np.zeros(2, dtype=np.uint64)
    stats = np.zeros(5, dtype=np.int64)
    if th is not None and n == 0:
        th = np.zeros(1, dtype=np.int32)   # (a non-null pointer: an empty list still runs the PDB form)
    _check(nat.lib().kg_row_preempt_pdb(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(rows) if n else None,
                                        nat.ptr(pr) if n else None, nat.ptr(ts) if n else None,
                                        nat.ptr(th) if th is not None else None, n, nat.ptr(pod_row), int(pod_priority),
                                        nat.ptr(q) if q is not None and len(q) else None, 0 if q is None else len(q),
                                        int(now_ns), ctypes.byref(status), nat.ptr(mask), nat.ptr(stats)),
           what="kg_row_preempt_pdb")
    return {"status": int(status.value), "victims": unpack_victims(mask), "n_victims": int(stats[0]),
            "hi_prio": int(stats[1]), "prio_sum": int(stats[2]), "earliest_ns": int(stats[3]), "n_violating": int(stats[4])}


def pdb_thresholds(priority, start_ns, quota, non_preemptible, pdb_first, pdb_ids, allowed) -> np.ndarray:
    """kg_pdb_thresholds: the PDB thresholds of one node's bound list (caller order).  Pod b decrements the PDBs
    pdb_ids[pdb_first[b]:pdb_first[b + 1]] (indices into `allowed`, the PDBs' Status.DisruptionsAllowed).  Returns
    int32 [n]: pod b is PDB-violating for a preemptor of priority P  <=>  out[b] < P (nat.PDB_PRIO_NONE: never)."""
    pr = np.ascontiguousarray(priority, dtype=np.int32).reshape(-1)
    n = len(pr)
    ts = np.ascontiguousarray(start_ns, dtype=np.int64).reshape(-1)
    qg = np.ascontiguousarray(quota, dtype=np.int32).reshape(-1)
    npre = np.ascontiguousarray(non_preemptible, dtype=np.uint8).reshape(-1)
    pf = np.ascontiguousarray(pdb_first, dtype=np.int32).reshape(-1)
    ids = np.ascontiguousarray(pdb_ids, dtype=np.int32).reshape(-1)
    al = np.ascontiguousarray(allowed, dtype=np.int32).reshape(-1)
    if len(ts) != n or len(qg) != n or len(npre) != n or len(pf) != n + 1:
        raise ValueError("pdb_thresholds takes one start time, quota and flag per pod and n + 1 offsets")
    out = np.zeros(n, dtype=np.int32)
    _check(nat.lib().kg_pdb_thresholds(nat.ptr(pr) if n else None, nat.ptr(ts) if n else None, nat.ptr(qg) if n else None,
                                       nat.ptr(npre) if n else None, n, nat.ptr(pf), nat.ptr(ids) if len(ids) else None,
                                       nat.ptr(al) if len(al) else None, len(al), nat.ptr(out) if n else None),
           what="kg_pdb_thresholds")
    return out


def unpack_victims(words: np.ndarray) -> np.ndarray:
    """Victim mask words uint64 [..., 2] -> bool [..., nat.BOUND_MAX_PER_NODE] (bit b: position b of the node's list)."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(*w.shape[:-1], 16), axis=-1, bitorder="little")
    return bits.astype(bool)


def _pick_dict(pick: np.ndarray) -> dict:
    """kg_preempt's pick words int64 [n][8] as named arrays (word 1: n_victims | n_violating << 32)."""
    pick = np.ascontiguousarray(pick, dtype=np.int64).reshape(-1, nat.PREEMPT_PICK_WORDS)
    return {"node": pick[:, 0].astype(np.int32), "victims": unpack_victims(pick[:, 5:7].view(np.uint64)),
            "n_victims": (pick[:, 1] & 0xFFFFFFFF).astype(np.int32), "n_violating": (pick[:, 1] >> 32).astype(np.int32),
            "hi_prio": pick[:, 2].astype(np.int32), "prio_sum": pick[:, 3].copy(),
            "earliest_ns": pick[:, 4].copy(), "n_candidates": pick[:, 7].astype(np.int32), "pick": pick}


# the reference's reason strings: upstream NodeResourcesFit ("Too many pods", "Insufficient <resource>"),
# LoadAwareScheduling (load_aware.go:45, resource not named: the word holds the plugin's verdict alone) and
# NodeNUMAResource (frameworkext/topologymanager/manager.go:70)
REASON_ABSENT = "node(s) not in the snapshot"
REASON_ELIG = "node(s) didn't match the pod's eligibility class"
REASON_FIT_PODS = "Too many pods"
REASON_LOADAWARE = "node(s) usage exceed threshold"
REASON_NUMA = "node(s) NUMA Topology affinity error"


def resource_names(cfg: np.ndarray) -> list:
    """The name of each resource id: the fixed ones, then the named slots from ext_resource_names."""
    ext = [bytes(b).split(b"\0")[0].decode() for b in np.asarray(cfg["ext_resource_names"]).reshape(-1)]
    return list(nat.FIXED_RES_NAMES) + [n or f"ext{i}" for i, n in enumerate(ext)]


def why_names(cfg: np.ndarray, word: int) -> list:
    """The reference's reason strings of a reason word (or of a counts slot index via 1 << slot), in the filter
    order: absent, eligibility, NodeResourcesFit ("Too many pods", "Insufficient <resource>" per failing resource,
    the named slots by their ext_resource_names), LoadAwareScheduling, NodeNUMAResource."""
    word = int(word)
    out = []
    if word & nat.WHY_ABSENT:
        out.append(REASON_ABSENT)
    if word & nat.WHY_ELIG:
        out.append(REASON_ELIG)
    if word & nat.WHY_FIT_PODS:
        out.append(REASON_FIT_PODS)
    names = resource_names(cfg)
    for r in range(nat.NUM_RES):
        if word & nat.WHY_FIT_RES(r):
            out.append("Insufficient " + names[r])
    if word & nat.WHY_LOADAWARE:
        out.append(REASON_LOADAWARE)
    if word & nat.WHY_NUMA:
        out.append(REASON_NUMA)
    return out


def why_histogram(cfg: np.ndarray, counts_row) -> str:
    """One pod's counts as the FailedScheduling event lists them: "312 Insufficient cpu, 97 Too many pods, ..."."""
    parts = []
    for b in range(nat.WHY_SLOT_REJECTED):
        c = int(counts_row[b])
        if c:
            parts += [f"{c} {s}" for s in why_names(cfg, 1 << b)]
    return ", ".join(parts)


def row_eval_rsv(cfg: np.ndarray, node_row: np.ndarray, rsv: np.ndarray, pod_row: np.ndarray, now_ns: int):
    """(feasible, fit, la, numa, raw, order, nominated) of one pair with the node's reservation slots
    (host rows)."""
    rsv = np.ascontiguousarray(rsv, dtype=nat.RESERVATION)
    f, a, b, n, r, nm = (ctypes.c_int32() for _ in range(6))
    o = ctypes.c_int64()
    _check(nat.lib().kg_row_eval_rsv(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(rsv) if len(rsv) else None, len(rsv),
                                     nat.ptr(pod_row), int(now_ns), ctypes.byref(f), ctypes.byref(a), ctypes.byref(b),
                                     ctypes.byref(n), ctypes.byref(r), ctypes.byref(o), ctypes.byref(nm)),
           what="kg_row_eval_rsv")
    return bool(f.value), a.value, b.value, n.value, r.value, o.value, nm.value


def row_rsv_restore(cfg: np.ndarray, node_row: np.ndarray, rsv: np.ndarray, pod_row: np.ndarray) -> np.ndarray:
    """The Reservation restore of one pair (kg_row_rsv_restore): a RSV_RESTORED record."""
    rsv = np.ascontiguousarray(rsv, dtype=nat.RESERVATION)
    out = np.zeros((), dtype=nat.RSV_RESTORED)
    _check(nat.lib().kg_row_rsv_restore(nat.ptr(cfg), nat.ptr(node_row), nat.ptr(rsv) if len(rsv) else None, len(rsv),
                                        nat.ptr(pod_row), nat.ptr(out)), what="kg_row_rsv_restore")
    return out


def batch_slot_map(cfg: np.ndarray, pod_rows: np.ndarray):
    """kg_batch_slot_map: the slot map set_pods chooses for the batch, on the host alone.  Returns (n_slots,
    slot_res, spill): 2, 4 or 8; the resource id of each of the 8 slots (−1 unused); and a bool per pod, True for
    the spill pods (pods that need a resource outside the map: only when the batch needs more than 8 resources)."""
    rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
    n_slots = ctypes.c_int32(0)
    slot_res = np.full(8, -1, dtype=np.int32)
    spill = np.zeros(max(len(rows), 1), dtype=np.uint8)
    _check(nat.lib().kg_batch_slot_map(nat.ptr(cfg), nat.ptr(rows) if len(rows) else None, len(rows),
                                       ctypes.addressof(n_slots), nat.ptr(slot_res), nat.ptr(spill)),
           what="kg_batch_slot_map")
    return int(n_slots.value), slot_res, spill[:len(rows)].astype(bool)


class Engine:
    """One engine = one GPU, one HIP stream, one HBM-resident node snapshot."""

    def __init__(self, cfg: np.ndarray):
        self.cfg = cfg.copy()
        self._h = ctypes.c_void_p()
        _check(nat.lib().kg_engine_create(nat.ptr(self.cfg), ctypes.byref(self._h)), what="kg_engine_create")
        self.n_nodes = 0
        self.n_pods = 0

    # lifecycle --------------------------------------------------------------------------
    def close(self) -> None:
        if self._h:
            nat.lib().kg_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_ptr: int) -> None:
        _check(nat.lib().kg_set_stream(self._h, ctypes.c_void_p(stream_ptr)), self, "kg_set_stream")

    def sync(self) -> None:
        _check(nat.lib().kg_sync(self._h), self, "kg_sync")

    # snapshot ---------------------------------------------------------------------------
    def load_snapshot(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=nat.NODE_ROW)
        _check(nat.lib().kg_snapshot_reset(self._h, len(rows)), self, "kg_snapshot_reset")
        self.n_nodes = len(rows)
        self.shard = (0, len(rows))
        self.upsert(np.arange(len(rows), dtype=np.int32), rows)

    def upsert(self, idx, rows: np.ndarray) -> None:
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=nat.NODE_ROW)
        _check(nat.lib().kg_snapshot_upsert(self._h, nat.ptr(idx), nat.ptr(rows), len(idx)), self, "kg_snapshot_upsert")

    def set_cpus(self, view, view_index: Optional[Sequence[int]] = None,
                 snap_index: Optional[Sequence[int]] = None) -> None:
        """kg_cpus_set: snapshot node snap_index[k] takes the CPU detail of view node view_index[k] (both
        default to k over every view node); other nodes keep their tables."""
        n = len(view.nodes) if view_index is None else len(view_index)
        vi = None if view_index is None else np.ascontiguousarray(view_index, dtype=np.int32)
        si = None if snap_index is None else np.ascontiguousarray(snap_index, dtype=np.int32)
        _check(nat.lib().kg_cpus_set(self._h, ctypes.byref(view.c_view), nat.ptr(vi), nat.ptr(si), n), self,
               "kg_cpus_set")

    def download_cpus(self, node: int, n_cpus: int) -> np.ndarray:
        out = np.zeros(n_cpus, dtype=nat.CPU_INFO)
        _check(nat.lib().kg_cpus_download(self._h, int(node), nat.ptr(out), n_cpus), self, "kg_cpus_download")
        return out

    def remove(self, i: int) -> None:
        _check(nat.lib().kg_snapshot_remove(self._h, int(i)), self, "kg_snapshot_remove")

    def download(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = self.n_nodes - first if n is None else n
        out = np.zeros(n, dtype=nat.NODE_ROW)
        _check(nat.lib().kg_snapshot_download(self._h, first, n, nat.ptr(out)), self, "kg_snapshot_download")
        return out

    def generation(self) -> int:
        """kg_snapshot_generation: successful snapshot mutations so far; raises once the state is stale."""
        g = ctypes.c_uint64(0)
        _check(nat.lib().kg_snapshot_generation(self._h, ctypes.byref(g)), self, "kg_snapshot_generation")
        return int(g.value)

    def set_shard(self, begin: int, end: int) -> None:
        _check(nat.lib().kg_set_shard(self._h, begin, end), self, "kg_set_shard")
        self.shard = (begin, end)

    def set_profiling(self, on: bool = True) -> None:
        _check(nat.lib().kg_set_profiling(self._h, int(on)), self, "kg_set_profiling")

    def eval_kernel_times(self, n: int = 256) -> np.ndarray:
        """Durations (ms) of the last ≤ n profiled k_eval launches, oldest first."""
        ms = np.zeros(n, dtype=np.float32)
        k = nat.lib().kg_eval_kernel_times(self._h, nat.ptr(ms), n)
        if k < 0:
            _check(k, self, "kg_eval_kernel_times")
        return ms[:k].astype(np.float64)

    @property
    def num_tiles(self) -> int:
        return nat.lib().kg_num_tiles(self._h)

    partial_slots = nat.PARTIAL_SLOTS   # uint32 per (pod, tile) of kg_place_chunk_eval's buffer

    # pods -------------------------------------------------------------------------------
    def set_pods(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=nat.POD_ROW)
        _check(nat.lib().kg_pods_set(self._h, nat.ptr(rows), len(rows)), self, "kg_pods_set")
        self.n_pods = len(rows)
        self._pod_rows = rows.copy() if debug.debug_top_n() else None  # the debug dump's reason lines (_why_line)

    def spill_count(self) -> int:
        """kg_pods_spill_count: pods of the uploaded batch outside its slot map (batch_slot_map), evaluated on the
        generic pair path."""
        return int(nat.lib().kg_pods_spill_count(self._h))

    def restricted_count(self) -> int:
        """kg_pods_restricted_count: pods of the uploaded batch with elig_class != 0."""
        return int(nat.lib().kg_pods_restricted_count(self._h))

    # node eligibility classes ---------------------------------------------------------------
    def set_eligibility(self, masks) -> None:
        """kg_elig_set: replace the eligibility table.  `masks`: bool [K][n_nodes] (True: the node is eligible for the
        class), or the packed form uint64 [K][ceil(n_nodes / 64)] (bit n % 64 of word n // 64); None or K = 0 drops
        the table.  A pod row with elig_class = k ≥ 1 may then only run on the nodes of class k − 1."""
        words = (self.n_nodes + 63) // 64
        if masks is None:
            packed = np.zeros((0, words), dtype=np.uint64)
        else:
            masks = np.asarray(masks)
            if masks.dtype == np.uint64:
                packed = np.ascontiguousarray(masks).reshape(-1, words) if masks.size else np.zeros((0, words), np.uint64)
            else:
                packed = pack_eligibility(masks.reshape(-1, self.n_nodes) if masks.size else masks.reshape(0, self.n_nodes))
        _check(nat.lib().kg_elig_set(self._h, nat.ptr(packed) if packed.size else None, len(packed), self.n_nodes), self,
               "kg_elig_set")

    def update_eligibility(self, cls: int, nodes, eligible) -> None:
        """kg_elig_update: set (True) or clear (False) the bits of `nodes` in class `cls` (a node event)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        el = np.ascontiguousarray(np.broadcast_to(np.asarray(eligible, dtype=bool), nodes.shape), dtype=np.uint8)
        _check(nat.lib().kg_elig_update(self._h, int(cls), nat.ptr(nodes) if len(nodes) else None,
                                        nat.ptr(el) if len(nodes) else None, len(nodes)), self, "kg_elig_update")

    # evaluation -------------------------------------------------------------------------
    @property
    def mask_words(self) -> int:
        return (self.shard[1] - self.shard[0] + 63) // 64

    @property
    def score_stride(self) -> int:
        return self.mask_words * 64

    def eval(self, now_ns: int, mask: bool = True, scores: bool = True, top1: bool = True,
             numa_scores: Optional[bool] = None, rsv_scores: Optional[bool] = None) -> dict:
        """Matrix mode into host arrays: mask [P][words] u64, scores [P][stride][2] u8, top1 [P] u64,
        numa_scores [P][stride] u8 (by default when NodeNUMAResource is enabled), rsv_scores [P][stride]
        u8 (normalized Reservation score, by default when Reservation is enabled)."""
        P = self.n_pods
        res = {}
        out = nat.EvalOut()
        if mask:
            res["mask"] = np.zeros((P, self.mask_words), dtype=np.uint64)
            out.mask = res["mask"].ctypes.data
        if scores:
            res["scores"] = np.zeros((P, self.score_stride, 2), dtype=np.uint8)
            out.scores = res["scores"].ctypes.data
        if top1:
            res["top1"] = np.zeros(P, dtype=np.uint64)
            out.top1 = res["top1"].ctypes.data
        if numa_scores is None:
            numa_scores = bool(int(self.cfg["enabled_plugins"]) & nat.PLUGIN_NUMA)
        if numa_scores:
            res["numa_scores"] = np.zeros((P, self.score_stride), dtype=np.uint8)
            out.numa_scores = res["numa_scores"].ctypes.data
        if rsv_scores is None:
            rsv_scores = bool(int(self.cfg["enabled_plugins"]) & nat.PLUGIN_RESERVATION)
        if rsv_scores:
            res["rsv_scores"] = np.zeros((P, self.score_stride), dtype=np.uint8)
            out.rsv_scores = res["rsv_scores"].ctypes.data
        out.out_on_device = 0
        _check(nat.lib().kg_eval(self._h, int(now_ns), ctypes.byref(out)), self, "kg_eval")
        top_n = debug.debug_top_n()   # --debug-scores (frameworkext/debug.go:32-48)
        if top_n:
            debug.dump_eval(self.cfg, res, min(self.n_nodes, self.score_stride), top_n,
                            reasons=lambda p: self._why_line(p, now_ns))
        return res

    def _why_line(self, pod: int, now_ns: int) -> str:
        """The reason histogram of pod `pod` of the uploaded batch (the debug dump's line for a pod without a
        feasible node); empty where kg_diagnose does not answer (reservation slots, cpuset binding)."""
        rows = getattr(self, "_pod_rows", None)
        if rows is None or pod >= len(rows):
            return ""
        try:
            got = self.diagnose(rows[pod:pod + 1], now_ns)
        except EngineError:
            return ""
        parts = [why_histogram(self.cfg, got["counts"][0])]
        if got["pod_why"][0] & nat.WHY_POD_QUOTA:
            parts.append("the pod's quota is exceeded")
        if got["pod_why"][0] & nat.WHY_POD_RSV_REQUIRED:
            parts.append("the pod requires a reservation and none is loaded")
        return ", ".join(p for p in parts if p)

    def eval_device(self, now_ns: int, mask_ptr: int = 0, scores_ptr: int = 0, top1_ptr: int = 0,
                    numa_ptr: int = 0, rsv_ptr: int = 0) -> None:
        """Matrix mode into caller-owned device buffers (16-byte aligned, any previous content: every requested
        plane is written whole over its in-range cells and the mask's pad bits); asynchronous on the engine stream."""
        out = nat.EvalOut()
        out.mask, out.scores, out.top1, out.out_on_device = mask_ptr or None, scores_ptr or None, top1_ptr or None, 1
        out.numa_scores, out.rsv_scores = numa_ptr or None, rsv_ptr or None
        _check(nat.lib().kg_eval(self._h, int(now_ns), ctypes.byref(out)), self, "kg_eval")

    @staticmethod
    def comm_unique_id() -> bytes:
        """An RCCL unique id for kg_comm_init (one rank makes it, every rank passes it)."""
        buf = ctypes.create_string_buffer(nat.COMM_ID_BYTES)
        st = nat.lib().kg_comm_unique_id(buf)
        if st != 0:
            raise EngineError(f"kg_comm_unique_id failed ({st})")
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes) -> None:
        buf = ctypes.create_string_buffer(bytes(unique_id), nat.COMM_ID_BYTES)
        _check(nat.lib().kg_comm_init(self._h, int(rank), int(world), buf), self, "kg_comm_init")

    def comm_init_loopback(self, rank: int, world: int, name: str) -> None:
        """kg_comm_init_loopback: the ranks merge partial keys through the host shared-memory segment `name`
        (the same "/…" on every rank) instead of RCCL — several ranks on one GPU run kg_place_sharded's own loop."""
        _check(nat.lib().kg_comm_init_loopback(self._h, int(rank), int(world), name.encode()), self,
               "kg_comm_init_loopback")

    def comm_kind(self) -> str:
        return {nat.COMM_NONE: "none", nat.COMM_RCCL: "rccl", nat.COMM_LOOPBACK: "loopback"}[nat.lib().kg_comm_kind(self._h)]

    def place_sharded(self, now_ns: int):
        """kg_place over the ranks' node shards (kg_place_sharded): per chunk one max-merge of the partial keys over
        the communicator (RCCL or loopback), the resolve and host Reserve steps replicated.  Same outputs as place()."""
        P = self.n_pods
        nodes = np.zeros(P, dtype=np.int32)
        scores = np.zeros(P, dtype=np.int64)
        _check(nat.lib().kg_place_sharded(self._h, int(now_ns), nat.ptr(nodes), nat.ptr(scores)), self,
               "kg_place_sharded")
        return nodes, scores

    def set_forms(self, forms: int) -> None:
        """Force size-chosen kernel forms (nat.FORM_*; 0 = by size), for parity tests on small clusters."""
        _check(nat.lib().kg_set_forms(self._h, int(forms)), self, "kg_set_forms")

    def eval_host(self, now_ns: int, mask_ptr: int = 0, scores_ptr: int = 0, top1_ptr: int = 0,
                  numa_ptr: int = 0, rsv_ptr: int = 0) -> None:
        """Matrix mode into caller-owned host buffers (e.g. pinned memory): the outputs the Go plugins read
        (INTEGRATION.md `Eval`), copied back over PCIe before the call returns."""
        out = nat.EvalOut()
        out.mask, out.scores, out.top1, out.out_on_device = mask_ptr or None, scores_ptr or None, top1_ptr or None, 0
        out.numa_scores, out.rsv_scores = numa_ptr or None, rsv_ptr or None
        _check(nat.lib().kg_eval(self._h, int(now_ns), ctypes.byref(out)), self, "kg_eval")

    def place(self, now_ns: int):
        P = self.n_pods
        nodes = np.zeros(P, dtype=np.int32)
        scores = np.zeros(P, dtype=np.int64)
        _check(nat.lib().kg_place(self._h, int(now_ns), nat.ptr(nodes), nat.ptr(scores)), self, "kg_place")
        return nodes, scores

    def place_gangs(self, now_ns: int, pod_gang, gang_min, gang_flags, gang_group=None, release_waiting: bool = False):
        """kg_place_gangs: place() with Coscheduling's Strict-mode rejection inside the batch.  `pod_gang`: int32 [P], the
        gang of each pod of the uploaded batch (-1: none); `gang_min`: int32 [n_gangs], the members the batch must
        still place; `gang_flags`: uint8 [n_gangs], nat.GANG_STRICT or 0; `gang_group`: int32 [n_gangs] or None (every
        gang its own group); `release_waiting`: roll the WAITING groups back (the Permit timeout).  Returns
        (nodes, scores, verdicts): verdicts uint8 [n_gangs] of nat.GANG_ALLOWED / GANG_WAITING / GANG_REJECTED."""
        P = self.n_pods
        pg = np.ascontiguousarray(pod_gang, dtype=np.int32).reshape(-1)
        if len(pg) != P:
            raise ValueError("place_gangs takes one gang index per pod of the batch")
        gm = np.ascontiguousarray(gang_min, dtype=np.int32).reshape(-1)
        gf = np.ascontiguousarray(gang_flags, dtype=np.uint8).reshape(-1)
        ng = len(gm)
        gg = None if gang_group is None else np.ascontiguousarray(gang_group, dtype=np.int32).reshape(-1)
        if len(gf) != ng or (gg is not None and len(gg) != ng):
            raise ValueError("gang_min, gang_flags and gang_group describe the same gangs")
        nodes = np.zeros(P, dtype=np.int32)
        scores = np.zeros(P, dtype=np.int64)
        verdicts = np.zeros(ng, dtype=np.uint8)
        _check(nat.lib().kg_place_gangs(self._h, int(now_ns), nat.ptr(pg) if P else None, nat.ptr(gm) if ng else None,
                                        nat.ptr(gg) if ng else None, nat.ptr(gf) if ng else None, ng,
                                        nat.PLACE_GANG_RELEASE_WAITING if release_waiting else 0,
                                        nat.ptr(nodes) if P else None, nat.ptr(scores) if P else None,
                                        nat.ptr(verdicts) if ng else None), self, "kg_place_gangs")
        return nodes, scores, verdicts

    def chunk_eval(self, now_ns: int, pod_begin: int, n: int, partial_ptr: int) -> None:
        _check(nat.lib().kg_place_chunk_eval(self._h, int(now_ns), pod_begin, n, ctypes.c_void_p(partial_ptr)), self,
               "kg_place_chunk_eval")

    def chunk_resolve(self, now_ns: int, pod_begin: int, n: int, partial_ptr: int, node_ptr: int,
                      score_ptr: int, prev_ptr: int = 0, n_prev: int = 0) -> None:
        """kg_place_chunk_resolve; with prev_ptr / n_prev the pipelined form kg_place_chunk_resolve_prev (the
        previous chunk's placements, device int32, re-scored like touched nodes)."""
        if n_prev:
            _check(nat.lib().kg_place_chunk_resolve_prev(self._h, int(now_ns), pod_begin, n, ctypes.c_void_p(partial_ptr),
                                                         ctypes.c_void_p(node_ptr), ctypes.c_void_p(score_ptr),
                                                         ctypes.c_void_p(prev_ptr), n_prev), self,
                   "kg_place_chunk_resolve_prev")
            return
        _check(nat.lib().kg_place_chunk_resolve(self._h, int(now_ns), pod_begin, n, ctypes.c_void_p(partial_ptr),
                                                ctypes.c_void_p(node_ptr), ctypes.c_void_p(score_ptr)), self,
               "kg_place_chunk_resolve")

    def set_eval_stream(self, hip_stream: int) -> None:
        """kg_set_eval_stream: chunk evaluations launch on this stream (0 ⇒ the engine stream)."""
        _check(nat.lib().kg_set_eval_stream(self._h, ctypes.c_void_p(hip_stream or None)), self, "kg_set_eval_stream")

    def counters(self) -> dict:
        """kg_counters_get as a dict (evals, out_bytes, resolved, placed, h2d_bytes, kernel_ns, ...)."""
        out = np.zeros(1, dtype=nat.COUNTERS)
        _check(nat.lib().kg_counters_get(self._h, nat.ptr(out)), self, "kg_counters_get")
        return {k: int(out[k][0]) for k in nat.COUNTERS.names}

    def reset_counters(self) -> None:
        _check(nat.lib().kg_counters_reset(self._h), self, "kg_counters_reset")

    def commit(self, pod: int, node: int) -> bool:
        """kg_commit; False ⇔ the Reserve failed (a cpuset the accumulator cannot take; nothing changed)."""
        st = nat.lib().kg_commit(self._h, pod, node)
        if st == nat.NOT_FOUND:
            return False
        _check(st, self, "kg_commit")
        return True

    def unreserve(self, pod_rows: np.ndarray, nodes, zone_release=None, rsv_slot=None) -> np.ndarray:
        """kg_unreserve: entry i undoes the Reserve of pod_rows[i] on nodes[i] (at most nat.UNRESERVE_MAX entries; the
        rows travel with the call, the batch of set_pods is not touched).  `zone_release`: int64 [n][MAX_ZONES][2], the
        pods' recorded zone allocations (row_numa_alloc), or None; `rsv_slot`: int32 [n], the set_reservations index
        each Reserve nominated (row_eval_rsv) or -1, or None.  Returns bool [n]: the entries released (a node is
        all-or-nothing: a removed node, one that holds fewer pods than the call releases, or an invalid slot)."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        n = len(rows)
        nd = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        if len(nd) != n:
            raise ValueError("unreserve takes one node per pod row")
        zr = None if zone_release is None else np.ascontiguousarray(zone_release, dtype=np.int64).reshape(n, nat.MAX_ZONES, 2)
        sl = None if rsv_slot is None else np.ascontiguousarray(rsv_slot, dtype=np.int32).reshape(n)
        out = np.zeros(n, dtype=np.uint8)
        _check(nat.lib().kg_unreserve(self._h, nat.ptr(rows) if n else None, nat.ptr(nd) if n else None, n, 0,
                                      nat.ptr(zr) if n else None, nat.ptr(sl) if n else None,
                                      nat.ptr(out) if n else None), self, "kg_unreserve")
        return out.astype(bool)

    def cycle_one(self, pod_row: np.ndarray, now_ns: int, commit: bool = True, planes: bool = False) -> dict:
        """kg_cycle_one: the scheduling cycle of one pod (Filter + Score over the shard, selectHost and, with
        `commit`, the Reserve of the chosen node) in one launch; the batch of set_pods is not touched.
        Returns node (−1: none), score (−1: none), key (eval()'s top1 key) and committed; with `planes` also mask
        [1][words] u64, scores [1][stride][2] u8 and numa_scores [1][stride] u8 of the snapshot before the commit.
        Raises EngineError (KG_ERR_UNSUPPORTED) for what the fused launch does not answer — reservation slots,
        ElasticQuota, cpuset binding: those callers keep set_pods + eval + commit."""
        row = np.ascontiguousarray(pod_row, dtype=nat.POD_ROW).reshape(-1)
        if len(row) != 1:
            raise ValueError("cycle_one takes exactly one pod row")
        res = {}
        out = nat.CycleOut()
        eo = None
        if planes:
            eo = nat.EvalOut()
            res["mask"] = np.zeros((1, self.mask_words), dtype=np.uint64)
            res["scores"] = np.zeros((1, self.score_stride, 2), dtype=np.uint8)
            res["numa_scores"] = np.zeros((1, self.score_stride), dtype=np.uint8)
            eo.mask, eo.scores, eo.numa_scores = (res[k].ctypes.data for k in ("mask", "scores", "numa_scores"))
            eo.out_on_device = 0
        _check(nat.lib().kg_cycle_one(self._h, nat.ptr(row), int(now_ns), nat.CYCLE_COMMIT if commit else 0,
                                      ctypes.byref(eo) if eo is not None else None, ctypes.byref(out)), self,
               "kg_cycle_one")
        res.update(node=int(out.node), score=int(out.score), key=int(out.key), committed=bool(out.committed))
        return res

    def cycle_one_host(self, pod_row: np.ndarray, now_ns: int, commit: bool = True, mask_ptr: int = 0,
                       scores_ptr: int = 0, numa_ptr: int = 0) -> "nat.CycleOut":
        """kg_cycle_one with the planes in caller-owned host buffers (e.g. pinned memory, as eval_host): what the
        Go plugins' per-pod loop calls (INTEGRATION.md `CycleOne`).  `pod_row`: a POD_ROW array of one row."""
        out = nat.CycleOut()
        eo = None
        if mask_ptr or scores_ptr or numa_ptr:
            eo = nat.EvalOut()
            eo.mask, eo.scores, eo.numa_scores, eo.out_on_device = mask_ptr or None, scores_ptr or None, numa_ptr or None, 0
        _check(nat.lib().kg_cycle_one(self._h, nat.ptr(pod_row), int(now_ns), nat.CYCLE_COMMIT if commit else 0,
                                      ctypes.byref(eo) if eo is not None else None, ctypes.byref(out)), self,
               "kg_cycle_one")
        return out

    def cycle_one_device(self, pod_row: np.ndarray, now_ns: int, commit: bool = False, mask_ptr: int = 0,
                         scores_ptr: int = 0, numa_ptr: int = 0, top1_ptr: int = 0) -> "nat.CycleOut":
        """kg_cycle_one with the planes (and the top1 key) in caller-owned device buffers, as eval_device."""
        out = nat.CycleOut()
        eo = nat.EvalOut()
        eo.mask, eo.scores, eo.numa_scores, eo.top1 = mask_ptr or None, scores_ptr or None, numa_ptr or None, top1_ptr or None
        eo.out_on_device = 1
        _check(nat.lib().kg_cycle_one(self._h, nat.ptr(pod_row), int(now_ns), nat.CYCLE_COMMIT if commit else 0,
                                      ctypes.byref(eo), ctypes.byref(out)), self, "kg_cycle_one")
        return out

    def diagnose(self, pod_rows: np.ndarray, now_ns: int, first_fail: bool = False, why: bool = False) -> dict:
        """kg_diagnose: why the pods (at most nat.DIAG_MAX_PODS rows; they travel with the call, the batch of
        set_pods is not touched) are rejected by the nodes of the shard, in one call.  Returns counts
        [n][nat.WHY_SLOTS] u32 (nodes per reason bit; slots 30 / 31: rejected / feasible nodes) and pod_why [n] u32
        (nat.WHY_POD_*), with `why` also the words [n][stride] u32 (columns as eval()'s planes).  `first_fail`: each
        word keeps the first failing group only (what the reference's NodeToStatusMap holds).  Mutates nothing."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        n = len(rows)
        res = {"counts": np.zeros((n, nat.WHY_SLOTS), dtype=np.uint32), "pod_why": np.zeros(n, dtype=np.uint32)}
        if why:
            res["why"] = np.zeros((n, self.score_stride), dtype=np.uint32)
        _check(nat.lib().kg_diagnose(self._h, nat.ptr(rows) if n else None, n, int(now_ns),
                                     nat.DIAG_FIRST_FAIL if first_fail else 0, nat.ptr(res["counts"]) if n else None,
                                     nat.ptr(res["pod_why"]) if n else None,
                                     nat.ptr(res["why"]) if why and res["why"].size else None, 0), self, "kg_diagnose")
        return res

    def diagnose_host(self, pod_rows: np.ndarray, now_ns: int, counts_ptr: int, pod_why_ptr: int = 0, why_ptr: int = 0,
                      first_fail: bool = False) -> None:
        """kg_diagnose into caller-owned host buffers (e.g. pinned memory, as eval_host): what the Go plugins'
        PostFilter calls (INTEGRATION.md `Diagnose`)."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        _check(nat.lib().kg_diagnose(self._h, nat.ptr(rows), len(rows), int(now_ns),
                                     nat.DIAG_FIRST_FAIL if first_fail else 0, counts_ptr or None, pod_why_ptr or None,
                                     why_ptr or None, 0), self, "kg_diagnose")

    def diagnose_device(self, pod_rows: np.ndarray, now_ns: int, counts_ptr: int, pod_why_ptr: int = 0, why_ptr: int = 0,
                        first_fail: bool = False) -> None:
        """kg_diagnose into caller-owned device buffers (16-byte aligned, any previous content), as eval_device; the
        call returns after the launches completed."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        _check(nat.lib().kg_diagnose(self._h, nat.ptr(rows), len(rows), int(now_ns),
                                     nat.DIAG_FIRST_FAIL if first_fail else 0, counts_ptr or None, pod_why_ptr or None,
                                     why_ptr or None, 1), self, "kg_diagnose")

    def candidates(self, pod_rows: np.ndarray, now_ns: int, k: int, scores: bool = True) -> dict:
        """kg_candidates: the k best feasible nodes of each pod (at most nat.CAND_MAX_PODS rows, 1 ≤ k ≤
        nat.CAND_MAX_K; the rows travel with the call, the batch of set_pods is not touched) over the shard, in one
        call.  Returns keys [n][k] u64 (eval()'s top1 encoding, strictly descending, 0 past the pod's feasible
        count), nodes [n][k] i32 (−1 where none), totals [n][k] i64 (−1 where none), n_feasible [n] u32 and, with
        `scores`, scores [n][k][4] u8 = {fit, loadaware, numa, 0}.  Mutates nothing."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        n, k = len(rows), int(k)
        kk = max(k, 0)
        res = {"keys": np.zeros((n, kk), dtype=np.uint64), "n_feasible": np.zeros(n, dtype=np.uint32)}
        if scores:
            res["scores"] = np.zeros((n, kk, 4), dtype=np.uint8)
        _check(nat.lib().kg_candidates(self._h, nat.ptr(rows) if n else None, n, int(now_ns), k, 0,
                                       nat.ptr(res["keys"]) if n else None,
                                       nat.ptr(res["scores"]) if scores and n else None,
                                       nat.ptr(res["n_feasible"]) if n else None, 0), self, "kg_candidates")
        node, total = decode_top1(res["keys"])
        res["nodes"], res["totals"] = node.astype(np.int32), total
        return res

    def candidates_device(self, pod_rows: np.ndarray, now_ns: int, k: int, keys_ptr: int, scores_ptr: int = 0,
                          n_feasible_ptr: int = 0) -> None:
        """kg_candidates into caller-owned device buffers (keys 8-byte aligned, the others 4-byte aligned, any
        previous content), as diagnose_device; the call returns after the launches completed."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        _check(nat.lib().kg_candidates(self._h, nat.ptr(rows), len(rows), int(now_ns), int(k), 0, keys_ptr or None,
                                       scores_ptr or None, n_feasible_ptr or None, 1), self, "kg_candidates")

    # preemption dry run ---------------------------------------------------------------------
    def set_bound_pods(self, first, rows: np.ndarray, priority, start_ns, max_per_node: int = nat.BOUND_MAX_PER_NODE) -> None:
        """kg_bound_set: replace the bound-pod table (NodeInfo.Pods of every snapshot node).  `first`: int32
        [n_nodes + 1] CSR offsets into `rows` (POD_ROW), `priority` (int32) and `start_ns` (int64,
        nat.START_NS_NONE for a pod without a start time); `max_per_node`: the slots kept per node (1..128)."""
        first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        if len(first) != self.n_nodes + 1:
            raise ValueError("set_bound_pods takes n_nodes + 1 offsets")
        rows = np.ascontiguousarray(rows, dtype=nat.POD_ROW).reshape(-1)
        pr = np.ascontiguousarray(priority, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(start_ns, dtype=np.int64).reshape(-1)
        if len(pr) != len(rows) or len(ts) != len(rows):
            raise ValueError("set_bound_pods takes one priority and one start time per row")
        n = len(rows)
        _check(nat.lib().kg_bound_set(self._h, nat.ptr(first), nat.ptr(rows) if n else None, nat.ptr(pr) if n else None,
                                      nat.ptr(ts) if n else None, int(max_per_node)), self, "kg_bound_set")
        self.bound_max = int(max_per_node)

    def update_bound_pods(self, node: int, rows: np.ndarray, priority, start_ns) -> None:
        """kg_bound_update: replace one node's list (empty arrays empty it).  The caller keeps the table in step with
        its pod events this way: place() / commit() / unreserve() do not touch it."""
        rows = np.ascontiguousarray(rows, dtype=nat.POD_ROW).reshape(-1)
        pr = np.ascontiguousarray(priority, dtype=np.int32).reshape(-1)
        ts = np.ascontiguousarray(start_ns, dtype=np.int64).reshape(-1)
        if len(pr) != len(rows) or len(ts) != len(rows):
            raise ValueError("update_bound_pods takes one priority and one start time per row")
        n = len(rows)
        _check(nat.lib().kg_bound_update(self._h, int(node), nat.ptr(rows) if n else None, nat.ptr(pr) if n else None,
                                         nat.ptr(ts) if n else None, n), self, "kg_bound_update")

    def download_bound_pods(self, node: int):
        """kg_bound_download: (rows, priority, start_ns) of one node's list in the caller's order.  A row carries the
        fields the table keeps (request, request_present, nonzero_request, numa_request, numa_request_present, quota,
        flags & POD_NON_PREEMPTIBLE); the others are zero."""
        cap = int(getattr(self, "bound_max", nat.BOUND_MAX_PER_NODE))
        rows = np.zeros(cap, dtype=nat.POD_ROW)
        pr = np.zeros(cap, dtype=np.int32)
        ts = np.zeros(cap, dtype=np.int64)
        n = ctypes.c_int32(0)
        _check(nat.lib().kg_bound_download(self._h, int(node), nat.ptr(rows), nat.ptr(pr), nat.ptr(ts), cap,
                                           ctypes.byref(n)), self, "kg_bound_download")
        return rows[:n.value].copy(), pr[:n.value].copy(), ts[:n.value].copy()

    def set_bound_pdb(self, first, pdb_prio) -> None:
        """kg_bound_pdb_set: load the PDB threshold plane (pdb_thresholds / ingest.bound_pdb), one int32 per bound pod in
        set_bound_pods' order with the same `first`; pdb_prio None drops the plane (preempt() then answers without
        PDBs again).  set_bound_pods and load_snapshot drop it too."""
        if pdb_prio is None:
            _check(nat.lib().kg_bound_pdb_set(self._h, None, None), self, "kg_bound_pdb_set")
            return
        first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
        if len(first) != self.n_nodes + 1:
            raise ValueError("set_bound_pdb takes n_nodes + 1 offsets")
        th = np.ascontiguousarray(pdb_prio, dtype=np.int32).reshape(-1)
        if len(th) != int(first[-1]):
            raise ValueError("set_bound_pdb takes one threshold per bound pod")
        if not len(th):
            th = np.zeros(1, dtype=np.int32)   # (a non-null pointer: an all-empty table still gets a plane)
        _check(nat.lib().kg_bound_pdb_set(self._h, nat.ptr(first), nat.ptr(th)), self, "kg_bound_pdb_set")

    def update_bound_pdb(self, node: int, pdb_prio) -> None:
        """kg_bound_pdb_update: replace one node's thresholds (as many as its list holds).  update_bound_pods resets the
        node's values to nat.PDB_PRIO_NONE; this call follows it."""
        th = np.ascontiguousarray(pdb_prio, dtype=np.int32).reshape(-1)
        n = len(th)
        _check(nat.lib().kg_bound_pdb_update(self._h, int(node), nat.ptr(th) if n else None, n), self, "kg_bound_pdb_update")

    def download_bound_pdb(self, node: int) -> np.ndarray:
        """kg_bound_pdb_download: one node's thresholds in the caller's order."""
        cap = int(getattr(self, "bound_max", nat.BOUND_MAX_PER_NODE))
        out = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_int32(0)
        _check(nat.lib().kg_bound_pdb_download(self._h, int(node), nat.ptr(out), cap, ctypes.byref(n)), self,
               "kg_bound_pdb_download")
        return out[:n.value].copy()

    def preempt(self, pod_rows: np.ndarray, priority, now_ns: int, plane: bool = False) -> dict:
        """kg_preempt: the preemption dry run of the pods (at most nat.PREEMPT_MAX_PODS rows with their priorities; they
        travel with the call, the batch of set_pods is not touched) against every node of the shard, and the node to
        preempt on.  Returns node [n] i32 (-1: no candidate), victims [n][128] bool (positions in the picked node's
        list), n_victims, hi_prio, prio_sum, earliest_ns, n_candidates and pick (the raw words, for merge_preempt);
        with `plane` also status / n_victims_plane / n_potential [n][stride] (columns as eval()'s planes).  With a PDB
        threshold plane loaded (set_bound_pdb) the violating potential victims are reprieved first and n_violating /
        n_violating_plane hold numViolatingVictim, the pick's criterion after "no victim"; both are zero without one.
        Mutates nothing."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        n = len(rows)
        pr = np.ascontiguousarray(priority, dtype=np.int32).reshape(-1)
        if len(pr) != n:
            raise ValueError("preempt takes one priority per pod row")
        pick = np.zeros((n, nat.PREEMPT_PICK_WORDS), dtype=np.int64)
        cells = np.zeros((n, self.score_stride), dtype=np.uint32) if plane else None
        _check(nat.lib().kg_preempt(self._h, nat.ptr(rows) if n else None, nat.ptr(pr) if n else None, n, int(now_ns), 0,
                                    nat.ptr(pick) if n else None,
                                    nat.ptr(cells) if plane and cells.size else None, 0), self, "kg_preempt")
        res = _pick_dict(pick)
        if plane:
            res["status"] = (cells & np.uint32(0xFF)).astype(np.uint8)
            res["n_victims_plane"] = ((cells >> np.uint32(8)) & np.uint32(0xFF)).astype(np.uint8)
            res["n_potential"] = ((cells >> np.uint32(16)) & np.uint32(0xFF)).astype(np.uint8)
            res["n_violating_plane"] = (cells >> np.uint32(24)).astype(np.uint8)
            res["plane"] = cells
        return res

    def preempt_device(self, pod_rows: np.ndarray, priority, now_ns: int, pick_ptr: int, plane_ptr: int = 0) -> None:
        """kg_preempt into caller-owned device buffers (pick 8-byte aligned, the plane 16-byte aligned, any previous
        content), as diagnose_device; the call returns after the launches completed."""
        rows = np.ascontiguousarray(pod_rows, dtype=nat.POD_ROW).reshape(-1)
        pr = np.ascontiguousarray(priority, dtype=np.int32).reshape(-1)
        _check(nat.lib().kg_preempt(self._h, nat.ptr(rows), nat.ptr(pr), len(rows), int(now_ns), 0, pick_ptr or None,
                                    plane_ptr or None, 1), self, "kg_preempt")

    # Reservation / ElasticQuota -----------------------------------------------------------
    def set_reservations(self, rsv: np.ndarray) -> None:
        rsv = np.ascontiguousarray(rsv, dtype=nat.RESERVATION)
        _check(nat.lib().kg_rsv_set(self._h, nat.ptr(rsv), len(rsv)), self, "kg_rsv_set")
        self.n_rsv = len(rsv)

    def download_reservations(self) -> np.ndarray:
        out = np.zeros(getattr(self, "n_rsv", 0), dtype=nat.RESERVATION)
        _check(nat.lib().kg_rsv_download(self._h, nat.ptr(out), len(out)), self, "kg_rsv_download")
        return out

    def set_quotas(self, q: np.ndarray) -> None:
        q = np.ascontiguousarray(q, dtype=nat.QUOTA)
        _check(nat.lib().kg_quota_set(self._h, nat.ptr(q), len(q)), self, "kg_quota_set")
        self.n_quota = len(q)

    def download_quotas(self) -> np.ndarray:
        out = np.zeros(getattr(self, "n_quota", 0), dtype=nat.QUOTA)
        _check(nat.lib().kg_quota_download(self._h, nat.ptr(out), len(out)), self, "kg_quota_download")
        return out


def decode_top1(keys: np.ndarray):
    """(total+1) << 32 | (0xFFFFFFFF − node) → (node or −1, total or −1)."""
    keys = np.asarray(keys, dtype=np.uint64)
    ok = keys != 0
    node = np.where(ok, (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64), -1)
    total = np.where(ok, (keys >> np.uint64(32)).astype(np.int64) - 1, -1)
    return node, total


def merge_candidates(results: Sequence[dict]) -> dict:
    """kg_candidates_merge: the candidates() results of several ranks or shards for the same pods and the same k,
    combined on the host.  Returns keys, nodes, totals, n_feasible (the sum over the disjoint shards) and, when every
    result carries them, scores.  Raises EngineError (KG_ERR_INVALID_ARG) for malformed or overlapping lists."""
    if not results:
        raise ValueError("merge_candidates takes at least one result")
    keys = np.ascontiguousarray(np.stack([np.asarray(r["keys"], dtype=np.uint64) for r in results]))
    _, n, k = keys.shape
    with_scores = all("scores" in r for r in results)
    sc = np.ascontiguousarray(np.stack([np.asarray(r["scores"], dtype=np.uint8) for r in results])) if with_scores else None
    res = {"keys": np.zeros((n, k), dtype=np.uint64)}
    if with_scores:
        res["scores"] = np.zeros((n, k, 4), dtype=np.uint8)
    _check(nat.lib().kg_candidates_merge(nat.ptr(keys), nat.ptr(sc), len(results), n, k, nat.ptr(res["keys"]),
                                         nat.ptr(res["scores"]) if with_scores else None), what="kg_candidates_merge")
    node, total = decode_top1(res["keys"])
    res["nodes"], res["totals"] = node.astype(np.int32), total
    res["n_feasible"] = np.sum([np.asarray(r["n_feasible"], dtype=np.uint32) for r in results], axis=0, dtype=np.uint32)
    return res


def merge_preempt(results: Sequence[dict]) -> dict:
    """kg_preempt_merge: the preempt() results of several ranks or shards for the same pods, combined on the host by
    the pick order (ties to the lowest node index); n_candidates is the sum over the shards."""
    if not results:
        raise ValueError("merge_preempt takes at least one result")
    picks = np.ascontiguousarray(np.stack([np.asarray(r["pick"], dtype=np.int64) for r in results]))
    _, n, _ = picks.shape
    out = np.zeros((n, nat.PREEMPT_PICK_WORDS), dtype=np.int64)
    _check(nat.lib().kg_preempt_merge(nat.ptr(picks), len(results), n, nat.ptr(out)), what="kg_preempt_merge")
    return _pick_dict(out)


def pack_eligibility(masks: np.ndarray) -> np.ndarray:
    """bool [K][n_nodes] → kg_elig_set's packed uint64 [K][ceil(n_nodes / 64)] (pad bits 0)."""
    masks = np.asarray(masks, dtype=bool)
    k, n = masks.shape
    words = (n + 63) // 64
    padded = np.zeros((k, words * 64), dtype=np.uint8)
    padded[:, :n] = masks
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint64).reshape(k, words)


def unpack_mask(mask: np.ndarray, n_nodes: int) -> np.ndarray:
    """[P][words] u64 → [P][n_nodes] bool."""
    b = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")
    return b[:, :n_nodes].astype(bool)
