"""Guarded device outputs for kg_eval / kg_cycle_one (tests/test_matrix_guard_gpu.py).

TEST INFRASTRUCTURE.  Every output plane gets a buffer of its own, laid out as [guard | payload | guard]: each guard
at least 64 KiB, the payload 256-byte aligned (as a hipMalloc would hand it out), the whole buffer filled with a prefill
byte.  The engine is handed the payload's address with out_on_device = 1; afterwards everything is copied back, so a
store outside a plane is read from the guards instead of landing in a neighbouring plane of the engine's scratch
(where the host path stages its outputs back to back) or faulting.  The buffers are uint8 tensors (torch has no
uint64); the host views them with numpy.

What the helper checks and what it leaves open: guards and unrequested planes must still hold the prefill; of a
requested plane the in-range cells (columns [0, width) of every row), the mask's pad bits (columns [width, 64·words)
of the last word, which must be 0) and top1 are specified.  The score and NUMA / Reservation pad columns
[width, 64·words) are unspecified (the kernels store whole vectors there) and are not compared.
"""
import numpy as np

GUARD = 64 * 1024
ALIGN = 256
PLANES = ("mask", "scores", "top1", "numa", "rsv")


def plane_bytes(n_pods, width):
    """Payload bytes of each plane for `n_pods` rows over `width` columns (include/koord_gpu.h kg_eval_out)."""
    words = (width + 63) // 64
    stride = words * 64
    return {"mask": n_pods * words * 8, "scores": n_pods * stride * 2, "top1": n_pods * 8, "numa": n_pods * stride,
            "rsv": n_pods * stride}


def total_bytes(nbytes):
    """Bytes to allocate for a payload of nbytes: both guards and the slack that aligns the payload."""
    return GUARD + ALIGN + nbytes + GUARD


def payload_offset(base_addr):
    """Offset of the payload in a buffer at base_addr: past the front guard, on the next ALIGN boundary."""
    return GUARD + (-(base_addr + GUARD)) % ALIGN


class GuardedPlane:
    def __init__(self, nbytes, prefill, device):
        import torch
        self.nbytes, self.prefill = int(nbytes), int(prefill)
        self.buf = torch.full((total_bytes(self.nbytes),), self.prefill, dtype=torch.uint8, device=device)
        self.off = payload_offset(self.buf.data_ptr())
        assert self.off >= GUARD and (self.buf.data_ptr() + self.off) % ALIGN == 0
        assert self.buf.numel() - self.off - self.nbytes >= GUARD

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def read(self):
        """(front guard, payload, back guard) as host uint8 arrays."""
        h = self.buf.cpu().numpy()
        return h[:self.off], h[self.off:self.off + self.nbytes].copy(), h[self.off + self.nbytes:]

    def stray(self, payload_too=False):
        """Offsets (relative to the payload) of the bytes outside the payload (of the whole buffer with
        `payload_too`) that no longer hold the prefill."""
        front, payload, back = self.read()
        bad = [np.flatnonzero(front != self.prefill) - self.off, self.nbytes + np.flatnonzero(back != self.prefill)]
        if payload_too:
            bad.append(np.flatnonzero(payload != self.prefill))
        return np.concatenate(bad)


class GuardedOutputs:
    """The five planes of one kg_eval over `n_pods` × `width`, each guarded; planes that a run does not request stay
    allocated and must come back untouched end to end."""

    def __init__(self, n_pods, width, prefill, device):
        self.n_pods, self.width = n_pods, width
        self.words = (width + 63) // 64
        self.stride = self.words * 64
        self.planes = {k: GuardedPlane(b, prefill, device) for k, b in plane_bytes(n_pods, width).items()}
        self.device = device

    def ptrs(self, request):
        return {k: (self.planes[k].ptr if k in request else 0) for k in PLANES}

    def eval(self, eng, now_ns, request):
        import torch
        torch.cuda.synchronize(self.device)   # the prefill is in place before the engine's stream starts
        p = self.ptrs(request)
        eng.eval_device(now_ns, mask_ptr=p["mask"], scores_ptr=p["scores"], top1_ptr=p["top1"], numa_ptr=p["numa"],
                        rsv_ptr=p["rsv"])
        eng.sync()
        return self.collect(request)

    def cycle_one(self, eng, pod_row, now_ns, request):
        import torch
        torch.cuda.synchronize(self.device)
        p = self.ptrs(request)
        out = eng.cycle_one_device(pod_row, now_ns, commit=False, mask_ptr=p["mask"], scores_ptr=p["scores"],
                                   numa_ptr=p["numa"], top1_ptr=p["top1"])
        eng.sync()
        return out, self.collect(request)

    def collect(self, request):
        """Asserts the guards of every plane and the whole buffer of every unrequested plane; returns the requested
        payloads shaped mask [P][words] u64, scores [P][stride][2] u8, top1 [P] u64, numa / rsv [P][stride] u8."""
        got = {}
        for k, pl in self.planes.items():
            bad = pl.stray(payload_too=k not in request)
            assert bad.size == 0, (f"{k} plane ({'requested' if k in request else 'not requested'}): {bad.size} bytes "
                                   f"outside the payload changed, the first at payload offset {int(bad[0])}")
            if k in request:
                got[k] = shape_payload(k, pl.read()[1], self.n_pods, self.words)
        return got


def shape_payload(kind, payload, n_pods, words):
    stride = words * 64
    if kind == "mask":
        return payload.view(np.uint64).reshape(n_pods, words)
    if kind == "scores":
        return payload.reshape(n_pods, stride, 2)
    if kind == "top1":
        return payload.view(np.uint64).reshape(n_pods)
    return payload.reshape(n_pods, stride)


def specified_cells(got, width):
    """The cells the contract specifies, for comparing two runs: whole mask words (pad bits included), top1, and
    columns [0, width) of the score, NUMA and Reservation planes."""
    out = {}
    for k, v in got.items():
        out[k] = v if k in ("mask", "top1") else v[:, :width]
    return out
