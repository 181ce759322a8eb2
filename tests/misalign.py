"""Device views at a chosen residue modulo 16 bytes, between sentinel pads (tests/test_gpu_misaligned*.py).

torch's allocator hands out addresses aligned to far more than 16 bytes, so a tensor passed as it comes only ever takes the aligned side of
the entry points' `(uintptr_t)p % 16` branches.  place() puts the data k elements after a 16-byte boundary inside a larger sentinel-filled
buffer, asserts the residue it meant to produce, and Placed.pads_ok() shows afterwards that nothing was written in front of or behind it."""
import numpy as np
import torch

DEVICE = "cuda"
PAD = 64                       # sentinel elements on each side (a multiple of 16 bytes at every element size)
SENT = 12345.678               # 4- and 8-byte floats
SENT16 = 0x5A5A                # 2-byte elements, as int16 payloads (bf16 / f16 / int16)
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
          np.dtype(np.int16): torch.int16, np.dtype(np.uint16): torch.int16, np.dtype(np.uint8): torch.uint8}


class Placed:
    def __init__(self, buf, view, k, shape, dtype, sent):
        self.buf, self.view, self.k, self.shape, self.dtype, self.sent = buf, view, k, shape, dtype, sent
        self.ptr = view.data_ptr()

    def get(self):
        """the view's contents now, in the shape and dtype of the array placed"""
        a = self.view.cpu().numpy()
        return (a.view(self.dtype) if a.dtype != self.dtype else a).reshape(self.shape).copy()

    def pads_ok(self):
        b = self.buf.cpu()
        lo, hi = b[:PAD + self.k], b[PAD + self.k + self.view.numel():]
        return bool((lo == self.sent).all()) and bool((hi == self.sent).all())

    def untouched(self):
        """every element, the view included, still holds the sentinel (an output of a refused call)"""
        return bool((self.buf.cpu() == self.sent).all())


def place(a, k=0, sentinel=False):
    """a: numpy array -> Placed whose view starts k elements (0..3 of 4 bytes, 0..7 of 2 bytes) after a 16-byte boundary.
    sentinel = True: the view itself is left as sentinels too (an output that a refused call must not touch)."""
    a = np.ascontiguousarray(a)
    size = a.dtype.itemsize
    assert 0 <= k * size < 16, (k, size)
    flat = a.reshape(-1)
    if a.dtype == np.uint16:
        flat = flat.view(np.int16)
    sent = SENT16 if size == 2 else 0x5A if size == 1 else int(SENT) if a.dtype.kind in "iu" else SENT
    slack = 16 // size                                            # room for every offset below 16 bytes
    buf = torch.full((PAD + flat.size + slack + PAD,), sent, dtype=_TORCH[a.dtype], device=DEVICE)
    assert buf.data_ptr() % 16 == 0 and (PAD * size) % 16 == 0
    view = buf[PAD + k: PAD + k + flat.size]
    if not sentinel:
        view.copy_(torch.from_numpy(flat))
    assert view.data_ptr() % 16 == k * size, (view.data_ptr() % 16, k, size)      # else the test would run the aligned route unnoticed
    return Placed(buf, view, k, a.shape, a.dtype, sent)


def bf16_round(a):
    """float32 -> the nearest bf16 value (ties to even), as float32: what (__bf16)x holds"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(a))


def bf16_bits(a):
    """float32 -> bf16 payloads (uint16), ties to even"""
    return (bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def bf16_value(bits):
    """bf16 payloads (uint16) -> float64"""
    return (np.ascontiguousarray(bits).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def max_rel(got, want):
    """max |got - want| / max |want|: the measure of tests/test_gpu_abi_ref.py"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.isfinite(got).all()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
