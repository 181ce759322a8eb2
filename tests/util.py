import contextlib

import torch


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    """global relative L2 error ||a-b|| / ||b|| (SURVEY 8d parity gate)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.is_complex() or b.is_complex():                      # complex spectra: as (re, im) pairs
        a, b = torch.view_as_real(a.resolve_conj().to(torch.complex128)), torch.view_as_real(b.resolve_conj().to(torch.complex128))
    a = a.double().flatten()
    b = b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def max_abs(a, b) -> float:
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def t(x, device="cuda"):
    import numpy as np
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.to(device).float().contiguous()


# ---------------------------------------------------------------- poisoned memory (tests/test_gpu_poison.py)
# Fill patterns: f32 quiet NaN, bf16 0x7FC0, f16 0x7E00, f64 NaN, integer and flag words 0xA5 bytes.  All comparisons are made on the integer view of
# the same width, so NaN == NaN and -0.0 != 0.0.
_BITS = {torch.float32: (torch.int32, 0x7FC00000), torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00),
         torch.float64: (torch.int64, 0x7FF8000000000000), torch.uint8: (torch.uint8, 0xA5), torch.int8: (torch.int8, 0xA5 - 256),
         torch.int16: (torch.int16, 0xA5A5 - (1 << 16)), torch.int32: (torch.int32, 0xA5A5A5A5 - (1 << 32)),
         torch.int64: (torch.int64, 0xA5A5A5A5A5A5A5A5 - (1 << 64))}


def bits(x: torch.Tensor) -> torch.Tensor:
    """the integer view of x (same element width)"""
    return x.view(_BITS[x.dtype][0])


def poison_(x: torch.Tensor) -> torch.Tensor:
    """fill x with its type's pattern -- for outputs and for scratch the callee is said to clear or to write in full"""
    bits(x).fill_(_BITS[x.dtype][1])
    return x


def has_poison(x: torch.Tensor) -> bool:
    return bool((bits(x) == _BITS[x.dtype][1]).any())


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def embed(x: torch.Tensor, lead: int = 64, trail: int = 64, row_pad: int = 0, fill: bool = True, device="cuda"):
    """Place the logical tensor x inside a larger allocation: `lead` elements in front, `trail` behind and, with row_pad > 0, rows (the last dimension)
    cols + row_pad elements apart -- the view is then 2-D [numel / cols, cols].  Everything outside the logical extent holds the type's fill pattern
    (fill = False: zeros -- the other run of a don't-care comparison).  Returns (view, check): check(what) asserts that every element outside the
    logical extent still holds what it held when embed() returned, compared as integers."""
    cols = x.shape[-1]
    rows = x.numel() // cols
    ld = cols + row_pad
    n = lead + rows * ld + trail
    buf = torch.zeros(n, dtype=x.dtype, device=device)
    if fill:
        poison_(buf)
    outside = torch.ones(n, dtype=torch.bool, device=device)
    if row_pad:
        view = buf.as_strided((rows, cols), (ld, 1), lead)
        outside.as_strided((rows, cols), (ld, 1), lead).fill_(False)
    else:
        view = buf[lead:lead + rows * cols].view(x.shape)
        outside[lead:lead + rows * cols] = False
    view.copy_(x)
    before = bits(buf).clone()

    def check(what=""):
        changed = (bits(buf) != before) & outside
        assert not bool(changed.any()), (f"{what}: {int(changed.sum())} elements outside the logical extent were written, the first at element "
                                         f"{int(changed.nonzero()[0])} of {n} (extent: {lead} + {rows} rows of {cols}, {ld} apart)")
    return view, check


def embed_out(shape, dtype=torch.float32, **kw):
    """an embedded OUTPUT: its logical extent is poisoned as well"""
    view, check = embed(torch.zeros(shape, dtype=dtype), **kw)
    poison_(view)
    return view, check


@contextlib.contextmanager
def poisoned_empty():
    """inside the block every torch.empty / torch.empty_like on the device returns poisoned memory: the outputs the wrappers of cruse_amd/ops.py
    allocate for the kernels then hold NaN (or 0xA5 bytes) where the kernel does not write.  The two functions are replaced for the WHOLE process
    until the block ends (keep it short, one thread); tensors that are not contiguous or whose dtype has no fill pattern (complex, bool) are
    returned as allocated, unpoisoned."""
    e, el = torch.empty, torch.empty_like

    def fill(r):
        return poison_(r) if (r.is_cuda and r.numel() and r.dtype in _BITS and r.is_contiguous()) else r
    torch.empty = lambda *a, **k: fill(e(*a, **k))
    torch.empty_like = lambda *a, **k: fill(el(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = e, el
