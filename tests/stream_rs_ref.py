"""Test-only: the float64 restatement of StreamingInferencer(io_rate=...), shared by tests/test_stream_rs_host.py (CPU) and
tests/test_gpu_stream_rs.py.  Pure torch float64, written from the formulas alone (its own design, not the package's):

  q = 2 (8 kHz, 32 kHz) or 3 (48 kHz), N = 32 q + 1, n = k - (N - 1) / 2, fc = 0.9 * 0.5 / q,
  h[k] = 2 fc sinc(2 fc n) kaiser(N, beta = 9)[k], divided by sum(h)
  decimate by q, phase 0:  D_q(u)[n] = sum_k h[k] u[q n - k]
  interpolate by q:        I_q(x)[m] = q sum_i h[m - q i] x[i],  0 <= m - q i <= N - 1
  both causal, zero before the clip.  32 / 48 kHz: In = D_q, Out = I_q.  8 kHz: In = I_2, Out = D_2.
  R(u) = Out(E(In(u))), E the float64 per-frame restatement of tests/stream_ref.py (stream_clip).

Every sum runs tap by tap over whole vectors (no convolution routine), so a clip converted block by block with carried history
gives the bits of the whole-clip form.
"""
from __future__ import annotations

import torch

from tests.stream_ref import stream_clip

F64 = torch.float64
RATES = (8000, 32000, 48000)


def ratio(io_rate: int) -> int:
    return {8000: 2, 32000: 2, 48000: 3}[io_rate]


def design(io_rate: int) -> torch.Tensor:
    """the N taps, float64"""
    q = ratio(io_rate)
    N = 32 * q + 1
    n = torch.arange(N, dtype=F64) - (N - 1) / 2
    fc = 0.9 * 0.5 / q
    h = 2 * fc * torch.sinc(2 * fc * n) * torch.kaiser_window(N, periodic=False, beta=9.0, dtype=F64)
    return h / h.sum()


def io_delay(io_rate: int) -> int:
    N = 32 * ratio(io_rate) + 1
    return (N - 1) // 2 if io_rate == 8000 else N - 1


def fir(z: torch.Tensor, h: torch.Tensor, hist=None):
    """y[m] = sum_k h[k] z[m - k] over the 1-D z, samples before it from hist (the N - 1 before z[0]; None: zeros).
    -> (y, the N - 1 last samples of [hist | z])"""
    N = h.numel()
    zp = torch.cat([torch.zeros(N - 1, dtype=F64) if hist is None else hist, z.to(F64)])
    y = torch.zeros(z.numel(), dtype=F64)
    for k in range(N):
        y += h[k] * zp[N - 1 - k:N - 1 - k + z.numel()]
    return y, zp[zp.numel() - (N - 1):].clone()


def decimate(u: torch.Tensor, h: torch.Tensor, q: int, hist=None):
    """D_q; u.numel() a multiple of q.  hist: at u's rate"""
    y, hist = fir(u, h, hist)
    return y[::q].clone(), hist


def interpolate(x: torch.Tensor, h: torch.Tensor, q: int, hist=None):
    """I_q.  hist: N - 1 samples of the zero-stuffed sequence (at the output's rate)"""
    z = torch.zeros(q * x.numel(), dtype=F64)
    z[::q] = x.to(F64)
    y, hist = fir(z, h, hist)
    return q * y, hist


def resample_in(u: torch.Tensor, io_rate: int, hist=None, with_hist: bool = False):
    """In(u): io_rate -> 16 kHz"""
    h, q = design(io_rate), ratio(io_rate)
    y, hist = interpolate(u, h, q, hist) if io_rate == 8000 else decimate(u, h, q, hist)
    return (y, hist) if with_hist else y


def resample_out(y16: torch.Tensor, io_rate: int, hist=None, with_hist: bool = False):
    """Out(y16): 16 kHz -> io_rate"""
    h, q = design(io_rate), ratio(io_rate)
    y, hist = decimate(y16, h, q, hist) if io_rate == 8000 else interpolate(y16, h, q, hist)
    return (y, hist) if with_hist else y


def R(model64, u: torch.Tensor, io_rate: int) -> torch.Tensor:
    """Out(E(In(u))) of the 1-D clip u at io_rate (a multiple of io_rate / 100 samples), float64; model64: stream_ref.as_double(module)"""
    return resample_out(stream_clip(model64, resample_in(u, io_rate), dtype=F64)[0], io_rate)


def response_db(h: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """20 log10 |H| at the frequencies f in cycles per sample of the filter's (higher) rate"""
    k = torch.arange(h.numel(), dtype=F64)
    ph = -2 * torch.pi * f.to(F64)[:, None] * k[None, :]
    re, im = (h * torch.cos(ph)).sum(1), (h * torch.sin(ph)).sum(1)
    return 10 * torch.log10(re ** 2 + im ** 2)
