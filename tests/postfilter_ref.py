"""Test-only: float64 references of the perceptual post-filter, shared by tests/test_postfilter_host.py (CPU) and
tests/test_gpu_postfilter.py.

pf(g, tau, kind): the two closed forms of DESIGN 12e in numpy float64, g the mask value in [0, 1], s = sin(pi g / 2):
    "iam"        g (1 + tau) s^2 / (s^2 + tau)
    "envelope"   g s sqrt((1 + tau) s / (s^2 + tau)),   0 at g = 0
tau == 0 returns g itself.  tests/test_postfilter_host.py pins them on the outputs of the reference's own two functions
(tests/golden/postfilter.npz).

e64_pf(frames, tau, kind): the float64 per-frame chain of tests/stream_ref.py with pf applied to every frame's mask row: the frames'
own spectra and masks (stream_clip's intermediates), the masked spectrum, inverse DFT, window and overlap-add redone.
mix(noisy, e64_of_filtered_mask, lim): R(x, lim) = lim x + (1 - lim) E64_pf(x), tests/stream_io_ref.mix on the filtered chain.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import stream_io_ref as IO
from tests.stream_ref import HOP, NFFT, as_double, stream_clip

KINDS = ("iam", "envelope")


def pf(g, tau: float, kind: str) -> np.ndarray:
    g = np.asarray(g, dtype=np.float64)
    if kind not in KINDS:
        raise ValueError(kind)
    if tau == 0.0:
        return g.copy()
    s = np.sin(0.5 * np.pi * g)
    den = s * s + tau
    if kind == "iam":
        return g * ((1.0 + tau) * s * s / den)
    return g * s * np.sqrt((1.0 + tau) * s / den)


def sweep(n: int = 4097) -> np.ndarray:
    """n gains, sorted: the uniform grid k / (n - 5), k = 0 .. n - 5 (n - 5 even: 0, 0.5 and 1 are on it), and 1e-30, 2^-24, 1e-4, 1 - 2^-24"""
    assert n >= 7 and (n - 5) % 2 == 0
    g = np.unique(np.concatenate([np.arange(n - 4, dtype=np.float64) / (n - 5), [1e-30, 2.0 ** -24, 1e-4, 1.0 - 2.0 ** -24]]))
    assert g.size == n and g[0] == 0.0 and g[-1] == 1.0 and 0.5 in g
    return g


def frames64(o, x: torch.Tensor):
    """the float64 restatement's per-frame intermediates for the 1-D clip x (re, im, mask, ...), computed once per clip"""
    return stream_clip(as_double(o), x, dtype=torch.float64)[1]


def e64_pf(frames, tau, kind: str) -> torch.Tensor:
    """the enhanced clip [L] in float64 with pf(mask, tau(t), kind) in place of the mask; tau: a float, or a callable frame index -> tau"""
    win = torch.hann_window(NFFT, dtype=torch.float64)
    env = win[:HOP] ** 2 + win[HOP:] ** 2
    tail = torch.zeros(HOP, dtype=torch.float64)
    zero = torch.zeros(1, dtype=torch.float64)
    blocks = []
    for t, fr in enumerate(frames):
        tt = tau(t) if callable(tau) else tau
        m = torch.from_numpy(pf(fr["mask"].numpy(), float(tt), kind))
        er, ei = torch.cat([m * fr["re"][:160], zero]), torch.cat([m * fr["im"][:160], zero])
        y = torch.fft.irfft(torch.complex(er, ei), n=NFFT) * win
        if t >= 1:
            blocks.append((tail + y[:HOP]) / env)
        tail = y[HOP:].clone()
    return torch.cat(blocks)


def mix(noisy: torch.Tensor, e64_of_filtered_mask: torch.Tensor, lim: float) -> torch.Tensor:
    """lim * noisy + (1 - lim) * E64_pf(noisy), float64"""
    return IO.mix(noisy, e64_of_filtered_mask, lim)
