"""The low-pass of cruse_resample_poly (csrc/resample.hip): the Kaiser-windowed sinc of inferencer/resample.py for
any reduced ratio, and the phase-major table the kernel reads.  Pure numpy: no torch, no device.

(up, down) = (dst_rate, src_rate) / gcd, q = max(up, down), N = 32 q + 1 taps,
    n = k - 16 q,  fc = 0.9 * 0.5 / q,  h[k] = 2 fc sinc(2 fc n) kaiser(N, beta = 9)[k],  h /= sum(h)
in float64 (np.sinc / np.kaiser conventions), rounded once to f32 for the device.  With v[up i] = x[i], zero elsewhere and outside
the clip,
    y[n] = up * sum_k h[k] v[n down + 16 q - k],   0 <= n < ceil(L up / down)
which is scipy.signal.resample_poly(x, up, down, window=h): zero-phase, zero-padded edges.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

BETA = 9.0
MAX_RATIO = 1024


def ratio(dst_rate: int, src_rate: int) -> Tuple[int, int]:
    """(up, down): the two rates over their gcd"""
    dst_rate, src_rate = int(dst_rate), int(src_rate)
    if dst_rate < 1 or src_rate < 1:
        raise ValueError(f"rates must be positive, got {src_rate} -> {dst_rate}")
    g = math.gcd(dst_rate, src_rate)
    return dst_rate // g, src_rate // g


def out_len(L: int, up: int, down: int) -> int:
    """ceil(L up / down): the samples a clip of L gives"""
    return -((-int(L) * int(up)) // int(down))


def design(up: int, down: int) -> np.ndarray:
    """the N = 32 max(up, down) + 1 taps in float64"""
    if not (1 <= up <= MAX_RATIO and 1 <= down <= MAX_RATIO) or math.gcd(up, down) != 1:
        raise ValueError(f"up = {up}, down = {down} must be reduced and lie in 1..{MAX_RATIO}")
    q = max(up, down)
    N = 32 * q + 1
    n = np.arange(N, dtype=np.float64) - 16 * q
    fc = 0.9 * 0.5 / q
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(N, BETA)
    return h / h.sum()


def taps_per_phase(up: int, down: int) -> int:
    """T = ceil(N / up): the taps that meet a sample, per output"""
    return -(-(32 * max(up, down) + 1) // up)


def phase_table(h: np.ndarray, up: int) -> np.ndarray:
    """[up, stride] with table[p, j] = h[p + up j], zeros beyond N; stride = T rounded up to a multiple of 4.  The dtype of h is kept."""
    N = h.shape[0]
    T = -(-N // up)
    stride = (T + 3) // 4 * 4
    flat = np.zeros(up * stride, dtype=h.dtype)
    full = np.zeros(up * T, dtype=h.dtype)
    full[:N] = h
    flat.reshape(up, stride)[:, :T] = full.reshape(T, up).T
    return flat.reshape(up, stride)


def from_phase_table(table: np.ndarray, N: int) -> np.ndarray:
    """the inverse of phase_table: h[k] = table[k mod up, k // up]"""
    up = table.shape[0]
    T = -(-N // up)
    return np.ascontiguousarray(table[:, :T].T).reshape(-1)[:N]


def direct_sum(x: np.ndarray, up: int, down: int, h: np.ndarray) -> np.ndarray:
    """the definition above, evaluated tap by tap in the dtype of h and x (float64 for a reference)"""
    L, N, c = x.shape[0], h.shape[0], 16 * max(up, down)
    y = np.zeros(out_len(L, up, down), dtype=np.result_type(x.dtype, h.dtype))
    m = np.arange(y.shape[0], dtype=np.int64) * down + c
    i0, p = m // up, m % up
    for j in range(-(-N // up)):
        k, i = p + up * j, i0 - j
        ok = (k < N) & (i >= 0) & (i < L)
        y[ok] += h[k[ok]] * x[i[ok]]
    return up * y
