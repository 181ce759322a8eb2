"""The sample-rate converters of StreamingInferencer(io_rate=...): the filter design and the sizes the kernels
(cruse_stream_resample_*, csrc/stream_rs.hip) and the host agree on.  Pure numpy: no torch, no device.

The model runs at 16 kHz.  With q = 2 (8 kHz, 32 kHz) or 3 (48 kHz) and N = 32 q + 1 taps, the low-pass is a Kaiser-windowed sinc
    n = k - (N - 1) / 2,  fc = 0.9 * 0.5 / q,  h[k] = 2 fc sinc(2 fc n) kaiser(N, beta = 9)[k],  h /= sum(h)
built in float64 (np.sinc / np.kaiser conventions) and rounded once to f32 for the device.  Both operators are causal from a zero
history:
    decimate by q, phase 0:  D_q(u)[n] = sum_k h[k] u[q n - k]
    interpolate by q:        I_q(x)[m] = q sum_i h[m - q i] x[i],  0 <= m - q i <= N - 1
32 / 48 kHz: x16 = D_q(u) on the way in, v = I_q(y16) on the way out, together N - 1 samples of delay at io_rate.
8 kHz: x16 = I_2(u), v = D_2(y16), together (N - 1) / 2 samples at 8 kHz.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

MODEL_RATE = 16000
IO_RATES = (8000, 16000, 32000, 48000)
BETA = 9.0


def check_rate(io_rate) -> int:
    if io_rate not in IO_RATES:
        raise ValueError(f"io_rate must be one of 8000, 16000, 32000, 48000, got {io_rate!r}")
    return int(io_rate)


def ratio(io_rate: int) -> int:
    """q: samples at the higher rate per sample at the lower one (1 at 16 kHz)"""
    io_rate = check_rate(io_rate)
    return {8000: 2, 16000: 1, 32000: 2, 48000: 3}[io_rate]


def design(io_rate: int) -> Tuple[int, np.ndarray]:
    """(q, the N = 32 q + 1 taps in float64) of io_rate 8000, 32000 or 48000"""
    q = ratio(io_rate)
    if q == 1:
        raise ValueError("io_rate 16000 is the model's rate: there is no filter to design")
    N = 32 * q + 1
    n = np.arange(N, dtype=np.float64) - (N - 1) / 2
    fc = 0.9 * 0.5 / q
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(N, BETA)
    return q, h / h.sum()


def io_block(io_rate: int) -> int:
    """samples of a 10 ms block at io_rate"""
    return check_rate(io_rate) // 100


def io_delay(io_rate: int) -> int:
    """samples at io_rate by which the two converters together delay the signal (0 at 16 kHz)"""
    q = ratio(io_rate)
    if q == 1:
        return 0
    return 16 * q if io_rate < MODEL_RATE else 32 * q


def history(io_rate: int) -> Tuple[int, int]:
    """(in-side, out-side) history samples a slot carries in rs_state: the in-side ones at io_rate, the out-side ones at 16 kHz"""
    q = ratio(io_rate)
    if q == 1:
        return 0, 0
    N = 32 * q + 1
    return ((N - 1) // q, N - 1) if io_rate < MODEL_RATE else (N - 1, (N - 1) // q)
