"""The classic (non-extended) STOI as DESIGN section 13 defines it, restated in numpy stage by stage: the reference of
tests/test_metrics_host.py and tests/test_gpu_metrics.py.  float64 by default; dtype=np.float32 evaluates the same stages with
every table, every intermediate array and every product in f32 (the DFT as a matrix product, not numpy's float64 FFT), which is what
shows how far an f32 evaluation may sit from the float64 one.  pystoi is not available here: agreement with it is not claimed."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

FS = 10000
TAPS, UP, DOWN = 257, 5, 8
FRAME, HOP, NFFT = 256, 128, 512
NBANDS, SEG = 15, 30
DYN_RANGE = 40.0
BETA_DB = 15.0
EPS = float(np.finfo(np.float64).eps)          # 2^-52
SHORT_SCORE = 1e-5


def design() -> np.ndarray:
    """the 257 prototype taps on the 80 kHz grid, float64 (the convention of cruse_amd/inferencer/resample.py)"""
    n = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    fc = 0.9 * 0.5 / DOWN
    h = 2.0 * fc * np.sinc(2.0 * fc * n) * np.kaiser(TAPS, 9.0)
    return h / h.sum()


def window() -> np.ndarray:
    return np.hanning(FRAME + 2)[1:-1]


def band_edges() -> Tuple[np.ndarray, np.ndarray]:
    """(lo[15], hi[15]): band k covers the bins [lo[k], hi[k]) of the 512-point spectrum at 10 kHz"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NBANDS, dtype=np.float64)
    lo = np.array([int(np.argmin(np.abs(f - 150.0 * 2.0 ** ((2 * q - 1) / 6.0)))) for q in k])
    hi = np.array([int(np.argmin(np.abs(f - 150.0 * 2.0 ** ((2 * q + 1) / 6.0)))) for q in k])
    return lo, hi


def sizes(L: int) -> Tuple[int, int]:
    """(L10, nF) of a clip of L samples at 16 kHz"""
    L10 = (5 * L + 7) // 8
    return L10, ((L10 - FRAME) // HOP + 1 if L10 >= FRAME else 0)


def resample(u: np.ndarray, dtype=np.float64) -> np.ndarray:
    """x10[n] = 5 sum_k h[k] v[8 n + 128 - k], v[5 i] = u[i], zero outside the clip"""
    L = u.shape[0]
    L10, _ = sizes(L)
    v = np.zeros(UP * L, dtype=dtype)
    v[::UP] = u.astype(dtype)
    c = np.convolve(v, design().astype(dtype))                       # c[m] = sum_k h[k] v[m - k], length 5 L + 256
    return (dtype(UP) * c[DOWN * np.arange(L10) + (TAPS - 1) // 2]).astype(dtype)


def _frames(x: np.ndarray, n: int) -> np.ndarray:
    idx = HOP * np.arange(n)[:, None] + np.arange(FRAME)[None, :]
    return x[idx]


def _dft_power(fr: np.ndarray, dtype) -> np.ndarray:
    """|X|^2 of bins 0..256 of the 512-point DFT of 256-sample frames [n, 256]"""
    if dtype == np.float64:
        X = np.fft.rfft(fr, n=NFFT, axis=1)
        return X.real ** 2 + X.imag ** 2
    j = (np.arange(FRAME)[:, None] * np.arange(NFFT // 2 + 1)[None, :]) % NFFT
    c = np.cos(2.0 * np.pi * j / NFFT).astype(dtype)
    s = np.sin(2.0 * np.pi * j / NFFT).astype(dtype)
    re, im = fr @ c, fr @ s
    return re * re + im * im


def stoi_stages(ref: np.ndarray, est: np.ndarray, dtype=np.float64) -> Dict[str, object]:
    """One clip.  -> {"x10": [2, L10], "e": [nF], "kept": int[n_kept], "tob": [2, 15, nG], "score": float}"""
    assert ref.ndim == 1 and ref.shape == est.shape
    eps = dtype(EPS)
    L10, nF = sizes(ref.shape[0])
    x10 = np.stack([resample(ref, dtype), resample(est, dtype)])
    out = {"x10": x10, "e": np.zeros(0, dtype), "kept": np.zeros(0, np.int64), "tob": np.zeros((2, NBANDS, 0), dtype),
           "score": SHORT_SCORE}
    if nF < 1:
        return out
    w = window().astype(dtype)
    fr = w[None, None, :] * np.stack([_frames(x10[0], nF), _frames(x10[1], nF)])          # [2, nF, 256]
    e = (dtype(20.0) * np.log10(np.sqrt((fr[0] * fr[0]).sum(axis=1)) + eps)).astype(dtype)
    kept = np.nonzero(e > e.max() - dtype(DYN_RANGE))[0]
    out["e"], out["kept"] = e, kept
    nk = kept.shape[0]
    y = np.zeros((2, (nk - 1) * HOP + FRAME), dtype)
    for c, i in enumerate(kept):                                     # overlap-add back to back
        y[:, c * HOP:c * HOP + FRAME] += fr[:, i]
    nG = nk - 1
    if nG < 1:
        return out
    lo, hi = band_edges()
    tob = np.zeros((2, NBANDS, nG), dtype)
    for r in range(2):
        p = _dft_power((w[None, :] * _frames(y[r], nG)).astype(dtype), dtype)              # [nG, 257]
        for k in range(NBANDS):
            tob[r, k] = np.sqrt(p[:, lo[k]:hi[k]].sum(axis=1))
    out["tob"] = tob
    if nG < SEG:
        return out
    X = np.lib.stride_tricks.sliding_window_view(tob[0], SEG, axis=1)                      # [15, nG - 29, 30]
    Y = np.lib.stride_tricks.sliding_window_view(tob[1], SEG, axis=1)
    nrm = lambda a: np.sqrt((a * a).sum(axis=2, keepdims=True))     # noqa: E731
    alpha = nrm(X) / (nrm(Y) + eps)
    Yp = np.minimum(alpha * Y, X * dtype(1.0 + 10.0 ** (BETA_DB / 20.0)))
    Xc = X - X.mean(axis=2, keepdims=True, dtype=dtype)
    Yc = Yp - Yp.mean(axis=2, keepdims=True, dtype=dtype)
    Xh = Xc / (nrm(Xc) + eps)
    Yh = Yc / (nrm(Yc) + eps)
    out["score"] = float((Xh * Yh).sum(dtype=dtype) / dtype(NBANDS * (nG - SEG + 1)))
    return out


def stoi(ref: np.ndarray, est: np.ndarray, dtype=np.float64) -> float:
    return stoi_stages(ref, est, dtype)["score"]


def threshold_margin(e: np.ndarray) -> float:
    """the least distance in dB of a frame energy from the 40 dB threshold (inf where there are no frames)"""
    return float(np.abs(e - (e.max() - DYN_RANGE)).min()) if e.shape[0] else float("inf")


def si_sdr(ref: np.ndarray, est: np.ndarray) -> float:
    ref, est = ref.astype(np.float64), est.astype(np.float64)
    p = (ref @ est) / (ref @ ref) * ref
    return float(10.0 * np.log10((p * p).sum() / ((est - p) ** 2).sum()))


def speechlike(L: int, seed: int, gap: Tuple[int, int] = None) -> np.ndarray:
    """A seeded "speech-like" clip (f32): a harmonic stack on a gliding pitch under a 3 Hz syllable envelope, zeroed over
    samples [gap[0], gap[1])."""
    rng = np.random.default_rng(seed)
    t = np.arange(L, dtype=np.float64) / 16000.0
    f0 = rng.uniform(100.0, 180.0) * (1.0 + 0.1 * np.sin(2.0 * np.pi * rng.uniform(0.5, 1.5) * t + rng.uniform(0, 6.28)))
    ph = 2.0 * np.pi * np.cumsum(f0) / 16000.0
    x = np.zeros(L)
    for h in range(1, 31):
        x += rng.uniform(0.3, 1.0) / h ** 0.8 * np.sin(h * ph + rng.uniform(0, 6.28))
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + rng.uniform(0, 6.28))        # never silent: only the gap removes frames
    x = 0.1 * x * env
    if gap is not None:
        x[gap[0]:gap[1]] = 0.0
    return x.astype(np.float32)


def add_noise(x: np.ndarray, snr_db: float, seed: int) -> np.ndarray:
    """x + white noise at snr_db relative to the power of x over the whole clip (f32)"""
    n = np.random.default_rng(seed).standard_normal(x.shape[0])
    g = np.sqrt((x.astype(np.float64) ** 2).mean() / (n ** 2).mean() / 10.0 ** (snr_db / 10.0))
    return (x + g * n).astype(np.float32)
