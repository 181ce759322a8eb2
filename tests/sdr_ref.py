"""bss_eval SDR of one source as DESIGN section 13g defines it, restated in float64 numpy stage by stage: the reference of
tests/test_sdr_host.py and tests/test_gpu_sdr.py.  Correlations by direct sums, the system by np.linalg.solve (LU) on the dense
Toeplitz matrix, the projection by np.convolve.  solver="levinson" solves with scipy.linalg.solve_toeplitz instead: the distance
between the two is the restatement's own spread, from which the GPU test takes its bars.  mir_eval is not available here: agreement
with it is not claimed."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from tests import stoi_ref as R

FILTER_LEN = 512
NAN = float("nan")


def speechlike(L: int, seed: int, floor_db: float = -30.0) -> np.ndarray:
    """stoi_ref.speechlike (harmonics on a gliding pitch under a slow envelope) plus a white noise floor floor_db under it (f32).  The
    floor bounds cond(toeplitz(raa)): about 1e3 at -30 dB."""
    x = R.speechlike(L, seed).astype(np.float64)
    w = np.random.default_rng(seed + 7919).standard_normal(L)
    p = (x ** 2).mean() if L else 1.0
    return (x + np.sqrt(p * 10.0 ** (floor_db / 10.0)) * w).astype(np.float32)


def distort(ref: np.ndarray, seed: int) -> np.ndarray:
    """est = a short FIR of ref + an independent stack at -20 dB + 0.05 tanh(3 ref) (f32)"""
    L = ref.shape[0]
    x = ref.astype(np.float64)
    y = np.convolve(x, np.array([0.8, 0.3, -0.15, 0.05]))[:L]
    o = speechlike(L, seed).astype(np.float64)
    g = np.sqrt((x ** 2).sum() / max((o ** 2).sum(), 1e-300) * 10.0 ** (-20.0 / 10.0))
    return (y + g * o + 0.05 * np.tanh(3.0 * x)).astype(np.float32)


def toeplitz(r: np.ndarray) -> np.ndarray:
    k = np.arange(r.shape[0])
    return r[np.abs(k[:, None] - k[None, :])]


def correlations(ref: np.ndarray, est: np.ndarray, K: int):
    """raa[k] = sum_i ref[i] ref[i+k], rab[k] = sum_i ref[i] est[i+k], samples outside the clip zero"""
    n = ref.shape[0]
    raa, rab = np.zeros(K), np.zeros(K)
    for k in range(min(K, n)):
        raa[k] = ref[:n - k] @ ref[k:]
        rab[k] = ref[:n - k] @ est[k:]
    return raa, rab


def solve(raa: np.ndarray, rab: np.ndarray, solver: str = "lu") -> np.ndarray:
    if solver == "lu":
        return np.linalg.solve(toeplitz(raa), rab)
    if solver == "levinson":
        from scipy.linalg import solve_toeplitz
        return solve_toeplitz(raa, rab)
    if solver == "cholesky":
        from scipy.linalg import cho_factor, cho_solve
        return cho_solve(cho_factor(toeplitz(raa)), rab)
    raise ValueError(solver)


def sdr_stages(ref: np.ndarray, est: np.ndarray, K: int = FILTER_LEN, length: Optional[int] = None, solver: str = "lu") -> Dict[str, object]:
    """One clip (its first `length` samples when given; nothing beyond is touched).
    -> {"raa": [K], "rab": [K], "C": [K], "s_target": [n + K - 1], "ss": sum s_target^2, "ee": sum e^2, "score": dB}; a degenerate clip
    (n = 0, all-zero ref) has NaN for C, the energies and the score"""
    assert ref.ndim == 1 and ref.shape == est.shape and K >= 1
    n = ref.shape[0] if length is None else int(length)
    x, y = ref[:n].astype(np.float64), est[:n].astype(np.float64)
    raa, rab = correlations(x, y, K)
    out = {"raa": raa, "rab": rab, "C": np.full(K, NAN), "s_target": np.zeros(0), "ss": NAN, "ee": NAN, "score": NAN}
    if n == 0 or raa[0] <= 0.0:
        return out
    C = solve(raa, rab, solver)
    s = np.convolve(C, x)                                            # n + K - 1
    e = np.concatenate([y, np.zeros(K - 1)]) - s
    ss, ee = float(s @ s), float(e @ e)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = float(10.0 * np.log10(np.float64(ss) / np.float64(ee)))
    out.update(C=C, s_target=s, ss=ss, ee=ee, score=score)
    return out


def sdr(ref: np.ndarray, est: np.ndarray, K: int = FILTER_LEN, solver: str = "lu") -> float:
    return sdr_stages(ref, est, K, solver=solver)["score"]


def rel(a, b) -> float:
    """|a - b| relative to |b| (rel-L2 for arrays)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))
