"""Float64 reference of the biquad cascade and of the six RBJ designs (a helper, not a test).  Nothing here imports the module under
test: the designs are restated from the RBJ Audio-EQ-Cookbook one by one with python's math, the filtering is scipy.signal.lfilter."""
from __future__ import annotations

import math

import numpy as np

SR = 16000.0
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
KINDS = ("high_shelf", "high_pass", "low_shelf", "low_pass", "peaking_eq", "notch")
FREQ_RANGE = {"high_shelf": (1000, 4000), "high_pass": (40, 400), "low_shelf": (40, 1000), "low_pass": (3000, 8000),
              "peaking_eq": (40, 4000), "notch": (40, 4000)}


def design(kind: str, f: float, gain_db: float, q: float, sr: float = SR) -> np.ndarray:
    """(b0 b1 b2 a0 a1 a2), float64"""
    w0 = 2.0 * math.pi * f / sr
    cs, sn = math.cos(w0), math.sin(w0)
    al = sn / (2.0 * q)
    A = 10.0 ** (gain_db / 40.0)
    sq = 2.0 * math.sqrt(A) * al
    if kind == "low_pass":
        c = [(1 - cs) / 2, 1 - cs, (1 - cs) / 2, 1 + al, -2 * cs, 1 - al]
    elif kind == "high_pass":
        c = [(1 + cs) / 2, -(1 + cs), (1 + cs) / 2, 1 + al, -2 * cs, 1 - al]
    elif kind == "notch":
        c = [1.0, -2 * cs, 1.0, 1 + al, -2 * cs, 1 - al]
    elif kind == "peaking_eq":
        c = [1 + al * A, -2 * cs, 1 - al * A, 1 + al / A, -2 * cs, 1 - al / A]
    elif kind == "low_shelf":
        c = [A * ((A + 1) - (A - 1) * cs + sq), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - sq),
             (A + 1) + (A - 1) * cs + sq, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - sq]
    elif kind == "high_shelf":
        c = [A * ((A + 1) + (A - 1) * cs + sq), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - sq),
             (A + 1) - (A - 1) * cs + sq, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - sq]
    else:
        raise KeyError(kind)
    return np.array(c, dtype=np.float64)


# name -> (kind, Hz, dB, Q): the designs closest to the unit circle and the extremes of every range the augmentation draws from
CORNERS = {
    "hp40_q1.5": ("high_pass", 40.0, 0.0, 1.5),
    "hp40_q0.5": ("high_pass", 40.0, 0.0, 0.5),
    "ls40_+15_q1.5": ("low_shelf", 40.0, 15.0, 1.5),
    "ls40_-15_q1.5": ("low_shelf", 40.0, -15.0, 1.5),
    "ls40_+15_q0.5": ("low_shelf", 40.0, 15.0, 0.5),
    "ls40_-15_q0.5": ("low_shelf", 40.0, -15.0, 0.5),
    "pk40_+15_q1.5": ("peaking_eq", 40.0, 15.0, 1.5),
    "pk40_-15_q1.5": ("peaking_eq", 40.0, -15.0, 1.5),
    "pk40_+15_q0.5": ("peaking_eq", 40.0, 15.0, 0.5),
    "pk40_-15_q0.5": ("peaking_eq", 40.0, -15.0, 0.5),
    "lp7900_q1.5": ("low_pass", 7900.0, 0.0, 1.5),
    "lp7900_q0.5": ("low_pass", 7900.0, 0.0, 0.5),
    "hs4000_+15_q1.5": ("high_shelf", 4000.0, 15.0, 1.5),
    "hs4000_-15_q0.5": ("high_shelf", 4000.0, -15.0, 0.5),
    "notch40_q1.5": ("notch", 40.0, 0.0, 1.5),
    "notch4000_q0.5": ("notch", 4000.0, 0.0, 0.5),
}


def corner(name: str) -> np.ndarray:
    return design(*CORNERS[name])


def corner_table() -> np.ndarray:
    """[len(CORNERS), 6]"""
    return np.stack([corner(k) for k in CORNERS])


def pole_radius(c) -> float:
    return float(np.abs(np.roots(np.asarray(c, dtype=np.float64)[3:6])).max()) if (c[4] != 0 or c[5] != 0) else 0.0


def response_db(c, f: float, sr: float = SR) -> float:
    z = np.exp(-1j * 2.0 * np.pi * f / sr)
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(divide="ignore"):                              # a notch's centre is an exact zero: -inf dB
        return float(20.0 * np.log10(np.abs((c[0] + c[1] * z + c[2] * z * z) / (c[3] + c[4] * z + c[5] * z * z))))


def cascade_ref(x, coef, clamp: bool) -> np.ndarray:
    """x [B, L] (or [L]); coef [S, 6] shared or [B, S, 6] -> float64, the definition: per section
    scipy.signal.lfilter(b / a0, a / a0, .) in float64 from rest, then (clamp) clipped to [-1, 1] before the next section"""
    from scipy.signal import lfilter
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    y = np.array(x.reshape(1, -1) if one else x, dtype=np.float64)
    coef = np.asarray(coef, dtype=np.float64)
    for b in range(y.shape[0]):
        for sec in (coef if coef.ndim == 2 else coef[b]):
            y[b] = lfilter(sec[0:3] / sec[3], sec[3:6] / sec[3], y[b])
            if clamp:
                np.clip(y[b], -1.0, 1.0, out=y[b])
    return y[0] if one else y


def seq_f32(x, coef) -> np.ndarray:
    """the same cascade (no clamp) as a SEQUENTIAL recurrence with f32 coefficients, states and arithmetic (transposed direct form II,
    the form lfilter runs) -> [L] float32: what an all-f32 kernel would compute at best"""
    f = np.float32
    y = np.asarray(x, dtype=np.float32).copy()
    for sec in np.asarray(coef, dtype=np.float64).reshape(-1, 6):
        b0, b1, b2, a1, a2 = (f(v) for v in (sec[0] / sec[3], sec[1] / sec[3], sec[2] / sec[3], sec[4] / sec[3], sec[5] / sec[3]))
        z0 = z1 = f(0.0)
        out = np.empty_like(y)
        for i, xi in enumerate(y):
            yo = f(b0 * xi + z0)
            z0 = f(f(b1 * xi + z1) - f(a1 * yo))
            z1 = f(f(b2 * xi) - f(a2 * yo))
            out[i] = yo
        y = out
    return y


def synth_like(B: int, L: int, seed: int, peak: float = 0.9) -> np.ndarray:
    """[B, L] float32 shaped like data.synth_batch's clean speech (a one-pole low-pass, a = 0.95, of white noise), each clip scaled
    so that its peak is `peak`"""
    from scipy.signal import lfilter
    w = np.random.default_rng(seed).standard_normal((B, L))
    s = lfilter([0.05], [1.0, -0.95], w, axis=1)
    s *= peak / np.maximum(np.abs(s).max(axis=1, keepdims=True), 1e-30)
    return s.astype(np.float32)


def bar(ref: np.ndarray) -> np.ndarray:
    """per clip: one f32 ulp at the clip's peak, 2^-23 max(peak |ref|, 1e-3)"""
    ref = np.atleast_2d(ref)
    return 2.0 ** -23 * np.maximum(np.abs(ref).max(axis=1), 1e-3)
