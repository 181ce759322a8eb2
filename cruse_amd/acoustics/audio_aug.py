"""EQ augmentation of train_base/acoustics/audioAug.py on the device: the six RBJ biquad designers (:13-129), their registries
(:132-147), compositeSecFilt (:149-165) and hp_filter (:168-178).  The filtering -- torchaudio.functional.lfilter there -- is
cruse_biquad_cascade (csrc/biquad.hip): float64 coefficients and recurrence, f32 samples, one launch per batch.

Repairs to the reference, each needed before its code can run at all:
  * `import torchaudio` (:3) is not installed and not a dependency; ops.biquad_cascade replaces torchaudio.functional.lfilter
    (:164, :177) with lfilter's default clamp=True;
  * high_shelf (:27-30) and low_shelf (:67-70) concatenate b and a into a flat [6], while both call sites index the result as
    [1, :] / [0, :] (:164, :177): EVERY designer here returns [2, 3], rows (b; a), float64;
  * notch builds b0 as `Tensor(1.)` (:117), which does not construct: b0 = b2 = 1;
  * high_pass annotates `sr: Tensor` (:33); it takes a float like the other five;
  * no designer checks its centre frequency: at sr / 2 low_pass has a double pole ON the unit circle and above it every design
    aliases.  center_freq >= sr / 2 (or <= 0) raises ValueError.
airAbsorption / interp_atten / as_windowed (:180-226) are not carried over: the function reads `att_interp_db` before assigning it
(:189) and inverts a hop-160 STFT with hop 320 (:191-195), so it never ran.

The formulas are those of the RBJ Audio-EQ-Cookbook, as the reference states them (w0 = 2 pi f / sr, alpha = sin(w0) / (2 Q),
A = 10^(gain_db / 40)), evaluated in float64 on the host."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

IDENTITY_SECTION = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _scalar(v) -> float:
    """the reference passes python floats, 1-element numpy arrays (np.random.uniform(.., 1)) and tensors alike"""
    if isinstance(v, torch.Tensor):
        return float(v.reshape(-1)[0])
    return float(np.asarray(v, dtype=np.float64).reshape(-1)[0])


def design_sections(kind: str, center_freq, gain_db, q_factor, sr) -> np.ndarray:
    """the one implementation of the six designs, over numpy arrays of any (common) shape -> [..., 6] float64, (b0 b1 b2 a0 a1 a2)"""
    f, g, q = (np.asarray(v, dtype=np.float64) for v in (center_freq, gain_db, q_factor))
    sr = float(sr)
    if not (np.all(f > 0.0) and np.all(f < 0.5 * sr)):
        raise ValueError(f"{kind}: center_freq = {f} Hz must lie inside (0, sr / 2 = {0.5 * sr})")
    if not np.all(q > 0.0):
        raise ValueError(f"{kind}: q_factor = {q} must be positive")
    w0 = 2.0 * np.pi * f / sr
    cw, alpha, amp = np.cos(w0), np.sin(w0) / (2.0 * q), np.power(10.0, g / 40.0)
    one = np.ones_like(cw * alpha * amp)
    if kind in ("high_shelf", "low_shelf"):
        r = 2.0 * np.sqrt(amp) * alpha
        sg = 1.0 if kind == "high_shelf" else -1.0                   # the two shelves mirror each other in cos(w0)
        c = sg * cw
        b = (amp * ((amp + 1) + (amp - 1) * c + r), -2 * sg * amp * ((amp - 1) + (amp + 1) * c), amp * ((amp + 1) + (amp - 1) * c - r))
        a = ((amp + 1) - (amp - 1) * c + r, 2 * sg * ((amp - 1) - (amp + 1) * c), (amp + 1) - (amp - 1) * c - r)
    elif kind == "peaking_eq":
        b = (1 + alpha * amp, -2 * cw, 1 - alpha * amp)
        a = (1 + alpha / amp, -2 * cw, 1 - alpha / amp)
    else:
        a = (1 + alpha, -2 * cw, 1 - alpha)
        if kind == "high_pass":
            b = ((1 + cw) / 2, -(1 + cw), (1 + cw) / 2)
        elif kind == "low_pass":
            b = ((1 - cw) / 2, 1 - cw, (1 - cw) / 2)
        elif kind == "notch":
            b = (one, -2 * cw, one)
        else:
            raise KeyError(kind)
    return np.stack([v * one for v in b + a], axis=-1)


def _designer(kind: str):
    def design(center_freq, gain_db, q_factor, sr: float) -> torch.Tensor:
        c = design_sections(kind, _scalar(center_freq), _scalar(gain_db), _scalar(q_factor), _scalar(sr))
        return torch.from_numpy(c.reshape(2, 3).copy())
    design.__name__ = design.__qualname__ = kind
    design.__doc__ = f"RBJ {kind.replace('_', ' ')} -> [2, 3] float64, rows (b; a)"
    return design


high_shelf, high_pass, low_shelf = _designer("high_shelf"), _designer("high_pass"), _designer("low_shelf")
low_pass, peaking_eq, notch = _designer("low_pass"), _designer("peaking_eq"), _designer("notch")


REGISTERED_SecFilter = {
    "high_shelf": high_shelf,
    "high_pass": high_pass,
    "low_shelf": low_shelf,
    "low_pass": low_pass,
    "peaking_eq": peaking_eq,
    "notch": notch,
}
REGISTERED_SecFilter_freq = {
    "high_shelf": [1000, 4000],
    "high_pass": [40, 400],
    "low_shelf": [40, 1000],
    "low_pass": [3000, 8000],
    "peaking_eq": [40, 4000],
    "notch": [40, 4000],
}
FILTER_LIST = ("high_shelf", "high_pass", "low_shelf", "low_pass", "peaking_eq", "notch")        # the order of :150-153
GAIN_DB_RANGE = (-15.0, 15.0)                                                                  # :161
Q_RANGE = (0.5, 1.5)                                                                           # :162, :173
HP_FREQ = 150.0                                                                                # :172


def _rng(rng) -> np.random.Generator:
    return np.random.default_rng() if rng is None else rng


def draw_sec_filter_params(n: int, filter_num: int = 3, sr: float = 16000, rng: Optional[np.random.Generator] = None):
    """the draws behind draw_sec_filters: (types [n, filter_num] indices into FILTER_LIST, freq, gain_db, q, each [n, filter_num])"""
    if not 0 < filter_num < len(FILTER_LIST):
        raise ValueError(f"filter_num = {filter_num} must lie in 1..{len(FILTER_LIST) - 1}")                # the assert of :154
    rng = _rng(rng)
    types = np.argsort(rng.random((n, len(FILTER_LIST))), axis=1)[:, :filter_num]                          # distinct per clip
    rng_log = np.log(np.array([REGISTERED_SecFilter_freq[k] for k in FILTER_LIST], dtype=np.float64))
    freq = np.exp(rng.uniform(rng_log[types, 0], rng_log[types, 1]))
    freq = np.minimum(freq, np.nextafter(0.5 * float(sr), 0.0))      # low_pass' range ends AT sr / 2 for sr = 16000
    gain = rng.uniform(*GAIN_DB_RANGE, size=(n, filter_num))
    q = rng.uniform(*Q_RANGE, size=(n, filter_num))
    return types, freq, gain, q


def draw_sec_filters(n: int, filter_num: int = 3, sr: float = 16000, rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """n independent draws of compositeSecFilt's cascade (:155-163) -> [n, filter_num, 6] float64, rows (b0 b1 b2 a0 a1 a2): per clip
    filter_num DISTINCT types, a centre frequency log-uniform over the type's range, gain U(-15, 15) dB, Q U(0.5, 1.5).
    The draws come from `rng` (a np.random.Generator; a fresh default_rng() when None).  They do NOT replay the reference's
    streams -- python's global `random`, scipy.stats.loguniform and np.random's global state -- only their distributions."""
    types, freq, gain, q = draw_sec_filter_params(n, filter_num, sr, rng)
    out = np.empty((n, filter_num, 6), dtype=np.float64)
    for t, kind in enumerate(FILTER_LIST):
        m = types == t
        if m.any():
            out[m] = design_sections(kind, freq[m], gain[m], q[m], sr)
    return out


def draw_hp_filters(n: int, filte_num: int = 1, sr: float = 16000, rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """n draws of hp_filter's section (:172-174): a 150 Hz high-pass with Q U(0.5, 1.5), the SAME section repeated filte_num times
    (:176-177) -> [n, filte_num, 6] float64.  `rng` as in draw_sec_filters."""
    if filte_num < 1:
        raise ValueError(f"filte_num = {filte_num} must be at least 1")
    q = _rng(rng).uniform(*Q_RANGE, size=n)
    sec = design_sections("high_pass", np.full(n, HP_FREQ), np.zeros(n), q, sr)
    return np.ascontiguousarray(np.broadcast_to(sec[:, None, :], (n, filte_num, 6)))


def _filter(indata: torch.Tensor, coef: np.ndarray) -> torch.Tensor:
    from .. import ops
    x = indata.reshape(1, -1) if indata.dim() == 1 else indata
    y = ops.biquad_cascade(x.contiguous().float(), torch.from_numpy(coef).to(x.device), clamp=True)
    return y.reshape(indata.shape)


def _clips(indata: torch.Tensor, name: str) -> int:
    if not isinstance(indata, torch.Tensor) or indata.dim() not in (1, 2) or not indata.is_cuda:
        raise RuntimeError(f"{name}: indata must be an [L] or [B, L] tensor on the HIP device (there is no CPU path)")
    return 1 if indata.dim() == 1 else indata.shape[0]


def compositeSecFilt(indata: torch.Tensor, filter_num: int = 3, sr: float = 16000, rng: Optional[np.random.Generator] = None) -> torch.Tensor:
    """:149-165 for [L] or a batch [B, L] on the device: one independent draw_sec_filters draw per clip, one launch; same shape out."""
    return _filter(indata, draw_sec_filters(_clips(indata, "compositeSecFilt"), filter_num, sr, rng))


def hp_filter(indata: torch.Tensor, filte_num: int = 1, sr: float = 16000, rng: Optional[np.random.Generator] = None) -> torch.Tensor:
    """fixed frequency high pass filter (:168-178) for [L] or [B, L] on the device: one Q per clip; same shape out."""
    return _filter(indata, draw_hp_filters(_clips(indata, "hp_filter"), filte_num, sr, rng))
