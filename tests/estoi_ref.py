"""Extended STOI (Jensen & Taal 2016) as DESIGN section 13f defines it, restated in numpy on the stages of tests/stoi_ref.py: the
reference of tests/test_metrics_ext_host.py and tests/test_gpu_metrics_ragged.py.  Stages 1-3 (10 kHz signals, kept frames, band
magnitudes) are STOI's; stage 4 normalises the rows and then the columns of every 15 x 30 segment and correlates, with no clipping.
float64 by default, dtype=np.float32 as in stoi_ref.  `length` states the ragged rule on a padded clip: samples at and beyond it are
outside the clip (whatever they hold, NaN included) and the stage sizes are those of a clip of `length` samples.  pystoi is not
available here: agreement with it is not claimed."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from tests import stoi_ref as R


def _stages_of_padded(ref: np.ndarray, est: np.ndarray, length: int, dtype) -> Dict[str, object]:
    """stages 1-3 of the clip ref[:length] evaluated ON THE PADDED arrays: the padding is replaced by the zeros that lie outside any
    clip, the whole padded row is resampled, and only then are the clip's own L10 and nF applied"""
    L = ref.shape[0]
    assert 0 <= length <= L
    eps = dtype(R.EPS)
    inside = np.arange(L) < length
    L10, nF = R.sizes(length) if length > 0 else (0, 0)
    x10 = np.stack([R.resample(np.where(inside, u, 0.0).astype(np.float32), dtype)[:L10] for u in (ref, est)])
    out = {"x10": x10, "e": np.zeros(0, dtype), "kept": np.zeros(0, np.int64), "tob": np.zeros((2, R.NBANDS, 0), dtype)}
    if nF < 1:
        return out
    w = R.window().astype(dtype)
    fr = w[None, None, :] * np.stack([R._frames(x10[0], nF), R._frames(x10[1], nF)])
    e = (dtype(20.0) * np.log10(np.sqrt((fr[0] * fr[0]).sum(axis=1)) + eps)).astype(dtype)
    kept = np.nonzero(e > e.max() - dtype(R.DYN_RANGE))[0]
    out["e"], out["kept"] = e, kept
    nG = kept.shape[0] - 1
    if nG < 1:
        return out
    y = np.zeros((2, nG * R.HOP + R.FRAME), dtype)
    for c, i in enumerate(kept):
        y[:, c * R.HOP:c * R.HOP + R.FRAME] += fr[:, i]
    lo, hi = R.band_edges()
    tob = np.zeros((2, R.NBANDS, nG), dtype)
    for r in range(2):
        p = R._dft_power((w[None, :] * R._frames(y[r], nG)).astype(dtype), dtype)
        for k in range(R.NBANDS):
            tob[r, k] = np.sqrt(p[:, lo[k]:hi[k]].sum(axis=1))
    out["tob"] = tob
    return out


def _row_col_normalise(a: np.ndarray, eps) -> np.ndarray:
    """a [nSeg, 15, 30]: every row (a band over its 30 frames) less its mean over (its norm + eps), then every column (a frame over
    its 15 bands) the same"""
    dt = a.dtype
    a = a - a.mean(axis=2, keepdims=True, dtype=dt)
    a = a / (np.sqrt((a * a).sum(axis=2, keepdims=True, dtype=dt)) + eps)
    a = a - a.mean(axis=1, keepdims=True, dtype=dt)
    return a / (np.sqrt((a * a).sum(axis=1, keepdims=True, dtype=dt)) + eps)


def estoi_stages(ref: np.ndarray, est: np.ndarray, dtype=np.float64, length: Optional[int] = None) -> Dict[str, object]:
    """One clip -> the stages of stoi_ref.stoi_stages with "score" the ESTOI score"""
    assert ref.ndim == 1 and ref.shape == est.shape
    st = dict(R.stoi_stages(ref, est, dtype)) if length is None else _stages_of_padded(ref, est, int(length), dtype)
    st["score"] = R.SHORT_SCORE
    tob = st["tob"]
    nG = tob.shape[2]
    if nG < R.SEG:
        return st
    eps = dtype(R.EPS)
    X = np.lib.stride_tricks.sliding_window_view(tob[0], R.SEG, axis=1).transpose(1, 0, 2)         # [nG - 29, 15, 30]
    Y = np.lib.stride_tricks.sliding_window_view(tob[1], R.SEG, axis=1).transpose(1, 0, 2)
    Xh, Yh = _row_col_normalise(X.astype(dtype), eps), _row_col_normalise(Y.astype(dtype), eps)
    st["score"] = float((Xh * Yh).sum(dtype=dtype) / dtype(R.SEG * (nG - R.SEG + 1)))
    return st


def estoi(ref: np.ndarray, est: np.ndarray, dtype=np.float64, length: Optional[int] = None) -> float:
    return estoi_stages(ref, est, dtype, length)["score"]
