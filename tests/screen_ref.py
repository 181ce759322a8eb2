"""Float64 numpy restatement of cruse_screen_clips and cruse_rt60 (include/cruse_hip.h), written from their definitions, and the inputs
tests/test_screen_host.py, tests/test_gpu_screen.py and tests/golden/make_golden_screen.py share."""
from __future__ import annotations

import math

import numpy as np

WINDOW = 800                  # int(16000 * 0.05)
CLIP_THR = 0.999
TARGET_DB = -25.0
ACT_THR = 0.13
MARGIN = 1e-3                 # no smoothed probability of a committed input lies closer to ACT_THR


def window_sums(x, window=WINDOW):
    """S_w = sum of x^2 over window w, float64; the last window is short"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([np.sum(x[s:s + window] ** 2) for s in range(0, x.shape[0], window)], dtype=np.float64)


def smoothed(x, window=WINDOW, target_db=TARGET_DB):
    """-> (rms, the smoothed probability of every window)"""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] == 0:
        return 0.0, np.zeros(0)
    rms = math.sqrt(float(np.mean(x ** 2)))
    scalar = 10.0 ** (target_db / 20.0) / (rms + 1e-6)
    e = 20.0 * np.log10(scalar * scalar * window_sums(x, window) + 1e-6)
    p = 1.0 / (1.0 + np.exp(-(-1.0 + 0.2 * e)))
    q = np.concatenate([[0.0], p[:-1]])                       # the unsmoothed value of the window before
    return rms, np.where(p > q, p * 0.8 + q * (1.0 - 0.8), p * 0.05 + q * (1.0 - 0.05))


def screen_row(x, window=WINDOW, clip_thr=CLIP_THR, target_db=TARGET_DB, act_thr=ACT_THR):
    """one row of cruse_screen_clips: peak, n_clipped, rms, n_windows, n_active, activity.  x: float32 samples"""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    if n == 0:
        return np.array([0.0, 0.0, 0.0, 0.0, 0.0, np.nan])
    a = np.abs(x)
    rms, sm = smoothed(x, window, target_db)
    nw = -(-n // window)
    na = int(np.sum(sm > act_thr))
    return np.array([float(a.max()), float(np.sum(a > np.float32(clip_thr))), rms, float(nw), float(na), na / nw])


def screen_clips(pool, start, length, **kw):
    return np.stack([screen_row(pool[s:s + n], **kw) for s, n in zip(start, length)]) if len(start) else np.zeros((0, 6))


def min_margin(x, act_thr=ACT_THR, **kw):
    _, sm = smoothed(x, **kw)
    return float(np.min(np.abs(sm - act_thr))) if sm.size else math.inf


# ---- RT60 ----------------------------------------------------------------------------------------------------------------------------
def _suffix_sums(v, order):
    """E[t] = sum_{m >= t} v[m] in float64: "sequential" from the last sample, or "pairwise": blocks of 128 summed by numpy's pairwise
    np.sum, block suffixes, and the sums inside a block"""
    if order == "sequential":
        return np.cumsum(v[::-1])[::-1]
    n = v.shape[0]
    nb = -(-n // 128)
    pad = np.concatenate([v, np.zeros(nb * 128 - n)]).reshape(nb, 128)
    tot = np.array([np.sum(r) for r in pad])
    behind = np.concatenate([np.cumsum(tot[::-1])[::-1][1:], [0.0]])
    return (np.cumsum(pad[:, ::-1], axis=1)[:, ::-1] + behind[:, None]).reshape(-1)[:n]


def _total(v, order):
    return float(np.cumsum(v)[-1]) if order == "sequential" else float(np.sum(v))


def rt60_row(h, sr=16000, lo_db=-5.0, hi_db=-25.0, order="sequential"):
    """one row of cruse_rt60: rt60 [s], t_peak, edc_floor_db.  h: float32 samples"""
    h = np.asarray(h, dtype=np.float32)
    n = h.shape[0]
    if n == 0:
        return np.array([np.nan, np.nan, np.nan])
    t0 = int(np.argmax(np.abs(h)))                            # the first index of the maximum
    E = _suffix_sums(h[t0:].astype(np.float64) ** 2, order)
    if not E[0] > 0.0:
        return np.array([np.nan, float(t0), np.nan])
    with np.errstate(divide="ignore"):
        D = 10.0 * np.log10(E / E[0])
    lo, hi = int(np.sum(D > lo_db)), int(np.sum(D > hi_db))   # E does not rise: the counts are the crossings
    rt = np.nan
    if hi - lo >= 2 and hi < D.shape[0]:
        x = np.arange(lo, hi, dtype=np.float64) - 0.5 * (lo + hi - 1)
        slope = _total(x * D[lo:hi], order) / _total(x * x, order)
        rt = -60.0 / (slope * sr)
    return np.array([rt, float(t0), float(D[-1])])


def rt60(pool, start, length, **kw):
    return np.stack([rt60_row(pool[s:s + n], **kw) for s, n in zip(start, length)]) if len(start) else np.zeros((0, 3))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def speech_like(n, seed, level=0.1):
    """bursts of noise between silences: windows are either loud (p near 1) or silent (p near 0), far from ACT_THR"""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.float64)
    pos, on = 0, True
    while pos < n:
        run = int(rng.integers(1, 4)) * WINDOW + (WINDOW // 2 if rng.random() < 0.3 else 0)
        if on:
            x[pos:pos + run] = level * rng.standard_normal(min(run, n - pos))
        pos += run
        on = not on
    return np.clip(x, -0.9, 0.9).astype(np.float32)


# rt60_order_disagreement() as measured when the GPU test's bar was set (numpy 2, x86-64): the restatement's sequential and pairwise
# orders differ by at most this much, relatively, over rt60_inputs(); the bar of tests/test_gpu_screen.py is ten times that
RT60_MEASURED = 2.0817e-15
RT60_BAR = 10.0 * RT60_MEASURED

DECAY = 6.908                 # the amplitude decay constant of the test responses: exp(-DECAY n / (T sr))


def decay_rt60(T):
    """the RT60 of the exact line exp(-DECAY n / (T sr)): 60 dB are 3 ln 10 = 6.9078 nepers, of which DECAY is the rounding"""
    return T * 3.0 * math.log(10.0) / DECAY


def decay(n, T, sr=16000, predelay=0, noise_seed=None):
    t = np.arange(n - predelay, dtype=np.float64)
    h = np.exp(-DECAY * t / (T * sr))
    if noise_seed is not None:
        h = h * np.random.default_rng(noise_seed).standard_normal(h.shape[0])
    return np.concatenate([np.zeros(predelay), h]).astype(np.float32)


def rt60_inputs():
    """(name, float32 response, the exact RT60 where the response is a noiseless line, else None; "nan" where RT60 must be NaN)"""
    ramp = np.linspace(0.01, 1.0, 300).astype(np.float32)                       # the peak is the last sample
    return [
        ("empty", np.zeros(0, dtype=np.float32), "nan"),
        ("two", np.array([1.0, 0.5], dtype=np.float32), "nan"),                 # never reaches -25 dB
        ("short64", decay(64, 0.002), None),
        ("noisy8000", decay(8000, 0.3, noise_seed=1), None),
        ("noisy8001", decay(8001, 0.25, noise_seed=2), None),
        ("line_T0.3", decay(12000, 0.3), decay_rt60(0.3)),                      # longer than a chunk of the scan (2048)
        ("line_T0.8", decay(30000, 0.8), decay_rt60(0.8)),
        ("predelay37", decay(12037, 0.3, predelay=37), decay_rt60(0.3)),
        ("noisy_predelay", decay(8001, 0.3, predelay=37, noise_seed=3), None),
        ("peak_last", ramp, "nan"),
        ("truncated", decay(200, 0.8), "nan"),                                  # its last sample alone holds more than -25 dB of E[t0]
        ("zeros", np.zeros(100, dtype=np.float32), "nan"),
    ]


def rt60_order_disagreement():
    """the largest relative disagreement of the restatement's two summation orders over rt60_inputs(): rt60 and edc_floor_db"""
    worst = 0.0
    for _, h, _ in rt60_inputs():
        a, b = rt60_row(h, order="sequential"), rt60_row(h, order="pairwise")
        assert np.array_equal(np.isnan(a), np.isnan(b)) and a[1] == b[1] or h.shape[0] == 0
        for k in (0, 2):
            if np.isfinite(a[k]) and a[k] != 0.0:
                worst = max(worst, abs(a[k] - b[k]) / abs(a[k]))
    return worst


GOLDEN_LENGTHS = (1, 799, 800, 801, 1600, 1601, 8000, 16037, 40001)


def golden_inputs():
    """the utterances of tests/golden/screen.npz: (name, float32 samples)"""
    out = [(f"speech{n}", speech_like(n, seed=11 + i, level=(0.02, 0.1, 0.4)[i % 3])) for i, n in enumerate(GOLDEN_LENGTHS)]
    sq = np.where(np.arange(2400) % 16 < 8, 1.0, -1.0).astype(np.float32)
    out.append(("square", sq))
    edge = speech_like(4000, seed=5)
    edge[1234] = np.float32(0.999)
    out.append(("edge_below", edge.copy()))
    edge[2345] = np.nextafter(np.float32(0.999), np.float32(2.0))
    out.append(("edge_above", edge))
    out.append(("zeros", np.zeros(1700, dtype=np.float32)))
    return out
