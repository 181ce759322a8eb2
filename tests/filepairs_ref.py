"""The reference side of the file-list dataset tests, numpy / scipy only.  The reference's SynDataset cannot be
imported (librosa, soundfile, joblib, tqdm), so its algorithm is restated here: float64 resampling through scipy with the designed
taps, _select_clean_y / _select_noise_y (dataset/dataset.py:147-203) over in-memory utterances with an injected generator, a plan
executor, snr_mix (:244-260) in float64, and the corpus the GPU tests write."""
import os
import wave

import numpy as np
from scipy import signal

from cruse_amd import resample_design as D

POOL_RATE = 16000
CAP = 1e-6                         # the bar is never looser than this (rel-L2)
FLOOR = 4 * 2.0 ** -23             # ... and never tighter than 4 roundings of an f32 (the floor of tests/test_gpu_fftconv.py)
RATES = (8000, 48000, 24000, 44100, 11025)


def taps64(up, down):
    return D.design(up, down)


def resample64(x, up, down):
    """the definition: scipy.signal.resample_poly in float64 with the designed window"""
    x = np.asarray(x, dtype=np.float64)
    if (up, down) == (1, 1):
        return x.copy()
    return signal.resample_poly(x, up, down, window=taps64(up, down))


def resample32(x, up, down):
    """what a user of the reference's arithmetic gets: scipy's own f32 path (f32 samples, f32 window)"""
    y = signal.resample_poly(np.asarray(x, dtype=np.float32), up, down, window=taps64(up, down).astype(np.float32))
    assert y.dtype == np.float32
    return y


def errors(got, want):
    """(rel-L2, max |d| / peak) of `got` against the float64 `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = got - want
    return float(np.linalg.norm(d) / max(np.linalg.norm(want), 1e-300)), float(np.abs(d).max() / max(np.abs(want).max(), 1e-300))


def bars(x, up, down):
    """-> (float64 truth, rel-L2 bar, max-abs bar) of one clip: 4 x scipy-f32's own error against float64, the rel-L2 bar never above
    CAP, neither below FLOOR.  Asserts first that scipy-f32 itself is inside the cap, so the cap cannot hide a failure."""
    want = resample64(x, up, down)
    e2, em = errors(resample32(x, up, down), want)
    assert e2 <= CAP, (up, down, len(x), e2)
    return want, min(max(4 * e2, FLOOR), CAP), max(4 * em, FLOOR)


def harmonic(n, rate, seed, f0=None):
    """a seeded harmonic stack plus noise at `rate`, peak below 0.9: not silence, and with content up to the band edge"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    f0 = f0 or rng.uniform(90.0, 280.0)
    x = sum(rng.uniform(0.2, 1.0) / (k + 1) * np.sin(2 * np.pi * f0 * (k + 1) * t + rng.uniform(0, 6.28)) for k in range(12))
    x = x + 0.1 * rng.standard_normal(n)
    return 0.9 * x / (np.abs(x).max() + 1e-12)


def to_pcm(x):
    return np.clip(np.rint(np.asarray(x) * 32767.0), -32768, 32767).astype(np.int16)


def write_wav(path, pcm, rate, channels=1, width=2):
    """pcm: int16 [frames * channels] interleaved (uint8 for width 1)"""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


# ---- SynDataset._select_clean_y / _select_noise_y, restated over in-memory utterances -------------------------------------------
def select_ref(first, utterances, target, silence_len, rng):
    """first = an index (clean, :147-182) or None (noise, :184-203).  random.choice -> rng.integers(len(list)); np.random.randint(n) ->
    rng.integers(n): the draws plan_clip makes, in its order."""
    y = np.zeros(0, dtype=np.float64) if first is None else np.asarray(utterances[first], dtype=np.float64)
    silence = np.zeros(silence_len)
    remain = target - len(y)
    while remain > 0:
        new = utterances[int(rng.integers(len(utterances)))]
        y = np.append(y, new)
        remain -= len(new)
        if remain > 0:
            n = min(remain, len(silence))
            y = np.append(y, silence[:n])
            remain -= n
    if len(y) > target:
        s = int(rng.integers(len(y) - target))
        y = y[s:s + target]
    assert len(y) == target
    return y


def execute_plan(rows, utterances, target):
    """rows [nseg, 4] (utterance, offset, dst, len) -> the clip"""
    y = np.zeros(target, dtype=np.float64)
    for u, off, dst, n in np.asarray(rows).reshape(-1, 4):
        y[dst:dst + n] = np.asarray(utterances[u])[off:off + n]
    return y


def execute_segs(seg, first, pool, L):
    """the device plan: seg [nseg, 3] (src, dst, len), first [B + 1] over the flat pool -> [B, L] in the pool's dtype"""
    out = np.zeros((len(first) - 1, L), dtype=pool.dtype)
    for b in range(len(first) - 1):
        for src, dst, n in seg[first[b]:first[b + 1]]:
            out[b, dst:dst + n] = pool[src:src + n]
    return out


def snr_mix64(c, n, snr, eps=1e-7):
    """SynDataset.snr_mix (:251-260) per row in float64 -> (noisy, clean, scaled noise)"""
    c, n = np.asarray(c, dtype=np.float64), np.asarray(n, dtype=np.float64)
    c = c / (np.abs(c).max(axis=1, keepdims=True) + eps)
    n = n / (np.abs(n).max(axis=1, keepdims=True) + eps)
    scalar = np.sqrt((c ** 2).mean(axis=1)) / 10 ** (np.asarray(snr, dtype=np.float64) / 20) / (np.sqrt((n ** 2).mean(axis=1)) + eps)
    n = n * scalar[:, None]
    return c + n, c, n


# ---- the corpus of tests/test_gpu_file_dataset.py ------------------------------------------------------------------------------------
CLEAN = ((16000, 1, 0.30), (8000, 1, 0.05), (44100, 1, 0.21), (16000, 2, 0.11), (44100, 1, 0.07), (8000, 1, 0.26))   # (rate, channels, seconds)
NOISE = ((16000, 1, 0.25), (44100, 1, 0.12), (8000, 1, 0.30), (16000, 1, 0.06))
RIRS = ((16000, 1, 0.05), (44100, 1, 0.05))
RIRS_NOISE = ((8000, 1, 0.05),)


def write_corpus(root):
    """-> {"clean" / "noise" / "rir" / "rir_noise": (list file, [(pcm int16 interleaved, channels, rate)])}"""
    out = {}
    for name, spec in (("clean", CLEAN), ("noise", NOISE), ("rir", RIRS), ("rir_noise", RIRS_NOISE)):
        paths, files = [], []
        for k, (rate, ch, sec) in enumerate(spec):
            n = int(round(sec * rate))
            seed = 1000 * (1 + len(out)) + k
            if name.startswith("rir"):                          # a direct path after a short delay and a decaying tail
                rng = np.random.default_rng(seed)
                x = 0.2 * rng.standard_normal(n) * np.exp(-np.arange(n) / (0.01 * rate))
                x[: 3 + k] = 0.0
                x[3 + k] = 0.9
                x = np.clip(x, -0.95, 0.95)
            elif name == "noise":
                x = 0.5 * np.clip(np.random.default_rng(seed).standard_normal(n) / 3, -1, 1) + 0.3 * harmonic(n, rate, seed, f0=50.0)
            else:
                x = harmonic(n, rate, seed)
            cols = [to_pcm(x)] + [to_pcm(harmonic(n, rate, seed + 500)) for _ in range(ch - 1)]         # channel 0 is the one read
            pcm = np.stack(cols, axis=1).reshape(-1)
            p = os.path.join(str(root), f"{name}_{k}.wav")
            write_wav(p, pcm, rate, ch)
            paths.append(p)
            files.append((pcm, ch, rate))
        lst = os.path.join(str(root), f"{name}.lst")
        with open(lst, "w") as f:
            f.write("\n".join(paths) + "\n")
        out[name] = (lst, files)
    return out


def pool64(files):
    """[(pcm, channels, rate)] -> the list of float64 utterances at 16 kHz (channel 0, / 32768), in list order"""
    utts = []
    for pcm, ch, rate in files:
        up, down = D.ratio(POOL_RATE, rate)
        utts.append(resample64(pcm.reshape(-1, ch)[:, 0].astype(np.float64) / 32768.0, up, down))
    return utts
