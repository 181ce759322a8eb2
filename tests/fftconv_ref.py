"""Plain numpy / scipy references for cruse_fftconv_* and the reverberation built on it: the float64 truth, an f32
restatement of the kernel's partition schedule, the synthetic room impulse response, add_reverb, and the bar.

The bar is measured against the reference's own arithmetic, not fixed: scipy's f32 fftconvolve(x, h)[:L] is what
SynDataset.snr_mix / add_reverb commit against float64; the kernel is allowed FACTOR = 4 times that (another radix, twiddle
source and summation order), per clip in rel-L2 and in max |y - ref| / peak |ref|, never less than FLOOR = 4 * 2^-23 (cases where
scipy is exact, L = R = 1) and, in rel-L2, never more than CAP = 5e-6, the project's bar for this operation (fixture G20)."""
import numpy as np
import scipy.fft
import scipy.signal

P = 2048                       # asserted against ops.FFTCONV_PART / CRUSE_FFTCONV_PART by the tests
FACTOR, FLOOR, CAP = 4.0, 4.0 * 2.0 ** -23, 5e-6


def truth(x, h, L=None):
    """float64 fftconvolve(x[b], h[b or 0])[:L] per clip; np.convolve (exact order of sums) for small cases"""
    x, h = np.atleast_2d(np.asarray(x, dtype=np.float64)), np.atleast_2d(np.asarray(h, dtype=np.float64))
    L = x.shape[1] if L is None else L
    out = np.empty((x.shape[0], L))
    for b in range(x.shape[0]):
        hb = h[b if h.shape[0] > 1 else 0]
        full = np.convolve(x[b], hb) if x.shape[1] * len(hb) <= 1 << 24 else scipy.signal.fftconvolve(x[b], hb)
        out[b] = full[:L]
    return out


def scipy_f32(x, h):
    """the reference's arithmetic: scipy.signal.fftconvolve on f32 arrays stays f32"""
    x, h = np.atleast_2d(np.asarray(x, dtype=np.float32)), np.atleast_2d(np.asarray(h, dtype=np.float32))
    out = np.stack([scipy.signal.fftconvolve(x[b], h[b if h.shape[0] > 1 else 0])[:x.shape[1]] for b in range(x.shape[0])])
    assert out.dtype == np.float32
    return out


def restatement(x, h, early_len=None, part=P):
    """the kernel's schedule in f32: spectra of the zero-padded partitions of h, spectra of the blocks x[(i-1)P : (i+1)P), per output
    block the sum over partitions in ascending order, inverse transform, second half.  -> y, or (y, y_early)"""
    x, h = np.atleast_2d(np.asarray(x, dtype=np.float32)), np.atleast_2d(np.asarray(h, dtype=np.float32))
    B, L = x.shape
    R = h.shape[1]
    nblk, npart = -(-L // part), -(-R // part)

    def spectra(a, n, shift):
        pad = np.zeros((a.shape[0], shift + n * part + part), dtype=np.float32)
        pad[:, shift:shift + a.shape[1]] = a
        out = np.stack([scipy.fft.rfft(pad[:, i * part:(i + 2) * part], axis=1) for i in range(n)], axis=1)
        assert out.dtype == np.complex64
        return out

    def run(hh):
        hz = np.zeros((hh.shape[0], npart * part), dtype=np.float32)
        hz[:, :R] = hh
        H = np.stack([scipy.fft.rfft(np.concatenate([hz[:, j * part:(j + 1) * part], np.zeros((hh.shape[0], part), np.float32)], axis=1), axis=1)
                      for j in range(npart)], axis=1)
        X = spectra(x, nblk, part)                                        # block i = samples (i-1)P .. (i+1)P
        y = np.zeros((B, nblk * part), dtype=np.float32)
        for i in range(nblk):
            acc = np.zeros((B, part + 1), dtype=np.complex64)
            for j in range(min(npart, i + 1)):
                acc = acc + X[:, i - j] * (H[:, j] if H.shape[0] > 1 else H[0, j])
            y[:, i * part:(i + 1) * part] = scipy.fft.irfft(acc, n=2 * part, axis=1)[:, part:]
        assert y.dtype == np.float32
        return y[:, :L]

    y = run(h)
    if early_len is None:
        return y
    el = np.clip(np.broadcast_to(np.asarray(early_len), (h.shape[0],)), 0, R)
    return y, run(np.where(np.arange(R)[None, :] < el[:, None], h, np.float32(0)))


def errors(got, ref):
    """per clip: rel-L2 and max |d| / peak |ref| of got against the float64 ref"""
    got, ref = np.atleast_2d(got).astype(np.float64), np.atleast_2d(ref)
    assert got.shape == ref.shape and np.isfinite(got).all()
    d = got - ref
    nrm = np.maximum(np.sqrt((ref ** 2).sum(axis=1)), 1e-300)
    pk = np.maximum(np.abs(ref).max(axis=1), 1e-300)
    return np.sqrt((d ** 2).sum(axis=1)) / nrm, np.abs(d).max(axis=1) / pk


def bars(x, h, ref):
    """per clip (rel-L2 bar, max-abs bar) from scipy's own f32 error on this case"""
    e2, em = errors(scipy_f32(x, h), ref)
    return np.minimum(np.maximum(FACTOR * e2, FLOOR), CAP), np.maximum(FACTOR * em, FLOOR)


def ratio(got, x, h, ref=None):
    """worst of (error / bar) over the clips and the two measures; <= 1 passes"""
    ref = truth(x, h) if ref is None else ref
    b2, bm = bars(x, h, ref)
    e2, em = errors(got, ref)
    return float(max((e2 / b2).max(), (em / bm).max()))


def signal_like(B, L, seed):
    """speech-like clips in the manner of data.synth_batch: 0.05 N(0,1) through a one-pole low-pass (a = 0.95, 64 taps), times 4"""
    rng = np.random.default_rng(seed)
    w = 0.05 * rng.standard_normal((B, L + 63))
    taps = 0.05 * 0.95 ** np.arange(64)
    return (4.0 * np.stack([np.convolve(w[b], taps, mode="valid") for b in range(B)])).astype(np.float32)


def synth_rir(n, R, seed, rt60_low=0.2, rt60_high=0.8, sr=16000, max_delay_ms=15):
    """[n, R] f32: a unit direct path after 0 .. max_delay_ms, then 0.3 N(0,1) 10^(-3 k / (rt60 sr)) (data.synth_rirs's recipe, numpy's
    draws)"""
    rng = np.random.default_rng(seed)
    delay = np.minimum(rng.integers(0, max_delay_ms * sr // 1000 + 1, size=n), R - 1)
    rt60 = rng.uniform(rt60_low, rt60_high, size=n)
    k = np.arange(R)
    h = 0.3 * rng.standard_normal((n, R)) * 10.0 ** (-3.0 * k[None, :] / (rt60[:, None] * sr))
    h[k[None, :] < delay[:, None]] = 0.0
    h[np.arange(n), delay] = 1.0
    return h.astype(np.float32)


def early_len(rir, predelay=50, sr=16000):
    """add_reverb's et per row of rir [n, R]: argmax of the VALUES + predelay ms (not clamped)"""
    return np.argmax(np.atleast_2d(rir), axis=1) + (predelay * sr) // 1000


def add_reverb(cln, rir, predelay=50, sr=16000, conv=truth):
    """(wav_tgt, wav_early_tgt) [B, L] as SynDataset.add_reverb defines them, through `conv`"""
    cln, rir = np.atleast_2d(cln), np.atleast_2d(rir)
    et = np.minimum(early_len(rir, predelay, sr), rir.shape[1])
    cut = np.where(np.arange(rir.shape[1])[None, :] < et[:, None], rir, 0).astype(rir.dtype)
    return conv(cln, rir), conv(cln, cut)


# the shapes of the GPU test: every L with every R (R > L included), each as one clip, and as three clips with one shared filter, a
# filter per clip, and a bank of two filters behind an index that repeats one
def gpu_lengths(part=P):
    return [1, 2, part - 1, part, part + 1, 2 * part + 1, 4099]


def gpu_taps(part=P):
    return [1, 2, 600, part - 1, part, part + 1, 2 * part + 1]


BANKS = ((1, "shared"), (3, "shared"), (3, "per_clip"), (3, "indexed"))


def case(B, L, R, bank, seed=0):
    """-> x [B, L], bank h [NR, R], index (int32 [B] or None), and the per-clip filters hb [B, R] the index selects.  The direct path
    sits at tap 0: a clip of one or two samples must still see it, an all-zero reference has no relative error."""
    x = signal_like(B, L, seed + 7 * L + R)
    if bank == "indexed":
        h = synth_rir(2, R, seed + L + 13 * R, max_delay_ms=0)
        idx = np.array([1, 0, 1], dtype=np.int32)[:B]
        return x, h, idx, h[idx]
    h = synth_rir(B if bank == "per_clip" else 1, R, seed + L + 13 * R, max_delay_ms=0)
    return x, h, None, np.broadcast_to(h, (B, R)) if bank == "shared" else h
