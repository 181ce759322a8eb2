"""Float64 restatement of the transform kernels' definitions (include/cruse_hip.h, the header comment of csrc/stft_general.hip), numpy only.

Dense DFT matrices and explicit loops over frames; nothing here is shared with the kernels or with oracle/cruse_ref.c.  tests/test_stft_ref_host.py
pins these functions (against float64 torch, the committed fixtures and their own adjoint identities) before tests/test_gpu_stft_shapes.py lets them
judge a kernel.  All spectra are frame-major [B, T, n_fft/2 + 1].

dtype = numpy.float32 in the *_f32 functions is the plainest float32 evaluation of the same formula: f32 twiddles and one sequential f32 sum per
output, which sets the bar for the direct-DFT kernels at the sizes (n_fft 2048, 4096) for which the project has no number of its own.
"""
import numpy as np

ENV_FLOOR = 1e-11          # istft writes 0 where the window-square envelope is not above this (torch.istft refuses such a case: NOLA)


def hann(n_fft):
    """periodic Hann window, 0.5 - 0.5 cos(2 pi n / N)"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def _phase(rows, cols, n_fft):
    """2 pi rows x cols / n_fft, the product reduced mod n_fft as integers first"""
    return 2.0 * np.pi * ((np.asarray(rows, np.int64)[:, None] * np.asarray(cols, np.int64)[None, :]) % n_fft) / n_fft


def _hermitian_weights(n_fft):
    c = np.full(n_fft // 2 + 1, 2.0)
    c[0] = c[n_fft // 2] = 1.0
    return c


# ---------------------------------------------------------------------------------------------------------------- cruse_stft_fwd
def stft(x, n_fft, hop):
    """x [B, L] -> re, im [B, 1 + L // hop, n_fft/2 + 1]: periodic Hann, reflect padding of n_fft/2 on both sides, no normalisation."""
    x = np.asarray(x, np.float64)
    B, L = x.shape
    assert n_fft % 2 == 0 and L > n_fft // 2 and hop > 0
    T = 1 + L // hop
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    ph = _phase(np.arange(n_fft), np.arange(n_fft // 2 + 1), n_fft)                # [n, k]
    C, S = np.cos(ph), np.sin(ph)
    w = hann(n_fft)
    re = np.empty((B, T, n_fft // 2 + 1))
    im = np.empty_like(re)
    for t in range(T):
        frame = xp[:, t * hop:t * hop + n_fft] * w
        re[:, t] = frame @ C
        im[:, t] = -(frame @ S)
    return re, im


def stft_f32(x, n_fft, hop):
    """stft() in float32: f32 window and twiddles, each bin one sequential f32 sum over n."""
    f = np.float32
    x = np.asarray(x, f)
    B, L = x.shape
    T = 1 + L // hop
    xp = np.pad(x, ((0, 0), (n_fft // 2, n_fft // 2)), mode="reflect")
    k = np.arange(n_fft // 2 + 1)
    tab_c = np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft).astype(f)
    tab_s = np.sin(2.0 * np.pi * np.arange(n_fft) / n_fft).astype(f)
    w = f(0.5) - f(0.5) * tab_c
    frames = np.stack([xp[:, t * hop:t * hop + n_fft] * w for t in range(T)], axis=1)          # [B, T, n] f32
    re = np.zeros((B, T, k.size), f)
    im = np.zeros_like(re)
    for n in range(n_fft):
        idx = (n * k) % n_fft
        re += frames[:, :, n, None] * tab_c[idx]
        im -= frames[:, :, n, None] * tab_s[idx]
    assert re.dtype == f and im.dtype == f
    return re, im


# ---------------------------------------------------------------------------------------------------------------- cruse_istft_fwd / _bwd
def envelope(T, n_fft, hop):
    """sum over frames of window^2, in padded coordinates [0, n_fft + hop (T - 1))"""
    env = np.zeros(n_fft + hop * (T - 1))
    w2 = hann(n_fft) ** 2
    for t in range(T):
        env[t * hop:t * hop + n_fft] += w2
    return env


def istft(re, im, n_fft, hop, L):
    """re, im [B, T, n_fft/2 + 1] -> [B, L]: overlap-add of window * irfft(frame), divided by the window-square envelope, samples
    [n_fft/2, n_fft/2 + L) of it; 0 where the envelope is <= 1e-11.  The imaginary parts of bins 0 and n_fft/2 are ignored."""
    re, im = np.asarray(re, np.float64), np.array(im, np.float64)
    B, T, nb = re.shape
    assert nb == n_fft // 2 + 1 and 0 < L <= n_fft + hop * (T - 1) - n_fft // 2
    im[..., 0] = 0.0
    im[..., n_fft // 2] = 0.0
    ph = _phase(np.arange(nb), np.arange(n_fft), n_fft)                             # [k, n]
    c = _hermitian_weights(n_fft)[:, None] / n_fft
    C, S = c * np.cos(ph), c * np.sin(ph)
    w = hann(n_fft)
    y = np.zeros((B, n_fft + hop * (T - 1)))
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += (re[:, t] @ C - im[:, t] @ S) * w
    env = envelope(T, n_fft, hop)
    ok = env > ENV_FLOOR
    out = np.zeros_like(y)
    out[:, ok] = y[:, ok] / env[ok]
    return out[:, n_fft // 2:n_fft // 2 + L]


def istft_adjoint(dwave, T, n_fft, hop):
    """the transpose of istft(., n_fft, hop, L = dwave.shape[1]) as a linear map of (re, im): dwave [B, L] -> dre, dim [B, T, n_fft/2 + 1].
    Closed form: divide by the envelope (0 where istft writes 0), place at n_fft/2 in padded coordinates, window each frame, and project on
    c_k cos / n_fft and -c_k sin / n_fft; bins 0 and n_fft/2 of dim are 0 because istft ignores those inputs."""
    d = np.asarray(dwave, np.float64)
    B, L = d.shape
    assert 0 < L <= n_fft + hop * (T - 1) - n_fft // 2
    env = envelope(T, n_fft, hop)
    g = np.zeros((B, env.size))
    g[:, n_fft // 2:n_fft // 2 + L] = d
    ok = env > ENV_FLOOR
    g[:, ok] /= env[ok]
    g[:, ~ok] = 0.0
    nb = n_fft // 2 + 1
    ph = _phase(np.arange(n_fft), np.arange(nb), n_fft)                             # [n, k]
    c = _hermitian_weights(n_fft)[None, :] / n_fft
    C, S = c * np.cos(ph), c * np.sin(ph)
    w = hann(n_fft)
    dre = np.empty((B, T, nb))
    dim = np.empty_like(dre)
    for t in range(T):
        frame = g[:, t * hop:t * hop + n_fft] * w
        dre[:, t] = frame @ C
        dim[:, t] = -(frame @ S)
    dim[..., 0] = 0.0
    dim[..., n_fft // 2] = 0.0
    return dre, dim


# ---------------------------------------------------------------------------------------------------------------- cruse_stft_framed / _istft_framed
def framed_frames(L, n_fft, hop, pad):
    """the default frame count of feature.stft_framed"""
    return (L + 2 * pad - n_fft) // hop + 1


def _padded(x, pad, pad_mode, need, dtype):
    """x_pad = the clip with `pad` samples in front (zeros, or reflected) and as many behind as `need` asks for"""
    x = np.asarray(x, dtype)
    L = x.shape[1]
    back = max(0, need - pad - L)
    if pad_mode in ("zeros", "constant", 0):
        return np.pad(x, ((0, 0), (pad, back)))
    assert pad_mode in ("reflect", 1) and pad < L and back < L, "a reflection that leaves the clip is not defined"
    return np.pad(x, ((0, 0), (pad, back)), mode="reflect")


def stft_framed(x, window, n_fft, hop, win_off, pad, pad_mode, T, scale):
    """X[b,t,f] = scale * sum_{n < win_len} w[n] * x_pad[b, t*hop + n + win_off] * exp(-2 pi i f (n + win_off) / n_fft)  ->  re, im [B, T, n_fft/2+1]"""
    w = np.asarray(window, np.float64)
    win_len = w.size
    assert win_len + win_off <= n_fft
    xp = _padded(x, pad, pad_mode, (T - 1) * hop + win_off + win_len, np.float64)
    ph = _phase(np.arange(win_len) + win_off, np.arange(n_fft // 2 + 1), n_fft)     # [n, f]
    C, S = np.cos(ph), np.sin(ph)
    re = np.empty((xp.shape[0], T, n_fft // 2 + 1))
    im = np.empty_like(re)
    for t in range(T):
        frame = scale * w * xp[:, t * hop + win_off:t * hop + win_off + win_len]
        re[:, t] = frame @ C
        im[:, t] = -(frame @ S)
    return re, im


def istft_framed(re, im, window, post, n_fft, hop, win_off, pad, L, scale, hermitian):
    """y[b,m] = post[m] * sum_{t,n : t*hop + n + win_off - pad == m} w[n] * scale * sum_f c_f (re cos - im sin)(2 pi f (n + win_off) / n_fft),
    c_f = 1, or with hermitian the weights 1, 2, .., 2, 1; post None = 1.  -> [B, L], 0 where no frame lands."""
    re, im = np.asarray(re, np.float64), np.asarray(im, np.float64)
    w = np.asarray(window, np.float64)
    B, T, nb = re.shape
    win_len = w.size
    assert nb == n_fft // 2 + 1 and win_len + win_off <= n_fft
    c = (_hermitian_weights(n_fft) if hermitian else np.ones(nb))[:, None]
    ph = _phase(np.arange(nb), np.arange(win_len) + win_off, n_fft)                 # [f, n]
    C, S = c * np.cos(ph), c * np.sin(ph)
    y = np.zeros((B, L))
    for t in range(T):
        frame = scale * w * (re[:, t] @ C - im[:, t] @ S)                           # [B, win_len]
        m0 = t * hop + win_off - pad
        lo, hi = max(0, -m0), min(win_len, L - m0)
        if lo < hi:
            y[:, m0 + lo:m0 + hi] += frame[:, lo:hi]
    if post is not None:
        y *= np.asarray(post, np.float64)
    return y


def stft_framed_f32(x, window, n_fft, hop, win_off, pad, pad_mode, T, scale):
    """stft_framed() in float32, each bin one sequential f32 sum over n."""
    f = np.float32
    w = np.asarray(window, f)
    win_len = w.size
    xp = _padded(x, pad, pad_mode, (T - 1) * hop + win_off + win_len, f)
    k = np.arange(n_fft // 2 + 1)
    tab_c = np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft).astype(f)
    tab_s = np.sin(2.0 * np.pi * np.arange(n_fft) / n_fft).astype(f)
    frames = np.stack([xp[:, t * hop + win_off:t * hop + win_off + win_len] * w * f(scale) for t in range(T)], axis=1)
    re = np.zeros((xp.shape[0], T, k.size), f)
    im = np.zeros_like(re)
    for n in range(win_len):
        idx = ((n + win_off) * k) % n_fft
        re += frames[:, :, n, None] * tab_c[idx]
        im -= frames[:, :, n, None] * tab_s[idx]
    assert re.dtype == f and im.dtype == f
    return re, im


def istft_framed_f32(re, im, window, post, n_fft, hop, win_off, pad, L, scale, hermitian):
    """istft_framed() in float32: each frame sample one sequential f32 sum over the bins, frames added in order."""
    f = np.float32
    re, im, w = np.asarray(re, f), np.asarray(im, f), np.asarray(window, f)
    B, T, nb = re.shape
    win_len = w.size
    c = (_hermitian_weights(n_fft) if hermitian else np.ones(nb)).astype(f)
    tab_c = np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft).astype(f)
    tab_s = np.sin(2.0 * np.pi * np.arange(n_fft) / n_fft).astype(f)
    n = np.arange(win_len) + win_off
    acc = np.zeros((B, T, win_len), f)
    for k in range(nb):
        idx = (k * n) % n_fft
        acc += (re[:, :, k, None] * c[k]) * tab_c[idx] - (im[:, :, k, None] * c[k]) * tab_s[idx]
    assert acc.dtype == f
    y = np.zeros((B, L), f)
    for t in range(T):
        m0 = t * hop + win_off - pad
        lo, hi = max(0, -m0), min(win_len, L - m0)
        if lo < hi:
            y[:, m0 + lo:m0 + hi] += acc[:, t, lo:hi] * w[lo:hi] * f(scale)
    if post is not None:
        y *= np.asarray(post, f)
    return y


def rel_l2(got, want):
    """||got - want|| / ||want|| over all elements, in float64; several arrays (re, im) count as one vector"""
    if isinstance(got, (tuple, list)):
        got = np.concatenate([np.asarray(g, np.float64).ravel() for g in got])
        want = np.concatenate([np.asarray(g, np.float64).ravel() for g in want])
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))
