"""Case tables and seeded inputs shared by tests/test_stft_ref_host.py (CPU: pins tests/stft_ref.py) and tests/test_gpu_stft_shapes.py (the kernels).

Every clip is under 6000 samples and every batch has B = 3 clips, so the (clip, tile) split of blockIdx.x is in play wherever a clip has more than one
tile.  The F32_* figures are the relative-L2 distance between the float32 evaluation of tests/stft_ref.py (stft_f32, stft_framed_f32,
istft_framed_f32: f32 twiddles, one sequential f32 sum per output) and its float64 evaluation on the very inputs below, measured on the CPU; the bar
for a direct-DFT kernel at n_fft 2048 / 4096 is 4 x that figure (the factor covers another summation order and sincospif against cos, nothing more).
tests/test_stft_ref_host.py recomputes every figure and fails if a recorded one is off.
"""
import numpy as np

B = 3
NFFT = 320


def _f32(a):
    """float64 holding float32 values: the kernels and the float64 reference then see the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


def wave(seed, L, b=B):
    return _f32(0.1 * np.random.default_rng(seed).standard_normal((b, L)))


def spectrum(seed, T, nb, b=B):
    """randn (re, im) [b, T, nb]; the imaginary parts of the first and the last bin are NOT zero"""
    g = np.random.default_rng(seed)
    return _f32(g.standard_normal((b, T, nb))), _f32(g.standard_normal((b, T, nb)))


def window(seed, n):
    """a random window with no symmetry: a reversed or shifted window index cannot pass"""
    return _f32(np.random.default_rng(seed).uniform(0.2, 1.0, n))


def positive(seed, n):
    return _f32(np.random.default_rng(seed).uniform(0.5, 2.0, n))


# ---------------------------------------------------------------------------------------------------------------- cruse_stft_fwd, 320-point FFT path
# (hop, L): the smallest legal clip (161: one frame reflects at both ends), both reflections inside one frame, T = 15 / 16 / 17 (one 16-frame tile less
# one, exactly, plus one) and tile remainder 1; then hops that do not divide 320, hop 1 (2001 frames) and the hop = n_fft limit
STFT_FFT = [(160, L) for L in (161, 162, 319, 320, 321, 2399, 2400, 2401, 2560)] + [(hop, 2000) for hop in (1, 64, 80, 100, 319, 320)]
STFT_IMPULSES = [(L, pos) for L in (161, 321) for pos in (0, 1, L - 2, L - 1)]
STFT_MAG_FORMS = [(bins, eps) for bins in (1, 160, 161) for eps in (0.0, 1e-8)]
STFT_FORMS_AT = [(160, 321), (100, 2000), (160, 2560)]               # (hop, L) at which the output forms are compared with the full call

# ---------------------------------------------------------------------------------------------------------------- cruse_stft_fwd, direct DFT
# (n_fft, hop, L, tolerance): 1e-4 is the project's bar for this kernel at n_fft <= 512; at 2048 it is 4 x the f32 distance
F32_STFT_2048_1025 = 7.91e-7
F32_STFT_2048_5000 = 8.08e-7
STFT_DFT = [(2, 1, 2, 1e-4), (4, 3, 9, 1e-4), (64, 16, 33, 1e-4), (322, 161, 700, 1e-4), (320, 321, 1000, 1e-4), (512, 128, 257, 1e-4),
            (512, 600, 2000, 1e-4),
            (2048, 512, 1025, 4 * F32_STFT_2048_1025),                # f32 distance 7.91e-7, bar 3.16e-6
            (2048, 512, 5000, 4 * F32_STFT_2048_5000)]                # f32 distance 8.08e-7, bar 3.23e-6
F32_STFT = {(2048, 512, 1025): F32_STFT_2048_1025, (2048, 512, 5000): F32_STFT_2048_5000}

STFT_ALL = [(NFFT, hop, L) for hop, L in STFT_FFT] + [c[:3] for c in STFT_DFT]


def stft_seed(n_fft, hop, L):
    return 10 + STFT_ALL.index((n_fft, hop, L))


# (n_fft, hop, L, mag_bins or None): refused as shape errors before any launch
STFT_REFUSED = [(320, 160, 160, None), (321, 160, 400, None), (2050, 512, 3000, None), (320, 160, 400, 162), (512, 128, 600, 258), (320, 0, 400, None)]

# ---------------------------------------------------------------------------------------------------------------- cruse_istft_fwd / cruse_istft_bwd
ISTFT_T_HOP = [(1, 160), (2, 160), (16, 160), (17, 160), (33, 160), (20, 80), (20, 100), (20, 64), (7, 319), (7, 320)]


def istft_max_len(T, hop):
    return hop * (T - 1) + NFFT // 2


def _istft_cases():
    out = []
    for T, hop in ISTFT_T_HOP:
        top = istft_max_len(T, hop)
        want = [1, hop * (T - 1), top, 15 * hop - 1, 15 * hop, 15 * hop + 1]         # 15 * hop: the output tile of one workgroup
        out += [(T, hop, L) for L in sorted({L for L in want if 0 < L <= top})]
    return out


ISTFT = _istft_cases()                                                               # (T, hop, L)
ISTFT_ROUND_TRIPS = [(160, 2400), (100, 2000), (64, 1280)]                           # (hop, L): istft(stft(x)) == x with T = 1 + L // hop

# ---------------------------------------------------------------------------------------------------------------- cruse_stft_framed / cruse_istft_framed
# (n_fft, win_len, win_off, hop, pad, pad_mode, L, T or None = (L + 2 pad - n_fft) // hop + 1)
FRAMED = [(320, 320, 0, 160, 0, "zeros", 800, None),
          (512, 320, 0, 160, 0, "zeros", 800, None),
          (512, 300, 7, 130, 0, "zeros", 1000, None),
          (64, 64, 0, 16, 48, "reflect", 49, None),
          (64, 64, 0, 16, 48, "zeros", 200, None),
          (2, 1, 1, 1, 0, "zeros", 5, 4),
          (384, 100, 284, 250, 0, "zeros", 900, None),                               # hop > win_len leaves gaps
          (320, 320, 0, 160, 160, "reflect", 640, 5),
          (320, 320, 0, 160, 0, "zeros", 640, 9),                                    # frames past the clip end, zero-fed
          (4096, 4096, 0, 1024, 0, "zeros", 5120, 2),                                # f32 distance: forward 1.156e-6, inverse 8.22e-7
          (4096, 257, 100, 4096, 0, "zeros", 4200, 1)]                               # f32 distance: forward 2.98e-7, inverse 8.08e-7
FRAMED_SCALES = (1.0, float(np.float32(0.37)))
F32_FRAMED_FWD = {(4096, 4096): 1.156e-6, (4096, 257): 2.98e-7}                       # by (n_fft, win_len); the worst of the scales
F32_FRAMED_INV = {(4096, 4096): 8.22e-7, (4096, 257): 8.08e-7}                       # the worst of scale, hermitian, post and the three lengths


def framed_T(case):
    n_fft, win_len, win_off, hop, pad, mode, L, T = case
    return T if T is not None else (L + 2 * pad - n_fft) // hop + 1


def framed_span(case):
    """one past the last output sample a frame lands on"""
    n_fft, win_len, win_off, hop, pad, mode, L, T = case
    return (framed_T(case) - 1) * hop + win_off + win_len - pad


def framed_fwd_tol(case):
    return 4 * F32_FRAMED_FWD[case[:2]] if case[0] > 512 else 1e-5


def framed_inv_tol(case):
    return 4 * F32_FRAMED_INV[case[:2]] if case[0] > 512 else 1e-5


def framed_seed(case):
    return 1000 + FRAMED.index(case)
