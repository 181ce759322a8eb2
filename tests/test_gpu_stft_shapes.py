"""The transform kernels (csrc/stft.hip, csrc/stft_general.hip) against the float64 restatement tests/stft_ref.py at the lengths, hops, windows and
output forms where such kernels go wrong: the smallest clip, a frame that reflects at both ends, one 16-frame tile and one more, hops that do not
divide n_fft, hop = n_fft (the Hann window's zero lands on a sample that no other frame covers), the longest output the frames allow, output lengths
inside / on / past the 15-hop tile, windows at an offset, frames past the clip end, the n_fft limits.  tests/test_stft_ref_host.py pins the reference
on the CPU over the same tables (tests/stft_cases.py).

Bars: the project's own for the same kernel and path -- relative L2 1e-5 on the 320-point FFT path (and max-abs 2e-5 on 0.1-scale data), 1e-5 for
the iSTFT and its adjoint, 1e-4 for the direct DFT at n_fft <= 512, 1e-5 for the framed pair at n_fft <= 512; at n_fft 2048 / 4096, 4 x the distance
of the reference's own float32 evaluation to its float64 one (figures in tests/stft_cases.py).  Each test walks one table and reports every failing
case with its tuple."""
import numpy as np
import pytest
import torch

from tests import stft_cases as C
from tests import stft_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from cruse_amd import ops as o
    return o


@pytest.fixture(scope="module")
def feature():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from cruse_amd.acoustics import feature as f
    return f


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Bad(list):
    """failures of one table, collected with their case"""

    def close(self, tag, got, want, tol, what="rel L2"):
        e = R.rel_l2([host(g) for g in got] if isinstance(got, (tuple, list)) else host(got), want)
        print(f"{tag} {what}: {e:.3e} (bar {tol:.3e})")
        if not e <= tol:
            self.append((tag, what, e, tol))

    def near(self, tag, got, want, tol, what="max abs"):
        g = host(got)
        e = float(np.abs(g - want).max()) if np.isfinite(g).all() else float("inf")
        print(f"{tag} {what}: {e:.3e} (bar {tol:.3e})")
        if not e <= tol:
            self.append((tag, what, e, tol))

    def parts(self, tag, got, want, tol):
        """(re, im) as one vector, then each part on its own -- unless that part of the reference is identically 0 up to float64 rounding (a frame
        that is symmetric about its centre has a real spectrum; sin(pi k) = 0), where a relative measure means nothing and the combined one holds"""
        self.close(tag, got, want, tol)
        whole = np.sqrt(np.sum(want[0] ** 2) + np.sum(want[1] ** 2))
        for g, w, name in ((got[0], want[0], "re"), (got[1], want[1], "im")):
            if np.linalg.norm(w) > 1e-9 * whole:
                self.close(tag, g, w, tol, name + " rel L2")
            else:
                self.near(tag, g, w, tol * whole, name + " (reference 0) max abs")

    def true(self, tag, cond, what):
        if not cond:
            self.append((tag, what))


def refused(fn, match):
    try:
        fn()
    except RuntimeError as ex:
        return match in str(ex)
    return False


# ---------------------------------------------------------------------------------------------------------------- cruse_stft_fwd
def test_stft_fft_path_lengths_and_hops(ops):
    bad = Bad()
    for hop, L in C.STFT_FFT:
        x = C.wave(C.stft_seed(C.NFFT, hop, L), L)
        want = R.stft(x, C.NFFT, hop)
        re, im, _ = ops.stft(dev(x), C.NFFT, hop)
        tag = ("fft", hop, L)
        bad.true(tag, re.shape == im.shape == (C.B, 1 + L // hop, 161), "shape")
        bad.parts(tag, (re, im), want, 1e-5)
        bad.near(tag, re, want[0], 2e-5)
        bad.near(tag, im, want[1], 2e-5)
    assert not bad, "\n".join(map(str, bad))


def test_stft_impulses_in_the_smallest_clips(ops):
    """a one-hot sample pins frame placement and both reflections: at L = 161 frame 1 reflects at both ends"""
    bad = Bad()
    for L, pos in C.STFT_IMPULSES:
        x = np.zeros((C.B, L))
        x[:, pos] = 1.0
        want = R.stft(x, C.NFFT, 160)
        re, im, _ = ops.stft(dev(x), C.NFFT, 160)
        bad.near(("impulse", L, pos), re, want[0], 1e-5)
        bad.near(("impulse", L, pos), im, want[1], 1e-5)
    assert not bad, "\n".join(map(str, bad))


def test_stft_output_forms_equal_the_full_call_bit_for_bit(ops):
    bad = Bad()
    for n_fft, hop, L in [(C.NFFT, hop, L) for hop, L in C.STFT_FORMS_AT] + [(512, 128, 257)]:
        x = dev(C.wave(C.stft_seed(n_fft, hop, L), L))
        T, F = 1 + L // hop, n_fft // 2 + 1
        for bins, eps in C.STFT_MAG_FORMS:
            tag = ("forms", n_fft, hop, L, bins, eps)
            re, im, mag = ops.stft(x, n_fft, hop, mag_bins=bins, mag_eps=eps)
            want = R.stft(host(x), n_fft, hop)
            bad.near(tag, mag, np.sqrt(want[0] ** 2 + want[1] ** 2 + eps)[..., :bins], 2e-5, "mag max abs")
            r0, i0, m0 = ops.stft(x, n_fft, hop, want_ri=False, mag_bins=bins, mag_eps=eps)
            bad.true(tag, r0 is None and i0 is None and m0.shape == (C.B, T, bins) and same_bits(m0, mag), "mag alone differs from the full call")
            only_re = torch.full((C.B, T, F), SENTINEL, device="cuda")
            ops.stft(x, n_fft, hop, out=(only_re, None, None))
            only_im = torch.full((C.B, T, F), SENTINEL, device="cuda")
            ops.stft(x, n_fft, hop, out=(None, only_im, None))
            bad.true(tag, same_bits(only_re, re), "re without im differs from the full call")
            bad.true(tag, same_bits(only_im, im), "im without re differs from the full call")
    assert not bad, "\n".join(map(str, bad))


def test_stft_direct_dft_path(ops):
    bad = Bad()
    for n_fft, hop, L, tol in C.STFT_DFT:
        x = C.wave(C.stft_seed(n_fft, hop, L), L)
        want = R.stft(x, n_fft, hop)
        re, im, _ = ops.stft(dev(x), n_fft, hop)
        tag = ("dft", n_fft, hop, L)
        bad.true(tag, re.shape == im.shape == (C.B, 1 + L // hop, n_fft // 2 + 1), "shape")
        bad.parts(tag, (re, im), want, tol)
    assert not bad, "\n".join(map(str, bad))


def test_stft_refusals_launch_nothing(ops):
    from cruse_amd._lib import lib
    bad = Bad()
    for n_fft, hop, L, bins in C.STFT_REFUSED:
        tag = ("refused", n_fft, hop, L, bins)
        x = dev(C.wave(1, L))
        outs = [torch.full((C.B * (1 + L // max(hop, 1)) * (n_fft // 2 + 2),), SENTINEL, device="cuda") for _ in range(3)]
        rc = lib.cruse_stft_fwd(x.data_ptr(), C.B, L, n_fft, hop, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr() if bins else None,
                                bins or 0, 0.0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        bad.true(tag, rc == -1 and lib.cruse_last_error().decode().startswith("stft"), f"rc {rc}: not a shape error")
        bad.true(tag, all(bool((o == SENTINEL).all()) for o in outs), "an output was written")
        if hop > 0:
            bad.true(tag, refused(lambda: ops.stft(x, n_fft, hop, mag_bins=bins or 0), "cruse_hip error -1"), "ops.stft did not raise")
    assert not bad, "\n".join(map(str, bad))


# ---------------------------------------------------------------------------------------------------------------- cruse_istft_fwd
def test_istft_frames_hops_and_lengths(ops):
    """the longest L = hop (T - 1) + 160 ends on samples that only the last frame covers, next to its window's end: the output there is
    frame / window, 1e4 times the other samples, and as exact as the kernel's window is (0.5 - 0.5 cos in f32 gave 1.0e-5 to 1.8e-5 here)"""
    bad = Bad()
    for i, (T, hop, L) in enumerate(C.ISTFT):
        re, im = C.spectrum(100 + i, T, 161)
        want = R.istft(re, im, C.NFFT, hop, L)
        y = ops.istft(dev(re), dev(im), C.NFFT, hop, L)
        tag = ("istft", T, hop, L)
        bad.true(tag, y.shape == (C.B, L) and bool(torch.isfinite(y).all()), "shape / not finite")
        bad.close(tag, y, want, 1e-5)
        if hop == C.NFFT:
            zeros = [p - 160 for p in range(C.NFFT, 160 + L, C.NFFT)]
            bad.true(tag, bool((y[:, zeros] == 0).all()), "samples 320 t are not exactly 0")
    for T, hop in C.ISTFT_T_HOP:
        re, im = (torch.zeros(C.B, T, 161, device="cuda") for _ in range(2))
        bad.true(("istft", T, hop, "L max + 1"), refused(lambda: ops.istft(re, im, C.NFFT, hop, C.istft_max_len(T, hop) + 1), "exceeds"), "not refused")
    assert not bad, "\n".join(map(str, bad))


def test_istft_inverts_stft(ops):
    bad = Bad()
    for hop, L in C.ISTFT_ROUND_TRIPS:
        x = dev(C.wave(5, L))
        re, im, _ = ops.stft(x, C.NFFT, hop)
        bad.true((hop, L), re.shape[1] == 1 + L // hop, "T")
        bad.near(("round trip", hop, L), ops.istft(re, im, C.NFFT, hop, L), host(x), 1e-5)
    assert not bad, "\n".join(map(str, bad))


# ---------------------------------------------------------------------------------------------------------------- cruse_istft_bwd
def test_istft_bwd_is_the_adjoint(ops):
    """against the float64 transpose, and as <istft(X), d> = <X, istft_bwd(d)> on the device's own outputs.  Bar of the identity: each side is
    off its exact value by at most 1e-5 of the norms it is made of (the kernels' bar, Cauchy-Schwarz), so the two differ by at most
    1e-5 (|y| |d| + |X| |g|)."""
    bad = Bad()
    for i, (T, hop, L) in enumerate(C.ISTFT):
        re, im = C.spectrum(100 + i, T, 161)
        d = C._f32(np.random.default_rng(200 + i).standard_normal((C.B, L)))
        want = R.istft_adjoint(d, T, C.NFFT, hop)
        dre, dim = ops.istft_bwd(dev(d), T, C.NFFT, hop)
        tag = ("istft_bwd", T, hop, L)
        bad.true(tag, dre.shape == dim.shape == (C.B, T, 161), "shape")
        bad.true(tag, bool(torch.isfinite(dre).all()) and bool(torch.isfinite(dim).all()), "not finite")
        bad.true(tag, bool((dim[..., 0] == 0).all()) and bool((dim[..., 160] == 0).all()), "dim of bins 0 / 160 is not exactly 0")
        bad.parts(tag, (dre, dim), want, 1e-5)
        y = host(ops.istft(dev(re), dev(im), C.NFFT, hop, L))
        im0 = im.copy()
        im0[..., 0] = 0.0
        im0[..., 160] = 0.0
        gr, gi = host(dre), host(dim)
        lhs, rhs = float(np.sum(y * d)), float(np.sum(re * gr) + np.sum(im0 * gi))
        bound = 1e-5 * (np.linalg.norm(y) * np.linalg.norm(d) + np.sqrt(np.sum(re ** 2) + np.sum(im0 ** 2)) * np.sqrt(np.sum(gr ** 2) + np.sum(gi ** 2)))
        print(f"{tag} <istft(X), d> {lhs:.9e}  <X, bwd(d)> {rhs:.9e}  bound {bound:.3e}")
        bad.true(tag, abs(lhs - rhs) <= bound, f"adjoint identity: {lhs} vs {rhs}, bound {bound}")
    for T, hop in C.ISTFT_T_HOP:
        d = torch.zeros(C.B, C.istft_max_len(T, hop) + 1, device="cuda")
        bad.true(("istft_bwd", T, hop, "L max + 1"), refused(lambda: ops.istft_bwd(d, T, C.NFFT, hop), "exceeds"), "not refused")
    assert not bad, "\n".join(map(str, bad))


# ---------------------------------------------------------------------------------------------------------------- cruse_stft_framed / cruse_istft_framed
def _framed_inputs(case):
    n_fft, win_len, win_off, hop, pad, mode, L, _ = case
    T, seed = C.framed_T(case), C.framed_seed(case)
    return T, seed, C.window(seed, win_len), C.wave(seed + 1, L), C.spectrum(seed + 2, T, n_fft // 2 + 1)


def test_framed_forward(feature):
    bad = Bad()
    for case in C.FRAMED:
        n_fft, win_len, win_off, hop, pad, mode, L, frames = case
        T, seed, w, x, _ = _framed_inputs(case)
        unit = R.stft_framed(x, w, n_fft, hop, win_off, pad, mode, T, 1.0)
        for scale in C.FRAMED_SCALES:
            want = (scale * unit[0], scale * unit[1])                                  # the formula is linear in scale
            re, im = feature.stft_framed(dev(x), dev(w), n_fft, hop, win_off=win_off, pad=pad, pad_mode=mode, frames=frames, scale=scale)
            tag, tol = ("framed", case, scale), C.framed_fwd_tol(case)
            bad.true(tag, re.shape == im.shape == (C.B, T, n_fft // 2 + 1), "shape")
            bad.parts(tag, (re, im), want, tol)
    assert not bad, "\n".join(map(str, bad))


def test_framed_inverse(feature):
    """three output lengths around the frames' span: one short of it, the span, and 70 more -- that tail is exactly 0 (the zero fill ran)"""
    bad = Bad()
    for case in C.FRAMED:
        n_fft, win_len, win_off, hop, pad, mode, L, _ = case
        T, seed, w, _, (Yr, Yi) = _framed_inputs(case)
        span = C.framed_span(case)
        for herm in (False, True):
            # output sample m does not depend on the length, and the formula is linear in scale and post: one reference per form
            unit = R.istft_framed(Yr, Yi, w, None, n_fft, hop, win_off, pad, span + 70, 1.0, herm)
            for scale in C.FRAMED_SCALES:
                for Lo in (span - 1, span, span + 70):
                    for post in (None, C.positive(seed + 3, Lo)):
                        want = scale * unit[:, :Lo] * (1.0 if post is None else post)
                        y = feature.istft_framed(dev(Yr), dev(Yi), dev(w), n_fft, hop, win_off=win_off, pad=pad, length=Lo, scale=scale,
                                                 hermitian=herm, post_full=None if post is None else dev(post))
                        tag = ("framed inverse", case, herm, scale, Lo, post is not None)
                        bad.true(tag, y.shape == (C.B, Lo), "shape")
                        bad.close(tag, y, want, C.framed_inv_tol(case))
                        if Lo > span:
                            bad.true(tag, bool((y[:, span:] == 0).all()), "the tail past the frames is not exactly 0")
    assert not bad, "\n".join(map(str, bad))


def test_framed_autograd_is_the_adjoint_pair(feature):
    bad = Bad()
    for case in C.FRAMED:
        n_fft, win_len, win_off, hop, pad, mode, L, frames = case
        T, seed, w, x, (Yr, Yi) = _framed_inputs(case)
        d = C._f32(np.random.default_rng(seed + 4).standard_normal((C.B, L)))
        reflecting = mode == "reflect" and pad > 0
        for scale in C.FRAMED_SCALES:
            tag = ("framed autograd", case, scale)
            xg = dev(x).requires_grad_(True)
            re, im = feature.stft_framed(xg, dev(w), n_fft, hop, win_off=win_off, pad=pad, pad_mode=mode, frames=frames, scale=scale)
            loss = (re * dev(Yr)).sum() + (im * dev(Yi)).sum()
            if reflecting:
                bad.true(tag, refused(loss.backward, "reflect padding"), "a gradient through reflect padding was not refused")
            else:
                loss.backward()
                bad.close(tag, xg.grad, R.istft_framed(Yr, Yi, w, None, n_fft, hop, win_off, pad, L, scale, False), C.framed_inv_tol(case), "d/dwave")
            rg, ig = dev(Yr).requires_grad_(True), dev(Yi).requires_grad_(True)
            y = feature.istft_framed(rg, ig, dev(w), n_fft, hop, win_off=win_off, pad=pad, length=L, scale=scale)
            (y * dev(d)).sum().backward()
            bad.close(tag, (rg.grad, ig.grad), R.stft_framed(d, w, n_fft, hop, win_off, pad, "zeros", T, scale), C.framed_fwd_tol(case), "d/d(re, im)")
        for kw in ({"hermitian": True}, {"post_full": dev(C.positive(seed + 3, L))}):
            rg = dev(Yr).requires_grad_(True)
            bad.true(("framed autograd", case, tuple(kw)),
                     refused(lambda: feature.istft_framed(rg, dev(Yi), dev(w), n_fft, hop, win_off=win_off, pad=pad, length=L, **kw), "plain adjoint form"),
                     "a gradient in the hermitian / post form was not refused")
    assert not bad, "\n".join(map(str, bad))
