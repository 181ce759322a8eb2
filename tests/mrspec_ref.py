"""The multi-resolution spectral loss of DESIGN section 20 restated on torch-CPU: what cruse_mrspec_loss computes, in the precision of the
waveforms handed in (float64 for the tests' reference, float32 to measure what f32 arithmetic alone costs).

    loss = sum_r factor * mean (a - s)^2 + f_complex[r] * mean |Yc - Sc|^2
    Y = STFT_N(est), S = STFT_N(ref): torch.stft(n_fft = N, hop = N / 4, periodic Hann, center = True (reflect), normalized = True)
    gamma != 1:  a = max(|Y|, 1e-12)^gamma, Yc = a e^{i arg Y}  (likewise s, Sc);   gamma == 1:  a = |Y|, Yc = Y

The gradient is torch autograd's, with the phase taken by `Angle`, whose backward divides by max(|x|^2, 1e-10)."""
from __future__ import annotations

from collections.abc import Iterable

import torch


class Angle(torch.autograd.Function):
    """atan2(imag, real); backward: grad / max(|x|^2, 1e-10) * (-imag, real)"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.atan2(x.imag, x.real)

    @staticmethod
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        g = grad / (x.real.square() + x.imag.square()).clamp_min(1e-10)
        return torch.view_as_complex(torch.stack((-x.imag * g, x.real * g), dim=-1))


def complex_weights(f_complex, R):
    """None (no complex term) or the R per-resolution weights, as the reference's constructor reads its argument"""
    if f_complex is None or (not isinstance(f_complex, Iterable) and f_complex == 0):
        return None
    if isinstance(f_complex, Iterable):
        w = [float(v) for v in f_complex]
        if len(w) != R:
            raise ValueError(f"f_complex has {len(w)} values for {R} resolutions")
        return w
    return [float(f_complex)] * R


def stft(x, n_fft):
    w = torch.hann_window(n_fft, dtype=x.dtype, device=x.device)
    return torch.stft(x, n_fft=n_fft, hop_length=n_fft // 4, window=w, normalized=True, return_complex=True)


def mrspec_loss(est, ref, n_ffts, gamma=0.3, factor=1.0, f_complex=None):
    """est, ref [B,L] (one dtype, one device) -> the scalar loss, differentiable wrt est"""
    fc = complex_weights(f_complex, len(n_ffts))
    loss = torch.zeros((), dtype=est.dtype, device=est.device)
    for i, n in enumerate(n_ffts):
        Y, S = stft(est, n), stft(ref, n)
        Ya, Sa = Y.abs(), S.abs()
        if gamma != 1:
            Ya = Ya.clamp_min(1e-12).pow(gamma)
            Sa = Sa.clamp_min(1e-12).pow(gamma)
        loss = loss + torch.nn.functional.mse_loss(Ya, Sa) * factor
        if fc is not None:
            if gamma != 1:
                Y = Ya * torch.exp(1j * Angle.apply(Y))
                S = Sa * torch.exp(1j * Angle.apply(S))
            loss = loss + torch.nn.functional.mse_loss(torch.view_as_real(Y), torch.view_as_real(S)) * fc[i]
    return loss


def mrspec_loss_and_grad(est, ref, n_ffts, gamma=0.3, factor=1.0, f_complex=None, dtype=torch.float64):
    """-> (loss, d loss / d est) as tensors of `dtype`, computed in `dtype` on the CPU"""
    x = est.detach().cpu().to(dtype).clone().requires_grad_(True)
    s = ref.detach().cpu().to(dtype)
    loss = mrspec_loss(x, s, n_ffts, gamma, factor, f_complex)
    loss.backward()
    return loss.detach(), x.grad.detach()


def make_pair(B, L, seed):
    """the tests' inputs: ref = 0.1 randn, est = ref + 0.05 randn, drawn in f64 and cast to f32"""
    g = torch.Generator().manual_seed(seed)
    ref = 0.1 * torch.randn(B, L, generator=g, dtype=torch.float64)
    est = ref + 0.05 * torch.randn(B, L, generator=g, dtype=torch.float64)
    return est.float(), ref.float()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())
