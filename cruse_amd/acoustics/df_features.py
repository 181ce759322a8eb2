"""DeepFilterNet's two normalised input features on one HIP kernel (ops.df_feat / cruse_df_feat).

The reference keeps these in test/ scripts, so there is no reference import path to mirror:
  - get_norm_alpha / _calculate_norm_alpha: test/test_norm.py:12-30, the rounding loop integer for integer
  - ExponentialUnitNorm: test/test_norm.py:33-61, its constructor, its buffer `init_state` and its forward line for line
  - the ERB feature: band_mean_norm_erb, test/test_erb.py:97-106, with ONE REPAIR: the reference starts `out_xs` from zeros instead of
    from `xs` and so returns -state / 40; here out = (x - state) / 40.  (band_unit_norm's `norm(x) * (1 - alpha + s * alpha)`,
    test_erb.py:116, is a misplaced parenthesis; ExponentialUnitNorm is the definition of the unit norm.)
The reference contains neither the log-power front end of the ERB feature nor the initial state of its mean.  Both are DeepFilterNet's
published ones: 10 log10(mean band power + 1e-10), and linspace(-60, -90, nb_erb) (ops.DF_ERB_INIT).

Both features are first-order recurrences along time.  The kernel takes the state in and hands it back, and any split of the frames
over calls gives the bits of one call: a frame-by-frame caller gets the offline features.  Inference only (no backward kernel): the
features are computed from the noisy input, which carries no gradient in DeepFilterNet.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .. import ops

TC = ops.DF_FEAT_TC          # the kernel's frame tile


def _calculate_norm_alpha(sr: int, hop_size: int, tau: float):
    """test/test_norm.py:28-30"""
    dt = hop_size / sr
    return math.exp(-dt / tau)


def get_norm_alpha(sr: int = 48000, hop_size: int = 480, tau: float = 1, log: bool = True):
    """test/test_norm.py:12-25: exp(-hop / (sr tau)) rounded to 3 decimals, to more while the rounding gives 1"""
    a_ = _calculate_norm_alpha(sr=sr, hop_size=hop_size, tau=tau)
    precision = 3
    a = 1.0
    while a >= 1.0:
        a = round(a_, precision)
        precision += 1
    if log:
        print(f"Running with normalization window alpha = '{a}'")
    return a


class ExponentialUnitNorm(nn.Module):
    """test/test_norm.py:33-61.  forward(x [b,c,t,f,2]) = x / sqrt(s), s[t] = |x[t]| (1 - alpha) + alpha s[t-1], |x| = sqrt(max(re^2 + im^2,
    eps)), with (b, c) as the kernel's batch and the interleaved x read in place.  Every call starts from `init_state` as the reference
    does, unless `state` [b,c,f] is given: it is the state before the first frame and is overwritten with the state after the last."""

    def __init__(self, alpha: float, num_freq_bins: int, eps: float = 1e-14):
        super().__init__()
        self.alpha = alpha
        self.eps = eps
        self.UNIT_NORN_INIT = list(ops.DF_UNIT_INIT)
        s = torch.linspace(self.UNIT_NORN_INIT[0], self.UNIT_NORN_INIT[1], num_freq_bins).unsqueeze(0)
        self.register_buffer("init_state", s.view(1, 1, num_freq_bins, 1))

    def forward(self, x: Tensor, state: Optional[Tensor] = None) -> Tensor:
        if x.dim() != 5 or x.shape[-1] != 2 or x.shape[3] != self.init_state.shape[2]:
            raise RuntimeError(f"ExponentialUnitNorm: expected [b,c,t,{self.init_state.shape[2]},2], got {tuple(x.shape)}")
        b, c, t, f, _ = x.shape
        x = x.contiguous()
        if state is None:
            st = self.init_state.view(1, f).to(x.device).repeat(b * c, 1)
        else:
            if tuple(state.shape) != (b, c, f) or not state.is_contiguous():
                raise RuntimeError(f"ExponentialUnitNorm: state must be contiguous [{b}, {c}, {f}], got {tuple(state.shape)}")
            st = state.view(b * c, f)
        xv = x.view(b * c, t, f, 2)
        _, y = ops.df_feat(xv[..., 0], xv[..., 1], None, f, self.alpha, unit_state=st, unit_eps=self.eps)
        return y.view(b, c, t, f, 2)


class DfFeatures(nn.Module):
    """The two features a DeepFilterNet reads, from a spectrum: feat_erb [B,1,T,nb_erb] = (e - mean) / 40 with e the log power of nb_erb
    ERB bands (widths: erb_fb(sr, fft_size, nb_erb, min_nb_freqs)) and feat_spec [B,1,T,nb_df,2] = the lowest nb_df bins under the
    exponential unit norm; alpha = get_norm_alpha(sr, hop_size, tau)."""

    def __init__(self, sr: int = 16000, fft_size: int = 320, hop_size: int = 160, nb_erb: int = 32, nb_df: int = 96, min_nb_freqs: int = 2,
                 tau: float = 1.0):
        super().__init__()
        from ..model.based_model.cust_conv import erb_fb
        self.sr, self.fft_size, self.hop_size, self.nb_erb, self.nb_df = int(sr), int(fft_size), int(hop_size), int(nb_erb), int(nb_df)
        self.freq_bins = self.fft_size // 2 + 1
        if not 1 <= self.nb_df <= self.freq_bins:
            raise ValueError(f"DfFeatures: nb_df = {nb_df} outside 1..{self.freq_bins}")
        self.widths = [int(w) for w in erb_fb(sr, fft_size, nb_erb, min_nb_freqs).tolist()]
        self.alpha = get_norm_alpha(sr=sr, hop_size=hop_size, tau=tau, log=False)

    def init_state(self, B: int, device) -> Tuple[Tensor, Tensor]:
        """(erb_state [B, nb_erb] = linspace(-60, -90), unit_state [B, nb_df] = linspace(0.001, 0.0001)) on `device`"""
        return ops.df_feat_states(B, self.nb_erb, self.nb_df, device)

    def forward(self, re: Tensor, im: Tensor, state: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
        """re, im [B,T,F] (ops.stft's planes, or the views of an interleaved tensor).  state = init_state(...)'s pair: updated in place;
        absent, the call starts from the defaults."""
        from ..model.based_model.cust_conv import _band_table
        starts, F = _band_table(self.widths, re.device)
        if re.dim() != 3 or re.shape[-1] != F:
            raise RuntimeError(f"DfFeatures: expected a [B,T,{F}] spectrum, got {tuple(re.shape)}")
        es, us = state if state is not None else (None, None)
        fe, fs = ops.df_feat(re, im, starts, self.nb_df, self.alpha, erb_state=es, unit_state=us)
        return fe.unsqueeze(1), fs.unsqueeze(1)

    def from_wave(self, wave: Tensor, state: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
        """wave [B,L] -> forward(*ops.stft(wave, fft_size, hop_size)).  `state` covers the features only: the STFT frames each call's
        waveform on its own, so framing across calls (overlap, padding) is the caller's."""
        re, im, _ = ops.stft(wave, self.fft_size, self.hop_size)
        return self.forward(re, im, state)
