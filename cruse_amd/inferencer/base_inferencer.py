"""Inference on the HIP path: noisy waveform -> magnitude -> unet_2 mask -> mask on the noisy spectrum (== enhanced
magnitude with the noisy phase) -> iSTFT, with the reference's RTF report and int16 scaling.

Mirrors train_base/inferencer/base_inferencer.py: `multi_channel_mag_to_mag` (:138-161: |STFT| -> model ->
enhanced_mag * (cos, sin)(noisy phase) -> istft(length=noisy.shape[-1])) and `__call__` (:163-200: batch size 1,
rtf = elapsed / (len / sr), 0.8 * int16 peak scaling).  CRUSE's unet_2 returns a sigmoid MASK on the first
`in_feat // 2 * 2` bins (model/cruse_net.py:164), so the enhanced magnitude is mask * |noisy| and
mag * cos(phase) == mask * real: the phase is never formed (PreProcess.masking, utils/utils.py:418-420).

head="df" is for a model trained with the DeepFilter loss (BASELINE config 4, TrainEngine(loss="wo_male_df")): its output is the real
part of a DeepFilter(t_dim, f_dim) filter field, and the enhanced spectrum is the neighbourhood sum of mask * N
(loss.deepfilter_spectrum, one kernel) instead of mask * N itself.

post_filter="iam" / "envelope" applies the reference's perceptual post-filter (utils/utils.py:345-362, ops.post_filter, one pointwise
kernel) to the mask before it meets the spectrum; None (the default) launches nothing new.
"""
from __future__ import annotations

import time
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from ..acoustics import feature
from ..loss import deepfilter_spectrum, enhanced_spectrum

HEADS = ("mask", "df")


class Inferencer:
    def __init__(self, model: torch.nn.Module, n_fft: int = 320, hop_length: int = 160, win_length: int = 320,
                 sr: int = 16000, device="cuda", atten_lim_db=None, head: str = "mask", df_dims=(1, 5), post_filter=None,
                 pf_tau: float = 0.02):
        from .. import ops
        if head not in HEADS:
            raise ValueError(f"Inferencer: head = {head!r}, expected one of {HEADS}")
        if post_filter is not None:
            ops.post_filter_kind(post_filter)
            if head == "df":
                raise ValueError("Inferencer(head=\"df\") takes no post_filter: the model's output is a filter field, not a gain")
        self.post_filter, self.pf_tau = post_filter, ops.post_filter_tau(pf_tau)
        t_dim, f_dim = (int(d) for d in df_dims)
        if not (0 <= t_dim <= 8 and 0 <= f_dim <= 16):
            raise ValueError(f"Inferencer: df_dims = {tuple(df_dims)!r}, expected (t_dim in 0..8, f_dim in 0..16)")
        self.head, self.df_dims = head, (t_dim, f_dim)
        self.lim = ops.atten_lim_gain(atten_lim_db)       # DeepFilterNet's atten_lim_db as a gain; 0: no limit (the default)
        self.model = model.to(device).eval()
        self.n_fft, self.hop, self.win, self.sr = n_fft, hop_length, win_length, sr
        self.device = torch.device(device)
        self.f_net = (n_fft // 2 + 1) // 2 * 2            # unet_2 runs on in_feat // 2 * 2 bins

    @torch.no_grad()
    def mag_mask_to_wave(self, noisy: torch.Tensor) -> torch.Tensor:
        """noisy [B,L] (device) -> enhanced [B,L] (device); with atten_lim_db: lim * noisy + (1 - lim) * enhanced, lim = 10^(-dB/20)."""
        if noisy.dim() != 2:
            raise RuntimeError(f"Inferencer expects [B,L] waveforms, got {tuple(noisy.shape)}")
        spec = feature.pre_stft(noisy, self.n_fft, self.hop, self.win, f_net=self.f_net)
        mask = self.model(spec["mag_net"])                                   # [B,1,T,f_net]
        if self.head == "df":
            est = deepfilter_spectrum(mask, spec["real"].squeeze(1), spec["imag"].squeeze(1), *self.df_dims)
        else:
            if self.post_filter is not None:
                from .. import ops
                mask = ops.post_filter(mask.contiguous(), self.pf_tau, self.post_filter)
            est = enhanced_spectrum(mask, spec["real"].squeeze(1), spec["imag"].squeeze(1))   # [B,T,F,2]
        wave = feature.istft_ri(est[..., 0], est[..., 1], self.n_fft, self.hop, length=noisy.shape[-1])
        if self.lim == 0.0:
            return wave
        return self.lim * noisy + (1.0 - self.lim) * wave

    @staticmethod
    def to_int16(enhanced: np.ndarray) -> np.ndarray:
        amp = np.iinfo(np.int16).max                                          # base_inferencer.py:183-185
        return np.int16(0.8 * amp * enhanced / np.max(np.abs(enhanced)))

    @torch.no_grad()
    def __call__(self, dataloader: Iterable[Tuple[torch.Tensor, list]], sink=None, log=print):
        """dataloader yields (noisy [1,L], [name]); returns [(name, rtf)], hands (name, int16 waveform) to sink."""
        out = []
        for noisy, name in dataloader:
            assert len(name) == 1, "The batch size of inference stage must 1."      # base_inferencer.py:173
            name = name[0]
            noisy = noisy.to(self.device)
            torch.cuda.synchronize()
            t1 = time.time()
            enhanced = self.mag_mask_to_wave(noisy).squeeze(0)
            torch.cuda.synchronize()
            t2 = time.time()
            enhanced = enhanced.cpu().numpy()
            if (np.abs(enhanced) > 1).any():
                log(f"Warning: enhanced is not in the range [-1, 1], {name}")
            wav = self.to_int16(enhanced)
            rtf = (t2 - t1) / (len(wav) * 1.0 / self.sr)                       # base_inferencer.py:187-190
            log(f"{name}, rtf: {rtf}")
            if sink is not None:
                sink(name, wav)
            out.append((name, rtf))
        return out
