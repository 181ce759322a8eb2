"""Test-only: a frame-by-frame restatement of the DeepFilter(1, 5) head on the stream (cruse_stream_df_head, csrc/stream.hip), and the
offline waveform it has to reproduce.

df_stream() is driven by the per-frame rows of tests/stream_ref.stream_clip (mask, re, im of frames 0..nb) and keeps what the kernel
keeps per slot: the product rows P[t-2], P[t-1], the noisy row N[t-1], an overlap-add tail of its own and the count of rows taken.  A step
takes row t and emits E[t-1]; frame 0 starts from a zero history and emits nothing; E[0]'s block lies in front of the clip; a drain step
on an all-zero row emits E[T-1].  float64 by default (any dtype the rows have).

offline_df() is the oracle's offline path of the same model: pre_stft -> unet_2 -> zero-padded mask -> oracle DeepFilter(1, 5) -> istft.
In float64 the STFT pair is torch.stft / torch.istft with a float64 periodic Hann window (the oracle's own helpers build the window in
float32 whatever the input: its float64 results carry that window's 6e-8 rounding)."""
from __future__ import annotations

import torch

from oracle import cruse_oracle as O

HOP, NFFT, NB, F0 = 160, 320, 161, 160
T_DIM, F_DIM = 1, 5


def product_row(fr: dict) -> torch.Tensor:
    """P[t] [2, 161] of a frame's rows: mask * N on bins 0..159, bin 160 zero"""
    z = torch.zeros(1, dtype=fr["re"].dtype)
    return torch.stack([torch.cat([fr["mask"] * fr["re"][:F0], z]), torch.cat([fr["mask"] * fr["im"][:F0], z])])


def window_sum(p2: torch.Tensor, p1: torch.Tensor, pc: torch.Tensor) -> torch.Tensor:
    """E[t-1] [2, 161] = sum over the three rows and bins f-5..f+5, zero outside the spectrum"""
    rows = torch.nn.functional.pad(p2 + p1 + pc, (F_DIM, F_DIM))
    return sum(rows[:, d:d + NB] for d in range(2 * F_DIM + 1))


def df_stream(frames, lim: float = 0.0):
    """frames: the rows of frames 0..nb (dicts with mask [160], re, im [161]) -> (wave [nb * 160], E [nb + 1, 2, 161])"""
    dtype = frames[0]["re"].dtype
    win = torch.hann_window(NFFT, dtype=dtype)
    env = win[:HOP] ** 2 + win[HOP:] ** 2
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    p2, p1, n1, tail, cnt = z(2, NB), z(2, NB), z(2, NB), z(HOP), 0
    blocks, rows = [], []
    for t, fr in enumerate(list(frames) + [None]):          # None: the drain step
        if t == 0:                                          # frame 0 of the clip: zero history, nothing emitted
            p2, p1, n1, tail, cnt = z(2, NB), z(2, NB), z(2, NB), z(HOP), 0
        pc = z(2, NB) if fr is None else product_row(fr)
        nc = z(2, NB) if fr is None else torch.stack([fr["re"], fr["im"]])
        if cnt >= 1:
            e = window_sum(p2, p1, pc)
            rows.append(e)
            sp = lim * n1 + (1.0 - lim) * e
            y = torch.fft.irfft(torch.complex(sp[0], sp[1]), n=NFFT) * win
            if cnt >= 2:                                    # E[0]'s block lies in front of the clip
                blocks.append((tail + y[:HOP]) / env)
            tail = y[HOP:].clone()
        p2, p1, n1, cnt = p1, pc, nc, min(cnt + 1, 2)
    return torch.cat(blocks), torch.stack(rows)


@torch.no_grad()
def offline_df(model, x: torch.Tensor, head: str = "df") -> torch.Tensor:
    """x [L] -> the oracle's offline waveform [L] of `model` (an oracle unet_2 in x's dtype) with the DeepFilter(1, 5) head, or
    (head="mask") with the magnitude mask of the same model"""
    dtype = x.dtype
    if dtype == torch.float32:
        f = O.pre_stft(x.view(1, -1), NFFT, HOP, NFFT, f_net=F0)
        re, im, mag = f["real"], f["imag"], f["mag_net"]
        inv = lambda c: O.istft(c, NFFT, HOP, NFFT, length=x.numel())
    else:                                                   # the same transform pair with the window in x's dtype
        win = torch.hann_window(NFFT, dtype=dtype)
        spec = torch.stft(x.view(1, -1), NFFT, HOP, NFFT, window=win, return_complex=True, center=True)      # [1,F,T]
        ri = torch.view_as_real(spec).permute(0, 3, 2, 1)
        re, im = ri[:, 0:1].contiguous(), ri[:, 1:2].contiguous()
        mag = torch.sqrt(re ** 2 + im ** 2 + 1e-8)[..., :F0]
        inv = lambda c: torch.istft(c, NFFT, HOP, NFFT, window=win, length=x.numel(), center=True)
    mask = model(mag)
    h_r = torch.nn.functional.pad(mask, (0, NB - F0)).squeeze(1).transpose(1, 2)                              # [1,F,T]
    x_r, x_i = re.squeeze(1).transpose(1, 2), im.squeeze(1).transpose(1, 2)
    if head == "mask":
        return inv(torch.complex(x_r * h_r, x_i * h_r)).view(-1)
    y = O.DeepFilter(T_DIM, F_DIM).to(dtype)([x_r, x_i], [h_r, torch.zeros_like(h_r)])
    return inv(torch.complex(y[:, :NB], y[:, NB:])).view(-1)
