"""Test-only: the per-frame torch-CPU restatement of streaming inference for CRUSE4MagAddSkipUpsample (n_fft = win = 320, hop = 160).

tests/stream_ref.py for the model with the upsample decoder: runs the children of oracle.cruse_oracle_ext.CRUSE4MagAddSkipUpsample
(eval mode) one frame at a time with the state the streaming kernels keep -- the previous input row of each encoder level, one h per GRU,
the analysis history and the overlap-add tail.  The encoder blocks are Conv2dNormAct (ConstantPad2d of one row on top, Conv2d (2,3),
BatchNorm, ReLU): a frame feeds rows t-1 and t to the conv itself, which is the padding's effect at t = 0 (the state starts at zero).
The decoder blocks (FreqUpsample, Conv2d (1,3), BatchNorm, act) have time extent 1 and run as they are on a one-row input.

dtype: float32 (default) or float64 (pass stream_ref.as_double(model)).  polyphase_upconv is the decoder level's arithmetic in the form
the kernel's header states, for the identity test of tests/test_stream_up_host.py.
"""
from __future__ import annotations

import torch

from tests.stream_ref import HOP, NFFT, as_double, frame_of, nontrivial_bn  # noqa: F401  (re-exported for the tests)


@torch.no_grad()
def frame_step(model, fr: torch.Tensor, st: dict, dtype=torch.float32) -> dict:
    """one frame through the model with streaming state st (updated in place); returns the frame's intermediates"""
    win = torch.hann_window(NFFT, dtype=dtype)
    fr = fr.to(dtype)
    spec = torch.fft.rfft(fr * win)
    re, im = spec.real.contiguous(), spec.imag.contiguous()
    mag = torch.sqrt(re ** 2 + im ** 2 + 1e-8)[:160].view(1, 1, 1, 160)
    out = {"re": re, "im": im}
    cur = mag
    for k in range(1, 5):
        enc = getattr(model, f"enc{k}")                                      # 0: pad, 1: conv, 2: BatchNorm, 3: ReLU
        inp = torch.cat([st["prev"][k - 1], cur], dim=2)                     # rows t-1, t
        st["prev"][k - 1] = cur
        cur = enc[3](enc[2](enc[1](inp)))
        out[f"e{k}"] = cur
        out[f"skip{k}"] = getattr(model, f"skip_connect_{k}")(cur)
    gru = model.gru
    g = gru.groups
    row = cur.transpose(1, 2).reshape(1, 1, -1)                              # [1,1,C4*F4]
    xs = torch.chunk(row, g, dim=-1)
    o1 = []
    for i in range(g):
        y, h = gru.gru_list1[i](xs[i], st["h1"][i])
        st["h1"][i] = h
        o1.append(y)
    out["gru1"] = torch.cat(o1, dim=-1).reshape(-1)                          # group-contiguous
    v = gru.ln1(torch.flatten(torch.stack(o1, dim=-1), start_dim=-2))
    xs = torch.chunk(v, g, dim=-1)
    o2 = []
    for i in range(g):
        y, h = gru.gru_list2[i](xs[i], st["h2"][i])
        st["h2"][i] = h
        o2.append(y)
    out["gru2"] = torch.cat(o2, dim=-1).reshape(-1)
    d = gru.ln2(torch.cat(o2, dim=-1)).view(1, 1, cur.shape[1], -1).transpose(1, 2) + out["skip4"]
    out["dec_in"] = d
    for k in range(4, 1, -1):
        d = getattr(model, f"dec{k}")(d) + out[f"skip{k - 1}"]
        out[f"d{k}"] = d
    mask = model.dec1(d).reshape(-1)
    out["mask"] = mask
    er = torch.cat([mask * re[:160], torch.zeros(1, dtype=dtype)])
    ei = torch.cat([mask * im[:160], torch.zeros(1, dtype=dtype)])
    y = torch.fft.irfft(torch.complex(er, ei), n=NFFT) * win
    env = win[:HOP] ** 2 + win[HOP:] ** 2
    out["block"] = (st["tail"] + y[:HOP]) / env                             # output block t-1
    st["tail"] = y[HOP:].clone()
    return out


def channels(model):
    return [model.enc1[1].in_channels] + [getattr(model, f"enc{k}")[1].out_channels for k in range(1, 5)]


def new_state(model, dtype=torch.float32) -> dict:
    ch, g = channels(model), model.gru.groups
    Hg = model.gru.gru_list1[0].hidden_size
    z = lambda *shape: torch.zeros(*shape, dtype=dtype)
    return {"prev": [z(1, ch[k], 1, 160 >> k) for k in range(4)], "h1": [z(1, 1, Hg) for _ in range(g)],
            "h2": [z(1, 1, Hg) for _ in range(g)], "tail": z(HOP)}


@torch.no_grad()
def stream_clip(model, x: torch.Tensor, dtype=torch.float32):
    """x [L] (L a multiple of 160, >= 320) -> (enhanced [L], [intermediates of frames 0..L/160]), both in `dtype`"""
    model.eval()
    if model.enc1[1].weight.dtype != dtype:
        raise ValueError(f"stream_clip: the module's weights are {model.enc1[1].weight.dtype}, dtype is {dtype} (see as_double)")
    x = x.to(dtype)
    nb = x.numel() // HOP
    st = new_state(model, dtype)
    frames, blocks = [], []
    for t in range(nb + 1):
        o = frame_step(model, frame_of(x, t), st, dtype)
        frames.append(o)
        if t >= 1:
            blocks.append(o["block"])
    return torch.cat(blocks), frames


def polyphase_upconv(x: torch.Tensor, W: torch.Tensor, b) -> torch.Tensor:
    """x [Cin, Fin], W [Cout, Cin, 3], b [Cout] or None -> [Cout, 2*Fin]: nearest x2 upsampling + Conv2d (1,3), padding (0,1), written
    out as the two phases: out[2j] = W0 in[j-1] + (W1 + W2) in[j], out[2j+1] = (W0 + W1) in[j] + W2 in[j+1], the terms past either edge
    absent."""
    Cout, Cin, _ = W.shape
    Fin = x.shape[1]
    out = torch.zeros(Cout, 2 * Fin, dtype=x.dtype)
    for j in range(Fin):
        even = (W[:, :, 1] + W[:, :, 2]) @ x[:, j]
        if j >= 1:
            even = even + W[:, :, 0] @ x[:, j - 1]
        odd = (W[:, :, 0] + W[:, :, 1]) @ x[:, j]
        if j + 1 < Fin:
            odd = odd + W[:, :, 2] @ x[:, j + 1]
        out[:, 2 * j], out[:, 2 * j + 1] = even, odd
    return out if b is None else out + b.view(-1, 1)
