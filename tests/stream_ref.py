"""Test-only: a per-frame torch-CPU restatement of streaming unet_2 inference (n_fft = win = 320, hop = 160).

Runs the oracle's modules (oracle.cruse_oracle.unet_2, eval mode) one frame at a time with the state the streaming kernels keep:
the previous input row of each encoder level, one h per GRU, the analysis history and the overlap-add tail.  Frame t covers
x[160t-160 .. 160t+159] of the reflect-padded clip: frame 0's first half is x[160], ..., x[1], the end frame's second half
x[L-2], ..., x[L-161].  Returns the L output samples and every frame's intermediates.

dtype: float32 (default) or float64.  For float64 pass a `.double()` copy of the module (as_double): the window, the state and
all arithmetic are then float64, the reference the f32 kernels are measured against at new shapes.
"""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F

HOP, NFFT = 160, 320


def frame_of(x: torch.Tensor, t: int) -> torch.Tensor:
    """the 320 samples of frame t of the 1-D clip x (len a multiple of 160), reflect-padded as torch.stft(center=True)"""
    L = x.numel()
    nb = L // HOP
    if t == 0:
        return torch.cat([x[1:HOP + 1].flip(0), x[:HOP]])
    if t == nb:
        return torch.cat([x[L - HOP:], x[L - HOP - 1:L - 1].flip(0)])
    return x[HOP * (t - 1):HOP * (t + 1)]


@torch.no_grad()
def frame_step(model, fr: torch.Tensor, st: dict, dtype=torch.float32) -> dict:
    """one frame through unet_2 with streaming state st (updated in place); returns the frame's intermediates"""
    win = torch.hann_window(NFFT, dtype=dtype)
    fr = fr.to(dtype)
    spec = torch.fft.rfft(fr * win)
    re, im = spec.real.contiguous(), spec.imag.contiguous()
    mag = torch.sqrt(re ** 2 + im ** 2 + 1e-8)[:160].view(1, 1, 1, 160)
    out = {"re": re, "im": im}
    cur = mag
    for k in range(1, 5):
        conv, bn = getattr(model, f"conv{k}"), getattr(model, f"bn{k}")
        inp = torch.cat([st["prev"][k - 1], cur], dim=2)                     # rows t-1, t
        st["prev"][k - 1] = cur
        cur = torch.relu(bn(F.conv2d(inp, conv.weight, conv.bias, stride=(1, 2), padding=(0, 1))))
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
    for k in range(4, 1, -1):
        d = torch.relu(getattr(model, f"bn{k}_t")(getattr(model, f"conv{k}_t")(d)[..., :-1])) + out[f"skip{k - 1}"]
    mask = torch.sigmoid(model.conv1_t(d)[..., :-1]).reshape(-1)
    out["mask"] = mask
    er = torch.cat([mask * re[:160], torch.zeros(1, dtype=dtype)])
    ei = torch.cat([mask * im[:160], torch.zeros(1, dtype=dtype)])
    y = torch.fft.irfft(torch.complex(er, ei), n=NFFT) * win
    env = win[:HOP] ** 2 + win[HOP:] ** 2
    out["block"] = (st["tail"] + y[:HOP]) / env                             # output block t-1
    st["tail"] = y[HOP:].clone()
    return out


def new_state(model, dtype=torch.float32) -> dict:
    ch, g = [model.conv1.in_channels] + [getattr(model, f"conv{k}").out_channels for k in range(1, 5)], model.gru.groups
    Hg = model.gru.gru_list1[0].hidden_size
    z = lambda *shape: torch.zeros(*shape, dtype=dtype)
    return {"prev": [z(1, ch[k], 1, 160 >> k) for k in range(4)], "h1": [z(1, 1, Hg) for _ in range(g)],
            "h2": [z(1, 1, Hg) for _ in range(g)], "tail": z(HOP)}


@torch.no_grad()
def stream_clip(model, x: torch.Tensor, dtype=torch.float32):
    """x [L] (L a multiple of 160, >= 320) -> (enhanced [L], [intermediates of frames 0..L/160]), both in `dtype`"""
    model.eval()
    if model.conv1.weight.dtype != dtype:
        raise ValueError(f"stream_clip: the module's weights are {model.conv1.weight.dtype}, dtype is {dtype} (see as_double)")
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


def as_double(model):
    """a float64 copy of the module, for stream_clip(..., dtype=torch.float64)"""
    return copy.deepcopy(model).double().eval()


def nontrivial_bn(model, seed: int = 3) -> None:
    """running statistics away from (0, 1) so that folding them is tested"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.running_mean.numel()
                mod.running_mean.copy_(0.2 * torch.randn(n, generator=gen))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=gen))
