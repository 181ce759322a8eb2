"""Test-only: the CPU emulation of StreamingInferencer(precision="f16") -- tests/stream_ref.py's per-frame restatement with the four
GRU cells (two layers x groups) replaced by a hand-written cell that rounds x, h, W_ih and W_hh through torch.float16 and computes
everything else (products' accumulation, biases, gates, the carried h) in the module's dtype.  stream_ref.frame_step is reused
unchanged: it is handed a copy of the module whose gru_list1 / gru_list2 entries are these cells.

With rounding=False the cell restates torch.nn.GRU (pinned by tests/test_stream_f16_host.py), so the emulation differs from the
reference in the four roundings alone.  Also here: the models and clips the host and the GPU module share (same seeds).
"""
from __future__ import annotations

import copy

import torch

from oracle import cruse_oracle as O
from tests.stream_ref import as_double, nontrivial_bn, stream_clip

CONFIGS = {"g4": dict(rnn_groups=4), "g1": dict(rnn_groups=1), "small_g2": dict(ch=(1, 4, 8, 16, 32), rnn_groups=2)}
STAGES_F32 = ("e1", "e2", "e3", "e4", "skip1", "skip2", "skip3", "skip4")   # computed before the GRU in a frame: the f32 bar, 1e-5
STAGES_F16 = ("gru1", "gru2", "mask")                                        # behind an f16-operand product: the reduced bar, 1e-3
BAR_F32, BAR_F16 = 1e-5, 1e-3


class F16Cell(torch.nn.Module):
    """one GRU step, called as torch.nn.GRU(batch_first=True) on x [1, 1, Hg], h [1, 1, Hg] -> (y, h')"""

    def __init__(self, gru: torch.nn.GRU, rounding: bool = True):
        super().__init__()
        self.w_ih, self.w_hh = gru.weight_ih_l0.detach().clone(), gru.weight_hh_l0.detach().clone()
        self.b_ih, self.b_hh = gru.bias_ih_l0.detach().clone(), gru.bias_hh_l0.detach().clone()
        self.hidden_size = gru.hidden_size
        self.rounding = rounding

    def _op(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(torch.float16).to(t.dtype) if self.rounding else t

    def forward(self, x, h):
        Hg = self.hidden_size
        gi = self._op(x.reshape(-1)) @ self._op(self.w_ih).t() + self.b_ih
        gh = self._op(h.reshape(-1)) @ self._op(self.w_hh).t() + self.b_hh
        r = torch.sigmoid(gi[:Hg] + gh[:Hg])
        z = torch.sigmoid(gi[Hg:2 * Hg] + gh[Hg:2 * Hg])
        n = torch.tanh(gi[2 * Hg:] + r * gh[2 * Hg:])
        hn = ((1.0 - z) * n + z * h.reshape(-1)).view(1, 1, Hg)            # the carried h is not rounded
        return hn, hn


def emulation(model, rounding: bool = True):
    """a copy of the oracle module (any dtype) with every GRU replaced by an F16Cell"""
    m = copy.deepcopy(model).eval()
    for lst in (m.gru.gru_list1, m.gru.gru_list2):
        for i in range(len(lst)):
            lst[i] = F16Cell(lst[i], rounding)
    return m


def emulate_clip(model, x: torch.Tensor, dtype=torch.float32, rounding: bool = True):
    """stream_ref.stream_clip of the emulation: (enhanced [L], frames)"""
    return stream_clip(emulation(model, rounding), x, dtype=dtype)


def oracle_model(cfg, seed: int = 0):
    """torch-default initialisation under `seed`, BatchNorm statistics away from (0, 1), eval mode"""
    torch.manual_seed(seed)
    o = O.unet_2(**cfg)
    nontrivial_bn(o)
    return o.eval()


def gpu_model(o, cfg):
    """the product module carrying the oracle module's weights, on the device"""
    from cruse_amd.model.cruse_net import unet_2
    m = unet_2(precision="f32", **cfg)
    m.load_state_dict(o.state_dict())
    return m.cuda().eval()


def clip(n_blocks: int, seed: int) -> torch.Tensor:
    """0.1 * randn, n_blocks * 160 samples"""
    return 0.1 * torch.randn(160 * n_blocks, generator=torch.Generator().manual_seed(seed))


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def stage_distance(frames, frames64):
    """{stage: worst rel-L2 over the frames} of one restatement against the float64 one"""
    worst = {}
    for fa, fb in zip(frames, frames64):
        for k in STAGES_F32 + STAGES_F16:
            worst[k] = max(worst.get(k, 0.0), rel(fa[k], fb[k]))
    return worst


def references(o, x):
    """(float64 clip, float64 frames, emulated clip, emulated frames, the emulation's whole-clip distance from float64)"""
    ref, frames64 = stream_clip(as_double(o), x, dtype=torch.float64)
    emu, frames16 = emulate_clip(o, x)
    return ref, frames64, emu, frames16, rel(emu, ref)


# the clips of the accuracy tests, shared by tests/test_stream_f16_host.py and tests/test_gpu_stream_f16.py
ACC_BLOCKS, ACC_SEED = 200, 11          # 2 s, the three CONFIGS
SHAPE_BLOCKS, SHAPE_SEED = 12, 0        # the matrix of tests/stream_shapes.py


def alive_model(cfg, x: torch.Tensor, min_frac: float = 0.125, seeds=range(8)):
    """oracle_model under the first seed whose FLOAT64 restatement of clip x keeps every encoder stage alive: at least min_frac of the
    elements of e1..e4 non-zero in every frame from 1 on.  A narrow model (two channels) under the default initialisation can have an
    encoder level whose ReLUs are all but dead (seed 0 at ch = (1,2,2,2,2): one element of e2's 80 survives, 0.009 left of a
    cancellation of O(1) terms); the rel-L2 of such a vector measures the conditioning of that cancellation, not a kernel, and the
    per-stage bar of 1e-5 means nothing on it.  The choice looks at the reference alone, never at what the kernels give.
    On the matrix's clip it moves two of the twelve models from seed 0 to seed 1: hg20_g1 (e1 down to 9 %, e2 to 0 of 80 alive in some
    frame; the f32 encoder measured 1.3e-5 on e2 there) and hg200_odd (e2 down to 4 of 200 alive; the kernels measured 1.0e-6 on it
    at seed 0, inside the bar, so nothing is hidden by the move).  Every other model keeps seed 0 with every stage at least 45 % alive.
    min_frac = 1/8: a ReLU behind a symmetric initialisation keeps about half of its elements, which is what all the kept models show;
    an eighth is a quarter of that, between the two populations found (<= 9 % and >= 45 %), not fitted to any kernel figure.
    -> (module, seed)"""
    for seed in seeds:
        o = oracle_model(cfg, seed)
        _, frames64 = stream_clip(as_double(o), x, dtype=torch.float64)
        if all(float((f[k] != 0).double().mean()) >= min_frac for f in frames64[1:] for k in ("e1", "e2", "e3", "e4")):
            return o, seed
    raise AssertionError(f"no seed in {list(seeds)} keeps the encoder of {cfg} alive on this clip")
