"""Stock-torch CPU restatement of the grouped linears and squeezed GRUs of DESIGN section 17 (nn.GRU, einsum, nn.Linear; autograd
for the gradients): the reference of tests/test_gpu_grouped_linear.py.  Written from the semantics, independent of cruse_amd: the
modules carry the same child names, so a state dict of the device modules loads into them."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn


def shuffle_columns(y: torch.Tensor, G: int) -> torch.Tensor:
    """GroupedLinear(shuffle=True): the last axis [G * Hg] viewed as [Hg, G], transposed, flattened"""
    Hg = y.shape[-1] // G
    return y.reshape(-1, Hg, G).transpose(-1, -2).reshape(y.shape)


def grouped_linear(x, w_gih, bias=None, relu=False, shuffle=False):
    """x [rows, G * Ig], w_gih [G, Ig, Hg], bias [G * Hg] -> [rows, G * Hg]"""
    G, Ig, Hg = w_gih.shape
    y = torch.einsum("rgi,gih->rgh", x.reshape(x.shape[0], G, Ig), w_gih).reshape(x.shape[0], G * Hg)
    if bias is not None:
        y = y + bias
    if relu:
        y = torch.relu(y)
    return shuffle_columns(y, G) if shuffle else y


class Einsum(nn.Module):
    def __init__(self, input_size, hidden_size, groups=1):
        super().__init__()
        self.groups = groups
        self.weight = nn.Parameter(torch.zeros(groups, input_size // groups, hidden_size // groups))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def forward(self, x):
        lead = x.shape[:-1]
        y = torch.einsum("...gi,gih->...gh", x.reshape(*lead, self.groups, -1), self.weight)
        return y.reshape(*lead, -1)


class Squeezed(nn.Module):
    """late_skip False: SqueezedGRU (skip after the GRU, before linear_out); True: SqueezedGRU_S (skip after linear_out, onto the input)"""

    def __init__(self, input_size, hidden_size, output_size=None, num_layers=1, linear_groups=8, batch_first=True, gru_skip_op=None,
                 linear_act_layer=nn.Identity, late_skip=False):
        super().__init__()
        self.late_skip = late_skip
        self.linear_in = nn.Sequential(Einsum(input_size, hidden_size, linear_groups), linear_act_layer())
        self.gru = nn.GRU(hidden_size, hidden_size, num_layers=num_layers, batch_first=batch_first)
        self.gru_skip = gru_skip_op() if gru_skip_op is not None else None
        self.linear_out = (nn.Sequential(Einsum(hidden_size, output_size, linear_groups), linear_act_layer())
                           if output_size is not None else nn.Identity())

    def forward(self, inp, h: Optional[torch.Tensor] = None):
        z = self.linear_in(inp)
        x, h = self.gru(z, h)
        if self.late_skip:
            x = self.linear_out(x)
            if self.gru_skip is not None:
                x = x + self.gru_skip(inp)
            return x, h
        if self.gru_skip is not None:
            x = x + self.gru_skip(z)
        return self.linear_out(x), h


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
