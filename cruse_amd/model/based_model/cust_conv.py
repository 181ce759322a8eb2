"""MI355X-native `model.based_model.cust_conv` conv / grouped-GRU blocks (8f item 2).

Same constructor arguments, child modules (hence state-dict keys and default initialisation) and forward semantics as
model/based_model/cust_conv.py:15-184 (Conv2dNormAct, ConvTranspose2dNormAct, convkxf with its normal / transposed /
upsample modes and the depthwise + 1x1 form, FreqUpsample) and :250-416 (GroupedGRULayer, GroupGRU with the inter-layer
shuffle and add_outputs).  The children are parameter containers; forward runs the fused HIP kernels of
cruse_amd/nn_generic.py (conv blocks) and the persistent GRU recurrence kernels (cruse_amd/csrc/gru.hip).
Layout is the reference's [B,C,T,F] / [B,T,I].  No CPU path.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch
from torch import Tensor, nn

from ... import ops
from ...nn_generic import FreqUpsample, HipSequential  # noqa: F401  (FreqUpsample is part of this module's surface)


class Conv2dNormAct(HipSequential):
    """cust_conv.py:15-62.  [B,C,T,F]; causal pad of kernel_size[0]-1 frames on top, frequency stride `fstride`."""

    def __init__(self, in_ch, out_ch, kernel_size, fstride=1, dilation=1, fpad=True, bias=True, separable=False,
                 norm_layer=torch.nn.BatchNorm2d, activation_layer=torch.nn.ReLU):
        lookahead = 0
        kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        fpad_ = kernel_size[1] // 2 + dilation - 1 if fpad else 0                     # :33-36
        pad = (0, 0, kernel_size[0] - 1 - lookahead, lookahead)                        # :37
        layers = []
        if any(x > 0 for x in pad):
            layers.append(nn.ConstantPad2d(pad, 0.0))
        groups = math.gcd(in_ch, out_ch) if separable else 1                           # :41
        if groups == 1:
            separable = False
        if max(kernel_size) == 1:
            separable = False
        layers.append(nn.Conv2d(in_ch, out_ch, kernel_size, padding=(0, fpad_), stride=(1, fstride),
                                dilation=(1, dilation), groups=groups, bias=bias))    # :46-55
        if separable:
            layers.append(nn.Conv2d(out_ch, out_ch, kernel_size=1, bias=False))        # :56-57
        if norm_layer is not None:
            layers.append(norm_layer(out_ch))
        if activation_layer is not None:
            layers.append(activation_layer())
        super().__init__(*layers)


class ConvTranspose2dNormAct(HipSequential):
    """cust_conv.py:65-111."""

    def __init__(self, in_ch, out_ch, kernel_size, fstride=1, dilation=1, fpad=True, bias=True, separable=False,
                 norm_layer=torch.nn.BatchNorm2d, activation_layer=torch.nn.ReLU):
        lookahead = 0
        kernel_size = (kernel_size, kernel_size) if isinstance(kernel_size, int) else kernel_size
        fpad_ = kernel_size[1] // 2 if fpad else 0                                     # :79-82
        pad = (0, 0, kernel_size[0] - 1 - lookahead, lookahead)
        layers = []
        if any(x > 0 for x in pad):
            layers.append(nn.ConstantPad2d(pad, 0.0))
        groups = math.gcd(in_ch, out_ch) if separable else 1
        if groups == 1:
            separable = False
        layers.append(nn.ConvTranspose2d(in_ch, out_ch, kernel_size=kernel_size,
                                         padding=(kernel_size[0] - 1, fpad_ + dilation - 1), output_padding=(0, fpad_),
                                         stride=(1, fstride), dilation=(1, dilation), groups=groups, bias=bias))  # :93-104
        if separable:
            layers.append(nn.Conv2d(out_ch, out_ch, kernel_size=1, bias=False))
        if norm_layer is not None:
            layers.append(norm_layer(out_ch))
        if activation_layer is not None:
            layers.append(activation_layer())
        super().__init__(*layers)


def convkxf(in_ch, out_ch, k=1, f=3, fstride=2, lookahead=0, batch_norm=False, act=None, mode="normal", depthwise=True,
            complex_in=False):
    """cust_conv.py:114-174; `act` defaults to nn.ReLU(inplace=True) as there."""
    if act is None:
        act = torch.nn.ReLU(inplace=True)
    bias = batch_norm is False
    assert f % 2 == 1
    stride = 1 if f == 1 else (1, fstride)
    if out_ch is None:
        out_ch = in_ch * 2 if mode == "normal" else in_ch // 2
    fpad = (f - 1) // 2
    convpad = (0, fpad)
    modules = []
    pad = [0, 0, k - 1 - lookahead, lookahead]
    if any(p > 0 for p in pad):
        modules.append(("pad", nn.ConstantPad2d(pad, 0.0)))
    groups = min(in_ch, out_ch) if depthwise else 1
    if in_ch % groups != 0 or out_ch % groups != 0:
        groups = 1
    if complex_in and groups % 2 == 0:
        groups //= 2
    convkwargs = {"in_channels": in_ch, "out_channels": out_ch, "kernel_size": (k, f), "stride": stride, "groups": groups,
                  "bias": bias}
    if mode == "normal":
        modules.append(("sconv", nn.Conv2d(padding=convpad, **convkwargs)))
    elif mode == "transposed":
        modules.append(("sconv", nn.ConvTranspose2d(padding=(k - 1, fpad), output_padding=convpad, **convkwargs)))
    elif mode == "upsample":
        modules.append(("upsample", FreqUpsample(fstride)))
        convkwargs["stride"] = 1
        modules.append(("sconv", nn.Conv2d(padding=convpad, **convkwargs)))
    else:
        raise NotImplementedError()
    if groups > 1:
        modules.append(("1x1conv", nn.Conv2d(out_ch, out_ch, 1, bias=False)))
    if batch_norm:
        modules.append(("norm", nn.BatchNorm2d(out_ch)))
    modules.append(("act", act))
    return HipSequential(OrderedDict(modules))


# ======================================================================================================================
# grouped GRUs
# ======================================================================================================================
class _GroupedGruFn(torch.autograd.Function):
    """g independent nn.GRU(I/g -> H/g) over feature slices, outputs concatenated (cust_conv.py:303-325), started from the
    state h0 [B, H] ("cat" layout) the caller passes -- DETACHED, as the reference does (:318-319): no gradient flows into
    it -- or from 0.  params = (w_ih_0, w_hh_0, b_ih_0, b_hh_0, w_ih_1, ...).  Exact-f32 MFMA kernels (v_mfma_f32_16x16x4_f32)."""

    @staticmethod
    def forward(ctx, x, g, h0, *params):
        x = x.contiguous()
        B, T, I = x.shape
        Ig = I // g
        Hg = params[1].shape[1]
        H = g * Hg
        rows = B * T
        gi = torch.empty(B, T, g * 3 * Hg, device=x.device, dtype=torch.float32)
        for i in range(g):
            w_ih, b_ih = params[4 * i], params[4 * i + 2]
            ops.gemm(False, True, rows, 3 * Hg, Ig, x, i * Ig, I, w_ih.contiguous(), 0, Ig, gi, i * 3 * Hg, 3 * H, bias=b_ih,
                     prec="f32")
        w_hh = [params[4 * i + 1].contiguous() for i in range(g)]
        b_hh = [params[4 * i + 3].contiguous() for i in range(g)]
        need = any(ctx.needs_input_grad)
        h, coef, an, z = ops.gru_seq_fwd(gi, w_hh, b_hh, B, T, g, Hg, "f32", save=need, h0=h0)
        ctx.g, ctx.dims = g, (B, T, I, Ig, Hg)
        ctx.h0 = h0
        ctx.save_for_backward(x, h, coef, an, z, *params)
        return h

    @staticmethod
    def backward(ctx, dout):
        x, h, coef, an, z, *params = ctx.saved_tensors
        g = ctx.g
        B, T, I, Ig, Hg = ctx.dims
        H, rows = g * Hg, B * T
        w_hh = [params[4 * i + 1].contiguous() for i in range(g)]
        dh = ops.gru_seq_bwd(dout.contiguous(), w_hh, coef, z, B, T, g, Hg, "f32")
        dgi, dgh = ops.gru_gate_grads(dh, coef, an, rows, g, Hg, "f32")
        grads = []
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        sk = max(1, min(8, rows // 512))
        for i in range(g):
            w_ih = params[4 * i].contiguous()
            dw_ih = torch.zeros_like(w_ih); dw_hh = torch.zeros_like(w_hh[i])
            db_ih = torch.zeros(3 * Hg, device=x.device); db_hh = torch.zeros(3 * Hg, device=x.device)
            ops.gemm(True, False, 3 * Hg, Ig, rows, dgi, i * 3 * Hg, 3 * H, x, i * Ig, I, dw_ih, 0, Ig, accumulate=True,
                     splitk=sk, prec="f32")
            ops.gemm(True, False, 3 * Hg, Hg, rows, dgh, i * 3 * Hg, 3 * H, h, i * Hg, H, dw_hh, 0, Hg, accumulate=True,
                     splitk=sk, b_shift_T=T, prec="f32")
            if ctx.h0 is not None:
                # frame 0's h_{t-1} is h0, not 0: dW_hh += dgh[:, 0]^T h0 (K = B; rows of frame 0 are T frames apart)
                ops.gemm(True, False, 3 * Hg, Hg, B, dgh, i * 3 * Hg, T * 3 * H, ctx.h0, i * Hg, H, dw_hh, 0, Hg, accumulate=True,
                         prec="f32")
            ops.col_sum(dgi, i * 3 * Hg, rows, 3 * Hg, 3 * H, db_ih)
            ops.col_sum(dgh, i * 3 * Hg, rows, 3 * Hg, 3 * H, db_hh)
            if dx is not None:
                ops.gemm(False, False, rows, Ig, 3 * Hg, dgi, i * 3 * Hg, 3 * H, w_ih, 0, Ig, dx, i * Ig, I, prec="f32")
            grads += [dw_ih, dw_hh, db_ih, db_hh]
        return (dx, None, None) + tuple(grads)



class GroupedGRULayer(nn.Module):
    """cust_conv.py:250-325."""

    def __init__(self, input_size: int, hidden_size: int, groups: int, batch_first: bool = True, bias=True,
                 dropout: float = 0, bidirectional=False):
        super().__init__()
        assert input_size % groups == 0
        assert hidden_size % groups == 0
        # dropout: nn.GRU applies it BETWEEN stacked layers only; every group's nn.GRU here has one layer (cust_conv.py:286-287), so the
        # reference's argument has no effect either (torch warns) -- it is accepted and kept in the sub-modules' kwargs
        kwargs = {"bias": bias, "batch_first": batch_first, "dropout": dropout, "bidirectional": bidirectional}
        self.input_size = input_size // groups
        self.hidden_size = hidden_size // groups
        self.out_size = hidden_size
        self.bidirectional = bidirectional
        self.num_directions = 2 if bidirectional else 1
        self.groups = groups
        self.batch_first = batch_first
        assert (self.hidden_size % groups) == 0, "Hidden size must be divisible by groups"       # :284-285
        if self.hidden_size % 32:
            raise RuntimeError(f"cruse_amd GroupedGRULayer: hidden size per group {self.hidden_size} must be a multiple of 32")
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                 # (torch: "dropout expects num_layers greater than 1")
            self.layers = nn.ModuleList(nn.GRU(self.input_size, self.hidden_size, **kwargs) for _ in range(groups))

    def flatten_parameters(self):
        pass

    def get_h0(self, batch_size: int = 1, device: torch.device = torch.device("cpu")):
        return torch.zeros(self.groups * self.num_directions, batch_size, self.hidden_size, device=device)

    def _direction(self, x: Tensor, h0c: Optional[Tensor], suffix: str) -> Tensor:
        params = []
        for layer in self.layers:
            w_ih, w_hh = getattr(layer, "weight_ih_l0" + suffix), getattr(layer, "weight_hh_l0" + suffix)
            if layer.bias:
                b_ih, b_hh = getattr(layer, "bias_ih_l0" + suffix), getattr(layer, "bias_hh_l0" + suffix)
            else:
                # nn.GRU(bias=False) (cust_conv.py:262,272) has no bias parameters: the kernels take zero vectors (one shared
                # buffer, no gradient asked for -- what _GroupedGruFn returns for them is dropped by autograd)
                b_ih = b_hh = self._zero_bias(w_ih.device)
            params += [w_ih, w_hh, b_ih, b_hh]
        return _GroupedGruFn.apply(x, self.groups, h0c, *params)

    def _zero_bias(self, device) -> Tensor:
        z = getattr(self, "_zb", None)
        if z is None or z.device != device:
            z = torch.zeros(3 * self.hidden_size, device=device)
            object.__setattr__(self, "_zb", z)                # (not a buffer: the state dict stays the reference's)
        return z

    def forward(self, input: Tensor, h0: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        # state [G*D, B, H/g] (:305-306; group-major, direction-minor) -> the kernel's [B, G*H/g] "cat" layout per direction;
        # detached like the reference's (:319)
        if not self.batch_first:
            # [T, B, I] (cust_conv.py:306): the kernels are batch-major -- one device transposition in, one out; the state
            # layout [G*D, B, H/g] does not depend on batch_first (torch)
            y, hn = self._forward_bf(input.transpose(0, 1), h0)
            return y.transpose(0, 1).contiguous(), hn
        return self._forward_bf(input, h0)

    def _forward_bf(self, input: Tensor, h0: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        B, D, g, Hg = input.shape[0], self.num_directions, self.groups, self.hidden_size
        h0d = [None] * D
        if h0 is not None:
            if tuple(h0.shape) != (g * D, B, Hg):
                raise RuntimeError(f"GroupedGRULayer: state {tuple(h0.shape)} != {(g * D, B, Hg)}")
            st = h0.detach().to(input.device, torch.float32).view(g, D, B, Hg)
            h0d = [st[:, d].transpose(0, 1).reshape(B, -1).contiguous() for d in range(D)]
        out = self._direction(input, h0d[0], "")
        if not self.bidirectional:
            # final states [G, B, H/g] = the last frame of every group's slice (cust_conv.py:323)
            return out, out[:, -1, :].reshape(B, g, Hg).transpose(0, 1).contiguous()
        # the reverse direction (nn.GRU(bidirectional=True): weights *_reverse) is the same recurrence on the time-reversed
        # sequence, its outputs reversed back; a group's output is [forward | reverse] (torch), the groups are concatenated
        # after that (:322), and a group's two final states are h_{T-1} of the forward and h_0 of the reverse direction
        rev = torch.flip(self._direction(torch.flip(input, dims=(1,)), h0d[1], "_reverse"), dims=(1,))
        T = out.shape[1]
        y = torch.stack((out.view(B, T, g, Hg), rev.view(B, T, g, Hg)), dim=3).reshape(B, T, g * 2 * Hg)
        hf = out[:, -1, :].reshape(B, g, Hg)
        hr = rev[:, 0, :].reshape(B, g, Hg)
        return y, torch.stack((hf, hr), dim=2).permute(1, 2, 0, 3).reshape(g * 2, B, Hg).contiguous()


class GroupGRU(nn.Module):
    """cust_conv.py:328-416: stacked GroupedGRULayers with the inter-layer feature shuffle
    view(B,T,-1,g).transpose(2,3) (:408-410) and optional add_outputs."""

    def __init__(self, input_size, hidden_size, num_layers=1, groups=4, bias=True, batch_first=True, dropout=0.,
                 bidirectional=False, shuffle=True, add_outputs=False):
        super().__init__()
        kwargs = {"groups": groups, "bias": bias, "batch_first": batch_first, "dropout": dropout,
                  "bidirectional": bidirectional}
        assert input_size % groups == 0
        assert hidden_size % groups == 0
        assert num_layers > 0
        self.input_size = input_size
        self.groups = groups
        self.num_layers = num_layers
        self.batch_first = batch_first
        self.hidden_size = hidden_size // groups
        self.bidirectional = bidirectional
        self.num_directions = 1
        if self.groups == 1:
            shuffle = False
        self.shuffle = shuffle
        self.add_outputs = add_outputs
        self.grus = nn.ModuleList()
        self.grus.append(GroupedGRULayer(input_size, hidden_size, **kwargs))
        for _ in range(1, num_layers):
            self.grus.append(GroupedGRULayer(hidden_size, hidden_size, **kwargs))

    def flatten_parameters(self):
        pass

    def get_h0(self, batch_size: int, device=None) -> Tensor:
        # the reference's forward calls get_h0(b, input.device) against a one-argument signature (:383-389,:397): the
        # evident intent (device optional) is what is implemented
        return torch.zeros((self.num_layers * self.groups * self.num_directions, batch_size, self.hidden_size), device=device)

    def forward(self, input: Tensor, state: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        dim0, dim1, _ = input.shape
        h = self.groups * self.num_directions
        if state is not None and state.shape[0] != self.num_layers * h:
            raise RuntimeError(f"GroupGRU: state has {state.shape[0]} rows, expected num_layers*groups = {self.num_layers * h}")
        output = None
        outstates = []
        for i, gru in enumerate(self.grus):
            input, s = gru(input, None if state is None else state[i * h:(i + 1) * h])                  # :402-404
            outstates.append(s)
            if self.shuffle and i < self.num_layers - 1:
                # a pure permutation of the feature axis: new[b*h + a] = old[a*g + b] (device copy, no arithmetic)
                input = input.view(dim0, dim1, -1, self.groups).transpose(2, 3).reshape(dim0, dim1, -1)
            if self.add_outputs:
                from ...nn_generic import add
                output = input if output is None else add(output, input.contiguous())
            else:
                output = input
        return output, torch.cat(outstates, dim=0)


# ======================================================================================================================
# grouped linears, squeezed GRUs, ERB bands (cust_conv.py:187-247, :419-579)
# ======================================================================================================================
class GroupedLinearEinsum(nn.Module):
    """cust_conv.py:503-542: weight [G, I/G, H/G], einsum("btgi,gih->btgh") flattened to [B, T, H] -- one cruse_grouped_linear_fwd
    launch for all groups (exact-f32 MFMA), gradients through cruse_grouped_linear_bwd_dx / _bwd_dw."""

    def __init__(self, input_size: int, hidden_size: int, groups: int = 1):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.groups = groups
        assert input_size % groups == 0, f"Input size {input_size} not divisible by {groups}"
        assert hidden_size % groups == 0, f"Hidden size {hidden_size} not divisible by {groups}"
        self.ws = input_size // groups
        self.register_parameter("weight", nn.Parameter(torch.zeros(groups, input_size // groups, hidden_size // groups),
                                                       requires_grad=True))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def _run(self, x: Tensor, relu: bool) -> Tensor:
        b, t, i = x.shape                                                               # (:530: three dimensions, as there)
        if i != self.input_size:
            raise RuntimeError(f"GroupedLinearEinsum: input has {i} features, expected {self.input_size}")
        y = ops.GroupedLinearFn.apply(x.reshape(b * t, i), self.weight, None, "gih", relu, False)
        return y.view(b, t, self.hidden_size)

    def forward(self, x: Tensor) -> Tensor:
        return self._run(x, False)

    def __repr__(self):
        cls = self.__class__.__name__
        return f"{cls}(input_size: {self.input_size}, hidden_size: {self.hidden_size}, groups: {self.groups})"


class GroupedLinear(nn.Module):
    """cust_conv.py:545-579: `groups` nn.Linear layers over feature slices, outputs concatenated and, with shuffle, interleaved by
    view(-1, H/G, G).transpose(-1, -2).  The layers are the parameter containers: per call their weights are gathered into one
    [G, H/G, I/G] operand (and the biases into [H]) for one launch, the shuffle is the kernel's store index, and autograd scatters the
    gradients of the gathered operands back to the layers.  Any leading dimensions, as the reference's slicing allows."""

    def __init__(self, input_size: int, hidden_size: int, groups: int = 1, shuffle: bool = True):
        super().__init__()
        assert input_size % groups == 0
        assert hidden_size % groups == 0
        self.groups = groups
        self.input_size = input_size // groups
        self.hidden_size = hidden_size // groups
        if groups == 1:
            shuffle = False
        self.shuffle = shuffle
        self.layers = nn.ModuleList(nn.Linear(self.input_size, self.hidden_size) for _ in range(groups))

    def forward(self, x: Tensor) -> Tensor:
        if x.shape[-1] != self.groups * self.input_size:
            raise RuntimeError(f"GroupedLinear: input has {x.shape[-1]} features, expected {self.groups * self.input_size}")
        w = torch.stack([layer.weight for layer in self.layers])                       # [G, H/G, I/G]
        bias = torch.cat([layer.bias for layer in self.layers])                         # [H], group-major
        y = ops.GroupedLinearFn.apply(x.reshape(-1, x.shape[-1]), w, bias, "ghi", False, self.shuffle)
        return y.view(*x.shape[:-1], self.groups * self.hidden_size)


def _linear_act(seq: nn.Module, x: Tensor) -> Tensor:
    """Sequential(GroupedLinearEinsum, act) of SqueezedGRU(_S): nn.Identity / nn.ReLU run in the kernel's epilogue, any other
    activation module is applied to the kernel's output as it is."""
    if isinstance(seq, nn.Identity):
        return x
    lin, act = seq[0], seq[1]
    if type(act) is nn.Identity:
        return lin._run(x, False)
    if type(act) is nn.ReLU:
        return lin._run(x, True)
    return act(lin._run(x, False))


class _StackedGruFn(_GroupedGruFn):
    """_GroupedGruFn at g = 1 -- its forward, its recurrence backward and its gate gradients -- with the parameter gradients summed
    in one order: _GroupedGruFn's bias gradients (ops.col_sum) and, from 1024 rows, its split-K weight gradients add with atomics,
    so two runs differ in the last bits.  Here dW_ih / db_ih and dW_hh / db_hh each come from one cruse_grouped_linear_bwd_dw
    launch (G = 1, the nn.GRU layout [3H, I] is its stacked-Linear layout; fixed-order row split), the latter against
    h_{t-1} = (h0 or 0, h_0 .. h_{T-2}) laid out by one device copy, and dX from cruse_grouped_linear_bwd_dx."""

    @staticmethod
    def backward(ctx, dout):
        x, h, coef, an, z, w_ih, w_hh, _, _ = ctx.saved_tensors
        B, T, I, _, H = ctx.dims
        rows = B * T
        dh = ops.gru_seq_bwd(dout.contiguous(), [w_hh.contiguous()], coef, z, B, T, 1, H, "f32")
        dgi, dgh = ops.gru_gate_grads(dh, coef, an, rows, 1, H, "f32")
        dgi, dgh = dgi.view(rows, 3 * H), dgh.view(rows, 3 * H)
        first = ctx.h0.view(B, 1, H) if ctx.h0 is not None else h.new_zeros(B, 1, H)
        h_prev = torch.cat((first, h[:, :-1]), dim=1).view(rows, H)
        dw_ih, db_ih = ops.grouped_linear_bwd_dw(dgi, x.view(rows, I), (1, 3 * H, I), "ghi", want_db=True)
        dw_hh, db_hh = ops.grouped_linear_bwd_dw(dgh, h_prev, (1, 3 * H, H), "ghi", want_db=True)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.grouped_linear_bwd_dx(dgi, w_ih.contiguous().view(1, 3 * H, I), "ghi").view(B, T, I)
        return dx, None, None, dw_ih[0], dw_hh[0], db_ih, db_hh


class _SqueezedBase(nn.Module):
    def __init__(self, input_size: int, hidden_size: int, output_size: Optional[int] = None, num_layers: int = 1, linear_groups: int = 8,
                 batch_first: bool = True, gru_skip_op=None, linear_act_layer=nn.Identity):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        if hidden_size % 32:
            raise RuntimeError(f"cruse_amd {type(self).__name__}: hidden size {hidden_size} must be a multiple of 32")
        self.linear_in = nn.Sequential(GroupedLinearEinsum(input_size, hidden_size, linear_groups), linear_act_layer())
        self.gru = nn.GRU(hidden_size, hidden_size, num_layers=num_layers, batch_first=batch_first)   # the parameter container
        self.gru_skip = gru_skip_op() if gru_skip_op is not None else None
        if output_size is not None:
            self.linear_out = nn.Sequential(GroupedLinearEinsum(hidden_size, output_size, linear_groups), linear_act_layer())
        else:
            self.linear_out = nn.Identity()

    def _gru(self, x: Tensor, h: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        """The stacked nn.GRU on batch-major x [B, T, hidden]: every layer is _GroupedGruFn with one group (_StackedGruFn: the same
        forward and recurrence, parameter gradients in a fixed order)."""
        L, B, H = self.gru.num_layers, x.shape[0], self.hidden_size
        if h is not None:
            if tuple(h.shape) != (L, B, H):
                raise RuntimeError(f"{type(self).__name__}: state {tuple(h.shape)} != {(L, B, H)}")
            h = h.detach().to(x.device, torch.float32)
        states = []
        for k in range(L):
            params = [getattr(self.gru, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            x = _StackedGruFn.apply(x, 1, None if h is None else h[k].contiguous(), *params)
            states.append(x[:, -1, :])
        return x, torch.stack(states, dim=0)

    def _skip(self, x: Tensor, inp: Tensor) -> Tensor:
        from ...nn_generic import add
        if self.gru_skip is None:
            return x
        if type(self.gru_skip) is not nn.Identity:
            inp = self.gru_skip(inp)
        return add(x, inp.contiguous())

    def forward(self, input: Tensor, h: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        if not self.gru.batch_first:
            # [T, B, I]: the kernels are batch-major -- one device transposition in, one out; h is [num_layers, B, hidden] either way
            y, hn = self._forward_bf(input.transpose(0, 1).contiguous(), h)
            return y.transpose(0, 1).contiguous(), hn
        return self._forward_bf(input.contiguous(), h)


class SqueezedGRU(_SqueezedBase):
    """cust_conv.py:419-458: grouped linear in (+ activation), nn.GRU(hidden, hidden, num_layers), the skip added after the GRU and
    before linear_out, grouped linear out (+ activation) or Identity.  Same arguments, children (linear_in, gru, gru_skip, linear_out)
    and state-dict keys.  h is [num_layers, B, hidden] in and out.  A passed h is DETACHED, as GroupedGRULayer's is: torch's nn.GRU
    would propagate a gradient into it, this block does not.  hidden_size must be a multiple of 32 (RuntimeError)."""

    def _forward_bf(self, input: Tensor, h: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        input = _linear_act(self.linear_in, input)
        x, h = self._gru(input, h)
        x = self._skip(x, input)
        return _linear_act(self.linear_out, x), h


class SqueezedGRU_S(_SqueezedBase):
    """cust_conv.py:461-500: as SqueezedGRU, but the skip is added after linear_out, onto the block's own input (so output_size must
    equal input_size when a skip is used).  A passed h is DETACHED (see SqueezedGRU)."""

    def _forward_bf(self, input: Tensor, h: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        x = _linear_act(self.linear_in, input)
        x, h = self._gru(x, h)
        x = _linear_act(self.linear_out, x)
        return self._skip(x, input), h


def freq2erb(freq_hz):
    """cust_conv.py:210-211"""
    return 9.265 * torch.log1p(freq_hz / (24.7 * 9.265))


def erb2freq(n_erb):
    """cust_conv.py:214-215"""
    return 24.7 * 9.265 * (torch.exp(n_erb / 9.265) - 1.)


def erb_fb(sr, fft_size, nb_bands, min_nb_freqs):
    """cust_conv.py:218-247: widths (int16 [nb_bands]) of non-overlapping ERB-spaced bands over the fft_size / 2 + 1 bins, every band at
    least min_nb_freqs wide; f32 arithmetic as there, so the widths are the reference's integer for integer."""
    freq_width = sr / fft_size
    erb_low = freq2erb(torch.Tensor([0.]))
    erb_high = freq2erb(torch.Tensor([sr / 2]))
    step = (erb_high - erb_low) / nb_bands
    erb = torch.zeros([nb_bands], dtype=torch.int16)
    prev_freq, freq_over = 0, 0
    for i in range(nb_bands):
        fb = int(torch.round(erb2freq(erb_low + (i + 1) * step) / freq_width))
        nb_freqs = fb - prev_freq - freq_over
        if nb_freqs < min_nb_freqs:
            freq_over = min_nb_freqs - nb_freqs                                         # borrowed from the next band
            nb_freqs = min_nb_freqs
        else:
            freq_over = 0
        erb[i] = nb_freqs
        prev_freq = fb
    erb[nb_bands - 1] += 1                                                              # the Nyquist bin
    too_large = torch.sum(erb) - (fft_size / 2 + 1)
    if too_large > 0:
        erb[nb_bands - 1] -= too_large
    assert torch.sum(erb) == (fft_size / 2 + 1)
    return erb


def _widths(width) -> List[int]:
    w = width.tolist() if hasattr(width, "tolist") else list(width)
    return [int(v) for v in w]


def erb_fb_use(width, sr: int, normalized: bool = True, inverse: bool = False) -> Tensor:
    """cust_conv.py:187-207: the dense filterbank matrix, [F, n_bands] with 1 (normalized: 1 / width) over every band's bins, or its
    transpose [n_bands, F] with 1 (NOT normalized: 1 / width -- the reference's asymmetry).  For users who want the matrix; the device
    products are erb_apply / erb_apply_inverse.  sr does not enter the values (the reference builds a frequency axis only for its length)."""
    w = _widths(width)
    fb = torch.zeros((sum(w), len(w)))
    b = 0
    for i, n in enumerate(w):
        fb[b:b + n, i] = 1
        b += n
    if inverse:
        fb = fb.t()
        if not normalized:
            fb /= fb.sum(dim=1, keepdim=True)
    elif normalized:
        fb /= fb.sum(dim=0)
    return fb


_BAND_TABLES = {}


def _band_table(width, device) -> Tuple[Tensor, int]:
    """int32 [n_bands + 1] start offsets of the bands on `device` (built once per width list and device, so that a captured graph
    replays without a host copy) and F = the sum of the widths; the table is judged here, on the host."""
    w = tuple(_widths(width))
    key = (w, str(device))
    hit = _BAND_TABLES.get(key)
    if hit is None:
        if not w or min(w) < 1:
            raise RuntimeError(f"erb bands: every width must be >= 1, got {list(w)}")
        if sum(w) > ops.BAND_MAX_F:
            raise RuntimeError(f"erb bands: {sum(w)} bins, at most {ops.BAND_MAX_F}")
        starts = [0]
        for n in w:
            starts.append(starts[-1] + n)
        hit = (torch.tensor(starts, dtype=torch.int32).to(device), starts[-1])
        _BAND_TABLES[key] = hit
    return hit


def erb_apply(x: Tensor, width, normalized: bool = True) -> Tensor:
    """x [..., F] @ erb_fb_use(width, sr, normalized) -> [..., n_bands] as band sums (cruse_band_pool): no matrix of zeros."""
    starts, F = _band_table(width, x.device)
    if x.shape[-1] != F:
        raise RuntimeError(f"erb_apply: {x.shape[-1]} bins, the widths sum to {F}")
    y = ops.BandPoolFn.apply(x.reshape(-1, F), starts, bool(normalized))
    return y.view(*x.shape[:-1], starts.numel() - 1)


def erb_apply_inverse(m: Tensor, width, normalized: bool = True) -> Tensor:
    """m [..., n_bands] @ erb_fb_use(width, sr, normalized, inverse=True) -> [..., F] (cruse_band_expand); divides by the width when
    NOT normalized, as the reference's matrix does."""
    starts, F = _band_table(width, m.device)
    nb = starts.numel() - 1
    if m.shape[-1] != nb:
        raise RuntimeError(f"erb_apply_inverse: {m.shape[-1]} bands, the table has {nb}")
    y = ops.BandExpandFn.apply(m.reshape(-1, nb), starts, F, not normalized)
    return y.view(*m.shape[:-1], F)
