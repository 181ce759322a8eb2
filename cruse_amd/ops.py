"""Torch-tensor wrappers over the C ABI (include/cruse_hip.h).

torch is used here for device memory and the current HIP stream only; every
arithmetic op is a kernel in libcruse_hip.so.  All tensors are f32 CUDA(HIP)
tensors in frame-major [B,T,C,F] layout unless stated.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import torch

from ._lib import PREC_BF16, PREC_BF16X3, PREC_BY_NAME, PREC_F32, SIGNATURES, check, lib  # noqa: F401


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("cruse_amd ops need tensors on the HIP device (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError(f"cruse_amd ops need contiguous tensors, got strides {t.stride()} for shape {tuple(t.shape)}")
    return t.data_ptr()


def _at(t: Optional[torch.Tensor], off: int, esize: int = 2):
    """address of element `off` of t's storage view (esize bytes per element: the 2-byte GEMM operands by default); None stays None"""
    return None if t is None else t.data_ptr() + esize * off


def _xdt(t: torch.Tensor, name: str) -> int:
    """CRUSE_DT_* of a conv / weight-gradient INPUT: f32, or bf16 for the backward-only tensors of the bf16 mode."""
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.bfloat16:
        return 2
    raise RuntimeError(f"{name}: expected float32 or bfloat16, got {t.dtype}")


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected float32, got {t.dtype}")
    return t


def set_option(name: str, value=None) -> None:
    """Library option (cruse_set_option: kernel-selection A/B switches and profiling aids -- the library reads no
    environment variables); value None restores the default."""
    check(lib.cruse_set_option(name.encode(), 0 if value is None else int(value), 1 if value is None else 0))


def get_option(name: str):
    v, isset = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.cruse_get_option(name.encode(), ctypes.byref(v), ctypes.byref(isset)))
    return v.value if isset.value else None


class options:
    """with ops.options(gru_bwd_rs=0, gru_wlo=0): ...  -- library options for the duration of the block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            set_option(k, v)


def prec_code(prec) -> int:
    if isinstance(prec, str):
        return PREC_BY_NAME[prec]
    return int(prec)


# ---------------------------------------------------------------- STFT / iSTFT
def stft_frames(L: int, hop: int) -> int:
    return 1 + L // hop


def stft(wave: torch.Tensor, n_fft: int, hop: int, want_ri: bool = True, mag_bins: int = 0,
         mag_eps: float = 0.0, out=None):
    """wave [B,L] -> (re [B,T,F], im [B,T,F], mag [B,T,mag_bins]); absent outputs are None.
    out = (re, im, mag): write into these (None entries are not produced) instead of allocating."""
    _f32(wave, "stft")
    if wave.dim() != 2:
        raise RuntimeError(f"stft expects [B,L], got {tuple(wave.shape)}")
    B, L = wave.shape
    T = stft_frames(L, hop)
    F = n_fft // 2 + 1
    if out is not None:
        re, im, mag = out
        mag_bins = mag.shape[-1] if mag is not None else 0
    else:
        re = torch.empty(B, T, F, device=wave.device, dtype=torch.float32) if want_ri else None
        im = torch.empty(B, T, F, device=wave.device, dtype=torch.float32) if want_ri else None
        mag = torch.empty(B, T, mag_bins, device=wave.device, dtype=torch.float32) if mag_bins > 0 else None
    check(lib.cruse_stft_fwd(_p(wave), B, L, n_fft, hop, _p(re), _p(im), _p(mag), mag_bins, mag_eps, _stream()))
    return re, im, mag


def istft(re: torch.Tensor, im: torch.Tensor, n_fft: int, hop: int, length: int) -> torch.Tensor:
    B, T, F = re.shape
    if F != n_fft // 2 + 1 or im.shape != re.shape:
        raise RuntimeError(f"istft: spectrum shape {tuple(re.shape)} does not match n_fft={n_fft}")
    wave = torch.empty(B, length, device=re.device, dtype=torch.float32)
    check(lib.cruse_istft_fwd(_p(re), _p(im), B, T, n_fft, hop, length, _p(wave), _stream()))
    return wave


def istft_bwd(dwave: torch.Tensor, T: int, n_fft: int, hop: int):
    B, L = dwave.shape
    F = n_fft // 2 + 1
    dre = torch.empty(B, T, F, device=dwave.device, dtype=torch.float32)
    dim = torch.empty(B, T, F, device=dwave.device, dtype=torch.float32)
    check(lib.cruse_istft_bwd(_p(dwave), B, T, n_fft, hop, L, _p(dre), _p(dim), _stream()))
    return dre, dim


# ---------------------------------------------------------------- convolutions
CONV_FORM_SUMS, CONV_FORM_BNB, CONV_FORM_BNI, CONV_FORM_BBI = 1, 2, 4, 8      # cruse_conv_plan
CONV_PREC = {"f32": PREC_F32, "bf16x3": PREC_BF16X3, "bf16": PREC_BF16X3, "valu": -1}


def conv_prec(prec) -> int:
    """MFMA precision used by the convolutions for a model precision mode: the convs are HBM-bound, so
    the bf16 mode runs them as split-bf16 x3 (~f32 accuracy) at no measurable cost."""
    if prec is None:
        return -1
    return CONV_PREC[prec] if isinstance(prec, str) else int(prec)


# The eight wrappers below are four forms times (gather, scatter2): one private function per form, the scatter2 wrapper being its gather
# twin called with scatter=True, S=2, Fout=2*Fg.  The C entry points of a pair differ in their argument lists only -- the scatter2 ones
# have no S and no w_layout -- which _geom / the `wl` tuples spell out.  _CONV_FN[scatter]: the pair members and their names in messages.
_CONV_FN = tuple((getattr(lib, f"cruse_conv_{n}"), getattr(lib, f"cruse_conv_{n}_bnbwd"), getattr(lib, f"cruse_conv_{n}_bnbwd_in"),
                  getattr(lib, f"cruse_conv_{n}_bnin"), getattr(lib, f"cruse_conv_{n}_bnstats"), f"conv_{n}", f"conv_{n} out",
                  f"conv_{n}_bwd_in out") for n in ("gather", "scatter2"))
_NO_SUMS = (None, 0)
_NO_BN_BWD = (None, None, None, None, None, False)


def _conv_out(like, B, T, Cout, Fout, bf16=False):
    return torch.empty(B, T, Cout, Fout, device=like.device, dtype=torch.bfloat16 if bf16 else torch.float32)


def _bn_sums(Cout, device):
    """(sums, zeroed) for the batch sums of a conv's Cout output channels"""
    return ARENA.take(2 * Cout * BN_STAT_REPLICAS, device)


def _bn_bwd_args(bn_bwd):
    by, mean, rstd, gamma, beta, relu = bn_bwd if bn_bwd is not None else _NO_BN_BWD
    return _p(by), _p(mean), _p(rstd), _p(gamma), _p(beta), 1 if relu else 0


def _geom(scatter, B, T, Cin, Fin, Cout, Fout, KT, S, pad):
    return (B, T, Cin, Fin, Cout, Fout, KT, pad) if scatter else (B, T, Cin, Fin, Cout, Fout, KT, S, pad)


def _conv(scatter, x, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, act, out, accum, prec, bn_bwd, out_bf16):
    fns = _CONV_FN[scatter]
    if out is None:
        out = _conv_out(x, B, T, Cout, Fout, out_bf16)
    geom, wl = _geom(scatter, B, T, Cin, Fin, Cout, Fout, KT, S, pad), () if scatter else (w_layout,)
    if bn_bwd is not None:
        sums, z = _bn_sums(Cout, x.device)
        check(fns[1](_p(x), _p(w), _p(out), *geom, *wl, 1 if accum else 0, conv_prec(prec), *_bn_bwd_args(bn_bwd), _p(sums), z,
                     _xdt(x, fns[5]), _xdt(out, fns[6]), _stream()))
        return out, sums
    check(fns[0](_p(x), _p(w), _p(bias), _p(out), *geom, *wl, act, 1 if accum else 0, conv_prec(prec), _xdt(x, fns[5]), _xdt(out, fns[6]),
                 _stream()))
    return out


def conv_gather(x, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout=0, act=0, out=None, accum=False,
                prec=None, bn_bwd=None, out_bf16=False):
    """bn_bwd = (bn_y, mean, rstd, gamma, beta, relu): the output is the gradient wrt the output of that BatchNorm(+ReLU); returns
    (out, sums) with the backward sums of bn_act_bwd accumulated by the conv's epilogue (cruse_conv_gather_bnbwd)."""
    return _conv(False, x, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, act, out, accum, prec, bn_bwd, out_bf16)


def conv_scatter2(g, w, bias, B, T, Cs, Fg, Cout, KT, pad, act=0, out=None, accum=False, prec=None, bn_bwd=None, out_bf16=False):
    """bn_bwd: as for conv_gather (cruse_conv_scatter2_bnbwd)."""
    return _conv(True, g, w, bias, B, T, Cs, Fg, Cout, 2 * Fg, KT, 2, pad, 0, act, out, accum, prec, bn_bwd, out_bf16)


def _bwd_in_args(dout, bn_in):
    y, mean, rstd, gamma, beta, sums, relu, training, dgamma, dbeta, dbias = bn_in
    dv = torch.empty(y.shape, device=y.device, dtype=torch.bfloat16)
    return dv, (_p(dout), _xdt(dout, "conv bnbwd_in dout"), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(sums), BN_STAT_REPLICAS,
                1 if relu else 0, 1 if training else 0, _p(dv), _p(dgamma), _p(dbeta), _p(dbias))


def _conv_bwd_in(scatter, dout, bn_in, w, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, out, accum, prec, bn_bwd, out_bf16):
    fns = _CONV_FN[scatter]
    if out is None:
        out = _conv_out(dout, B, T, Cout, Fout, out_bf16)
    dv, head = _bwd_in_args(dout, bn_in)
    sums, z = _bn_sums(Cout, dout.device) if bn_bwd is not None else _NO_SUMS
    check(fns[2](*head, _p(w), _p(out), *_geom(scatter, B, T, Cin, Fin, Cout, Fout, KT, S, pad), *(() if scatter else (w_layout,)),
                 1 if accum else 0, conv_prec(prec), *_bn_bwd_args(bn_bwd), _p(sums), z, _xdt(out, fns[7]), _stream()))
    return out, sums, dv


def conv_gather_bwd_in(dout, bn_in, w, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout=0, out=None, accum=False, prec=None, bn_bwd=None,
                       out_bf16=False):
    """Data gradient with the BatchNorm(+ReLU) backward of its INPUT fused into the staging (cruse_conv_gather_bnbwd_in).
    bn_in = (y_pre, mean, rstd, gamma, beta, sums [BN_STAT_REPLICAS][2*Cin], relu, training, dgamma, dbeta, dbias or None): `dout` is the gradient
    wrt that BatchNorm's output.  Returns (out, output-side sums or None, dy [B,T,Cin,Fin] bf16 -- the weight gradient's operand)."""
    return _conv_bwd_in(False, dout, bn_in, w, B, T, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, out, accum, prec, bn_bwd, out_bf16)


def conv_scatter2_bwd_in(dout, bn_in, w, B, T, Cs, Fg, Cout, KT, pad, out=None, accum=False, prec=None, bn_bwd=None, out_bf16=False):
    """As conv_gather_bwd_in for the stride-2 transposed form (cruse_conv_scatter2_bnbwd_in)."""
    return _conv_bwd_in(True, dout, bn_in, w, B, T, Cs, Fg, Cout, 2 * Fg, KT, 2, pad, 0, out, accum, prec, bn_bwd, out_bf16)


class BnIn:
    """The BatchNorm2d(train) + ReLU a forward conv applies to its INPUT while staging it (cruse_conv_*_bnin): `y_pre` the layer's
    pre-BN tensor, `sums` its batch sums [BN_STAT_REPLICAS][2C], gamma / beta, count = rows * F; mean / rstd (+ running statistics)
    are published by the ONE consumer that is handed them (publish=True); add: tensor added after the ReLU (the decoder's skip)."""

    def __init__(self, y_pre, sums, nrep, count, eps, momentum, gamma, beta, mean, rstd, running_mean=None, running_var=None, add=None):
        self.y_pre, self.sums, self.nrep, self.count, self.eps, self.momentum = y_pre, sums, nrep, count, eps, momentum
        self.gamma, self.beta, self.mean, self.rstd, self.rm, self.rv, self.add = gamma, beta, mean, rstd, running_mean, running_var, add

    def args(self, publish, copy_bf16):
        return (_p(self.y_pre), _p(self.sums), self.nrep, self.count, self.eps, self.momentum, _p(self.gamma), _p(self.beta),
                _p(self.mean) if publish else None, _p(self.rstd) if publish else None, _p(self.rm) if publish else None,
                _p(self.rv) if publish else None, _p(self.add), _p(copy_bf16))


def bnin_eligible(prec, Cin, Cout) -> bool:
    """shapes / modes cruse_conv_*_bnin takes: the MFMA forward convs of the bf16 mode"""
    # (the bf16 MODE: its forward convs run split-bf16 x3 and its weight gradients take the bf16 copies as they are)
    return (prec is not None and prec_code(prec) == PREC_BF16 and conv_prec(prec) == PREC_BF16X3 and 8 <= Cin <= 64
            and (Cin & (Cin - 1)) == 0 and 8 <= Cout <= 64)


def _conv_bnin(scatter, bn, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, prec, publish, copy_bf16, want_sums, out):
    if out is None:
        out = _conv_out(w, B, T, Cout, Fout)
    sums, z = _bn_sums(Cout, w.device) if want_sums else _NO_SUMS
    check(_CONV_FN[scatter][3](*bn.args(publish, copy_bf16), _p(w), _p(bias), _p(out), *_geom(scatter, B, T, Cin, Fin, Cout, Fout, KT, S, pad),
                               conv_prec(prec), _p(sums), z, _stream()))
    return (out, sums) if want_sums else out


def conv_gather_bnin(bn: BnIn, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, prec, publish=False, copy_bf16=None, want_sums=False,
                     out=None):
    """conv_gather on relu(bn(y_pre)) [+ add] without materialising it -> y, or (y, sums) with want_sums."""
    return _conv_bnin(False, bn, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, prec, publish, copy_bf16, want_sums, out)


def conv_scatter2_bnin(bn: BnIn, w, bias, B, T, Cs, Fg, Cout, KT, pad, prec, publish=False, copy_bf16=None, want_sums=False):
    return _conv_bnin(True, bn, w, bias, B, T, Cs, Fg, Cout, 2 * Fg, KT, 2, pad, prec, publish, copy_bf16, want_sums, None)


def _conv_bnstats(scatter, x, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, prec):
    out = _conv_out(x, B, T, Cout, Fout)
    sums, z = _bn_sums(Cout, x.device)
    check(_CONV_FN[scatter][4](_p(x), _p(w), _p(bias), _p(out), *_geom(scatter, B, T, Cin, Fin, Cout, Fout, KT, S, pad), conv_prec(prec),
                               _p(sums), z, _stream()))
    return out, sums


def conv_gather_bnstats(x, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, prec=None):
    """conv_gather + the BatchNorm batch sums of its output, accumulated by the conv's epilogue -> (y, sums)."""
    return _conv_bnstats(False, x, w, bias, B, T, Cin, Fin, Cout, Fout, KT, S, pad, prec)


def conv_scatter2_bnstats(g, w, bias, B, T, Cs, Fg, Cout, KT, pad, prec=None):
    return _conv_bnstats(True, g, w, bias, B, T, Cs, Fg, Cout, 2 * Fg, KT, 2, pad, prec)


def conv_plan(scatter, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, B, T, prec, x_dtype=0, y_dtype=0, act=0, accum=0, forms=0) -> dict:
    """what a frame-major convolution call launches (cruse_conv_plan; host-only): the route and its tile, grid and LDS bytes.  forms: bit set of
    CONV_FORM_SUMS / _BNB / _BNI / _BBI; with _BBI `fused` tells the fused kernel from the two-call fallback and x_dtype is that of dout."""
    out = (ctypes.c_int * 7)()
    check(lib.cruse_conv_plan(1 if scatter else 0, Cin, Fin, Cout, Fout, KT, S, pad, w_layout, B, T, conv_prec(prec), x_dtype, y_dtype, act,
                              1 if accum else 0, forms, ctypes.cast(out, ctypes.c_void_p)))
    return {"route": "mfma" if out[0] else "valu", "fused": bool(out[1]), "mt": out[2], "nw": out[3], "grid": out[4], "lds_bytes": out[5],
            "co_t": out[6]}


WGRAD_KERNELS = ("valu", "mfma", "rd")
WGRAD_REDUCES = (None, "wgrad_reduce", "wgrad_rd_reduce")


def conv_wgrad_plan(B, T, Ca, Fa, Cb, Fb, KT, S, pad, prec=None, a_dtype=0, bt_dtype=0, a_misalign=0, bt_misalign=0, ws_bytes=0) -> dict:
    """what a conv_wgrad call launches (cruse_conv_wgrad_plan; host-only): the kernel ("valu", "mfma" the LDS-staged one, "rd" the
    register-direct one), its template integers `t`, grid, block and LDS bytes, the partial slabs, the register-direct kernel's workgroups
    per slab and frames per slab, and the reduce kernel with its grid.  a_dtype / bt_dtype: DT_F32 / DT_BF16; a_misalign / bt_misalign:
    the operand addresses modulo 16; ws_bytes 0: the workspace conv_wgrad passes.  "raw" is the array as the library wrote it."""
    out = (ctypes.c_int * 14)()
    pc = -1 if prec is None else (WGRAD_PREC[prec] if isinstance(prec, str) else int(prec))
    check(lib.cruse_conv_wgrad_plan(B, T, Ca, Fa, Cb, Fb, KT, S, pad, pc, a_dtype, bt_dtype, a_misalign, bt_misalign, ws_bytes,
                                    ctypes.cast(out, ctypes.c_void_p)))
    return {"kernel": WGRAD_KERNELS[out[0]], "t": tuple(out[1:5]), "grid": out[5], "block": out[6], "lds_bytes": out[7], "slabs": out[8],
            "tg": out[9], "frames_per_slab": out[10], "reduce": WGRAD_REDUCES[out[11]], "reduce_grid": (out[12], out[13]), "raw": list(out)}


NCHW_REQ_BN_SUMS, NCHW_REQ_RESIDUAL, NCHW_REQ_BNBWD, NCHW_REQ_DB = 1, 2, 4, 1      # cruse_conv2d_nchw_plan
NCHW_CONV_FORMS = ("pw_tr_f16", "pw_mfma_f16", "pw", "dw_lds_f16", "dw", "general")
NCHW_WGRAD_FORMS = ("pw_mfma_f16", "dw_lds_f16", "dw", "rows", "weight")
NCHW_PASSES = (None, "add", "stats", "channel_sum")


def nchw_conv_plan(wgrad, B, Cin, Hin, Win, Cout, Hout, Wout, KH, KW, sh=1, sw=1, dh=1, dw=1, pt=0, pl=0, groups=1, up_w=1, transposed=0,
                   act=0, accumulate=0, dtype=0, requests=0) -> dict:
    """what an NCHW convolution (wgrad = 0) or weight-gradient (wgrad = 1: N, CA, HS, WS, CB, HB, WB) call launches (cruse_conv2d_nchw_plan;
    host-only): the kernel form, its template integers, grid, block and LDS bytes, which of the requests (bit set of NCHW_REQ_*) the kernel
    serves in its epilogue and the pass owed for the others.  "raw" is the array as the library wrote it."""
    out = (ctypes.c_int * 11)()
    check(lib.cruse_conv2d_nchw_plan(1 if wgrad else 0, B, Cin, Hin, Win, Cout, Hout, Wout, KH, KW, sh, sw, dh, dw, pt, pl, groups, up_w,
                                     1 if transposed else 0, act, 1 if accumulate else 0, dtype, requests, ctypes.cast(out, ctypes.c_void_p)))
    return {"form": (NCHW_WGRAD_FORMS if wgrad else NCHW_CONV_FORMS)[out[0]], "form_id": out[0], "t0": out[1], "t1": out[2], "grid": (out[3], out[4], out[5]),
            "block": out[6], "lds_bytes": out[7], "aux": out[8], "served": out[9], "pass": NCHW_PASSES[out[10]], "raw": list(out)}


_wgrad_ws = {}
_ws_retired = []          # outgrown workspaces: captured HIP graphs may still point at them, so they are never freed


def _ws(key, nbytes: int, device, zero: bool = True) -> torch.Tensor:
    """zero = False: a scratch whose user writes every byte it reads (weight-gradient / split-K slabs).  Those are keyed by STREAM, so a
    HIP-graph capture meets new keys -- and a torch.zeros made during capture is a fill NODE that replays with every step (round 6: eight
    5-15 us fills in the leaf chain of the captured step)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:       # "cuda" and "cuda:0" must name the same workspace
        device = torch.device("cuda", torch.cuda.current_device())
    buf = _wgrad_ws.get((key, device))
    if buf is None or buf.numel() < nbytes:
        old = buf
        # zero-filled: the GRU workspace starts with a STICKY 256-byte header (hand-off status word) that the library
        # never clears (include/cruse_hip.h, cruse_gru_seq_fwd); a grown buffer inherits the old header
        buf = (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device=device)
        if old is not None:
            _ws_retired.append((key, old))           # (graphs captured on the old buffer keep it alive)
        _wgrad_ws[(key, device)] = buf
    return buf


_gru_hdr: Dict[torch.device, torch.Tensor] = {}


def gru_header(device) -> torch.Tensor:
    """The STICKY 256-byte status header of the recurrence kernels (word 0: a hand-off timed out; bytes 64.. / 128..: the
    s_memtime stamps of the gru_dbg = 32 instances) -- ONE tensor per device for the life of the process, never regrown:
    HIP graphs captured before the panel scratch grew for a larger batch keep writing their time-outs where step_health and
    the guarded Adam look (the header used to be the first 256 bytes of the regrowable workspace)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    h = _gru_hdr.get(device)
    if h is None:
        h = _gru_hdr[device] = torch.zeros(256, dtype=torch.uint8, device=device)
    return h


WGRAD_PREC = {"f32": PREC_F32, "bf16x3": PREC_BF16X3, "bf16": PREC_BF16, "valu": -1}


def conv_wgrad(a, bt, dw, B, T, Ca, Fa, Cb, Fb, KT, S, pad, prec=None):
    """dw[ca][cb][kt][kf] += ... (dw is a contiguous f32 tensor of Ca*Cb*KT*3 elements)."""
    nbytes = lib.cruse_conv_wgrad_ws_bytes(Ca, Cb, KT)
    # one partial-slab workspace PER STREAM: weight-gradient leaves may run concurrently on several side streams
    ws = _ws(("wgrad", _stream()), nbytes, a.device, zero=False)
    pc = -1 if prec is None else (WGRAD_PREC[prec] if isinstance(prec, str) else int(prec))
    check(lib.cruse_conv_wgrad(_p(a), _p(bt), _p(dw), B, T, Ca, Fa, Cb, Fb, KT, S, pad, pc, _xdt(a, "conv_wgrad a"),
                               _xdt(bt, "conv_wgrad bt"), _p(ws), _stream()))


def upsample_w(x, rows, W, up=2):
    """nearest FreqUpsample along the last axis (cust_conv.py:177-184): x [rows, W] f32 -> [rows, W * up]"""
    _f32(x, "upsample_w")
    out = torch.empty(rows, W * up, device=x.device, dtype=torch.float32)
    check(lib.cruse_upsample_w(_p(x), rows, W, up, _p(out), 0, _stream()))
    return out


def downsum_w(dxu, rows, W, up=2):
    """its gradient: [rows, W * up] f32 -> [rows, W] (sums of `up` neighbours)"""
    _f32(dxu, "downsum_w")
    out = torch.empty(rows, W, device=dxu.device, dtype=torch.float32)
    check(lib.cruse_downsum_w(_p(dxu), rows, W, up, _p(out), 0, _stream()))
    return out


def channel_sum(g, rows, C, F, out):
    check(lib.cruse_channel_sum(_p(g), rows, C, F, _p(out), _stream()))


def col_sum(g, g_off, rows, ncol, ld, out):
    check(lib.cruse_col_sum(g.data_ptr() + 4 * g_off, rows, ncol, ld, _p(out), _stream()))


# ---------------------------------------------------------------- zeroed scratch for the step's reductions
class _ZeroArena:
    """f64 accumulators for the reductions of ONE training step (BatchNorm batch sums, backward sums, loss sums), carved
    from one buffer that a single cruse_zero clears at the top of the step -- instead of one memset launch in front of
    every reduction kernel (15 launches per step).  Inactive outside `with ARENA.step(device):` -- callers then get a
    fresh tensor and the kernel clears it itself.  Under HIP-graph capture the slices are handed out in the same order on
    every capture, so the captured pointers stay valid."""

    CAP = 1 << 14           # doubles (128 KiB)

    def __init__(self):
        self.bufs = {}
        self.active = None
        self.off = 0

    def step(self, device):
        arena = self

        class _Ctx:
            def __enter__(self_):
                dev = torch.device(device)
                buf = arena.bufs.get(dev)
                if buf is None:
                    buf = arena.bufs[dev] = torch.zeros(arena.CAP, device=dev, dtype=torch.float64)
                arena.active, arena.off = buf, 0
                zero_(buf)
                return arena

            def __exit__(self_, *exc):
                arena.active = None
        return _Ctx()

    def take(self, n: int, device):
        """-> (f64 tensor of n elements, zeroed flag)."""
        if self.active is None or self.active.device != device or self.off + n > self.CAP:
            return torch.empty(n, device=device, dtype=torch.float64), 0
        t = self.active[self.off:self.off + n]
        self.off += (n + 1) // 2 * 2                    # keep 16-byte alignment
        return t, 1


ARENA = _ZeroArena()


# ---------------------------------------------------------------- BatchNorm
def bn_stats(y, rows, C, F):
    sums, z = ARENA.take(2 * C, y.device)
    check(lib.cruse_bn_stats(_p(y), rows, C, F, _p(sums), z, _stream()))
    return sums


BN_STAT_REPLICAS = 16      # CRUSE_BN_STAT_REPLICAS (include/cruse_hip.h): layout of the sums of conv_*_bnstats


def bn_finalize_act_fwd(y, sums, count, eps, momentum, gamma, beta, skip, rows, C, F, relu=True, running_mean=None,
                        running_var=None, out_bf16=None):
    """bn_finalize + bn_act_fwd in one launch -> (out, mean, rstd).  sums: [2*C] (bn_stats) or [replicas, 2*C]
    (conv_*_bnstats); the statistic is the sum over the replicas."""
    if sums.numel() % (2 * C) != 0:
        raise RuntimeError(f"bn_finalize_act_fwd: {sums.numel()} sums for {C} channels")
    out = torch.empty_like(y)
    mean = torch.empty(C, device=y.device, dtype=torch.float32)
    rstd = torch.empty(C, device=y.device, dtype=torch.float32)
    if out_bf16 is not None and (out_bf16.dtype not in (torch.bfloat16, torch.float16) or out_bf16.numel() < y.numel()):
        raise RuntimeError("bn_finalize_act_fwd: out_bf16 must be a bf16 (or f16) tensor of at least y.numel() elements")
    # (the operand copy takes the element type of the tensor handed in: bf16, or f16 for the single-pass f16 gate projection)
    check(lib.cruse_bn_finalize_act_fwd_c(_p(y), _p(sums), sums.numel() // (2 * C), count, eps, momentum, _p(gamma), _p(beta), _p(skip), _p(out),
                                          _p(out_bf16), _copy_dt(out_bf16), _p(mean), _p(rstd), _p(running_mean), _p(running_var), rows, C, F,
                                          1 if relu else 0, _stream()))
    return out, mean, rstd


def bn_finalize(sums, count, C, eps, momentum, running_mean=None, running_var=None):
    mean = torch.empty(C, device=sums.device, dtype=torch.float32)
    rstd = torch.empty(C, device=sums.device, dtype=torch.float32)
    check(lib.cruse_bn_finalize(_p(sums), count, C, eps, momentum, _p(mean), _p(rstd), _p(running_mean),
                                _p(running_var), _stream()))
    return mean, rstd


def bn_eval_stats(running_mean, running_var, eps):
    C = running_mean.numel()
    mean = torch.empty(C, device=running_mean.device, dtype=torch.float32)
    rstd = torch.empty(C, device=running_mean.device, dtype=torch.float32)
    check(lib.cruse_bn_eval_stats(_p(running_mean), _p(running_var), C, eps, _p(mean), _p(rstd), _stream()))
    return mean, rstd


def bn_act_fwd(y, mean, rstd, gamma, beta, skip, rows, C, F, relu=True):
    out = torch.empty_like(y)
    check(lib.cruse_bn_act_fwd(_p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(skip), _p(out), rows, C, F,
                               1 if relu else 0, _stream()))
    return out


def bn_act_bwd(dout, y, mean, rstd, gamma, beta, rows, C, F, relu, training, dgamma, dbeta, dbias=None, sums=None,
               out_bf16=False):
    """sums: the backward sums the convolution that produced dout has already accumulated (conv_gather / conv_scatter2 with
    bn_bwd: [BN_STAT_REPLICAS][2*C]); None: the reduce pass runs here.  out_bf16: dy as a bf16 tensor (its consumers -- the
    data-gradient conv and the weight gradient of the bf16 mode -- round it to bf16 operands anyway: the same bits, half the
    bytes written once and read twice)."""
    nrep = BN_STAT_REPLICAS
    if sums is None:
        nrep = 1
        sums, z = ARENA.take(2 * C, y.device)
        _f32(dout, "bn_act_bwd (reduce pass) dout")       # (a bf16 gradient arrives with its sums from the conv that stored it)
        check(lib.cruse_bn_act_bwd_reduce(_p(dout), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), rows, C, F,
                                          1 if relu else 0, _p(sums), z, _stream()))
    dy = torch.empty_like(y, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    check(lib.cruse_bn_act_bwd_apply(_p(dout), _p(y), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(sums), nrep, rows, C, F,
                                     1 if relu else 0, 1 if training else 0, _xdt(dout, "bn_act_bwd dout"), _p(dy), 2 if out_bf16 else 0,
                                     _p(dgamma), _p(dbeta),
                                     _p(dbias), _stream()))
    return dy


def _copy_dt(t) -> int:
    """CRUSE_DT_* of a 2-byte operand copy (CRUSE_DT_F16 = 1, CRUSE_DT_BF16 = 2; None: bf16)"""
    return 1 if (t is not None and t.dtype == torch.float16) else 2


# ---------------------------------------------------------------- LayerNorm
def ln_fwd(x, gamma, beta, res, rows, H, interleave_g=1, eps=1e-5, save=True, out=None, out_bf16=None, seg=None, stats=None):
    """seg = (seg_len, seg_stride, seg_off): only the rows of one time chunk (cruse_ln_fwd row segments; rows = B * seg_len),
    into the full-size out / out_bf16 / stats = (mean, rstd) of the call that owns them."""
    y = torch.empty_like(x) if out is None else out
    if stats is not None:
        mean, rstd = stats
    else:
        nstat = x.numel() // H
        mean = torch.empty(nstat, device=x.device, dtype=torch.float32) if save else None
        rstd = torch.empty(nstat, device=x.device, dtype=torch.float32) if save else None
    sl, ss, so = seg if seg is not None else (0, 0, 0)
    if out_bf16 is not None and (out_bf16.dtype not in (torch.bfloat16, torch.float16) or out_bf16.numel() < x.numel()):
        raise RuntimeError("ln_fwd: out_bf16 must be a bf16 (or f16) tensor of at least x.numel() elements")
    check(lib.cruse_ln_fwd_c(_p(x), _p(gamma), _p(beta), _p(res), _p(y), _p(out_bf16), _copy_dt(out_bf16), _p(mean), _p(rstd), rows, H,
                             interleave_g, eps, sl, ss, so, _stream()))
    return y, mean, rstd


def ln_bwd(dy, x, mean, rstd, gamma, rows, H, interleave_g, dgamma, dbeta):
    dx = torch.empty_like(x)
    check(lib.cruse_ln_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), rows, H, interleave_g, _p(dx), _p(dgamma),
                           _p(dbeta), _stream()))
    return dx


# ---------------------------------------------------------------- GEMM
def gemm(transA, transB, M, N, K, A, a_off, lda, Bm, b_off, ldb, C, c_off, ldc, bias=None, accumulate=False,
         splitk=1, b_shift_T=0, prec=PREC_F32):
    """Raw-pointer GEMM; *_off are element offsets into the tensors' storage views."""
    pa = A.data_ptr() + 4 * a_off
    pb = Bm.data_ptr() + 4 * b_off
    pc = C.data_ptr() + 4 * c_off
    check(lib.cruse_gemm(1 if transA else 0, 1 if transB else 0, M, N, K, pa, lda, pb, ldb, pc, ldc, _p(bias),
                         1 if accumulate else 0, splitk, b_shift_T, prec_code(prec), _stream()))


def gemm_bf16_nt(M, N, K, A, a_off, lda, Bm, b_off, ldb, C, c_off, ldc, bias=None, accumulate=False, splitk=1,
                 a_kstride=64, b_kstride=64, slabs=False):
    """C[M,N] (+)= A[M,K] . B[N,K]^T on bf16 operands (element offsets into the tensors' storage).
    *_kstride == 64: row-major operand; larger: the K-tiled time-major layout (lda == 64), see cruse_hip.h.
    slabs (split-K, accumulate): the k-slices store partial sums to a per-stream scratch that one kernel adds to C in slice order
    -- no atomics (cruse_gemm_bf16_nt_slabs)."""
    if slabs and accumulate and bias is None and abs(splitk) > 1 and N % 4 == 0 and C.dtype == torch.float32:
        if A.dtype != torch.bfloat16 or Bm.dtype != torch.bfloat16:
            raise RuntimeError("gemm_bf16_nt needs bf16 operands")
        nbytes = lib.cruse_gemm_bf16_slab_bytes(M, N, splitk)
        ws = _ws(("gemm_slabs", _stream()), nbytes, C.device, zero=False)
        check(lib.cruse_gemm_bf16_nt_slabs(M, N, K, _at(A, a_off), lda, a_kstride, _at(Bm, b_off), ldb, b_kstride,
                                           _at(C, c_off, 4), ldc, splitk, _p(ws), ws.numel(), _stream()))
        return
    if C.dtype in _OUT16 and A.dtype == torch.bfloat16 and Bm.dtype == torch.bfloat16 and not accumulate and abs(splitk) <= 1:
        return _gemm_nt_out16(M, N, K, A, None, a_off, lda, a_kstride, Bm, None, b_off, ldb, b_kstride, C, c_off, ldc, bias, False)
    if A.dtype != torch.bfloat16 or Bm.dtype != torch.bfloat16 or C.dtype != torch.float32:
        raise RuntimeError("gemm_bf16_nt needs bf16 operands and an f32 result")
    check(lib.cruse_gemm_bf16_nt(M, N, K, _at(A, a_off), lda, a_kstride, _at(Bm, b_off), ldb, b_kstride,
                                 _at(C, c_off, 4), ldc, _p(bias), 1 if accumulate else 0, splitk, _stream()))


def gemm_bf16_nt_cat(Ms, N, K, A, a_rows, lda, Bs, b_off, ldb, C, c_off, ldc, splitk, a_kstride=64, b_kstride=64):
    """C[sum Ms, N] += cat_i(A[a_rows[i] : a_rows[i] + Ms[i]] . Bs[i]^T): up to three split-K slab products in ONE launch
    (cruse_gemm_bf16_nt_slabs_cat; a_rows in rows of A, b_off / c_off in elements)."""
    n = len(Ms)
    if A.dtype != torch.bfloat16 or any(b.dtype != torch.bfloat16 for b in Bs) or C.dtype != torch.float32:
        raise RuntimeError("gemm_bf16_nt_cat needs bf16 operands and an f32 result")
    nbytes = lib.cruse_gemm_bf16_slab_bytes(int(sum(Ms)), N, splitk)
    ws = _ws(("gemm_slabs", _stream()), nbytes, C.device, zero=False)
    ms = (ctypes.c_int * n)(*[int(m) for m in Ms])
    ar = (ctypes.c_longlong * n)(*[int(r) for r in a_rows])
    bs = (ctypes.c_void_p * n)(*[_at(b, b_off) for b in Bs])
    check(lib.cruse_gemm_bf16_nt_slabs_cat(n, ctypes.cast(ms, ctypes.c_void_p), N, K, A.data_ptr(), ctypes.cast(ar, ctypes.c_void_p), lda, a_kstride,
                                           ctypes.cast(bs, ctypes.c_void_p), ldb, b_kstride, _at(C, c_off, 4), ldc, splitk, _p(ws),
                                           ws.numel(), _stream()))


def gemm_bf16_nt_atr(M, N, K, A_T, a_off, a_mb_stride, n_mb, Bm, b_off, ldb, C, c_off, ldc, accumulate=False, b_kstride=64):
    """C[M,N] (+)= A . B^T with A read from its time-major K-tiled image (element (m, k) at A_T[a_off + (m // 64) * a_mb_stride + k * 64 + m % 64]):
    cruse_gemm_bf16_nt_atr -- dX straight from the gate-gradient tensor dgT, no row-major dgi."""
    if A_T.dtype != torch.bfloat16 or Bm.dtype != torch.bfloat16 or C.dtype != torch.float32:
        raise RuntimeError("gemm_bf16_nt_atr needs bf16 operands and an f32 result")
    check(lib.cruse_gemm_bf16_nt_atr(M, N, K, _at(A_T, a_off), a_mb_stride, n_mb, _at(Bm, b_off), ldb, b_kstride,
                                     _at(C, c_off, 4), ldc, 1 if accumulate else 0, _stream()))
    return C


def gemm_bf16_nt_groups(M, N, K, G, A_hi, A_lo, lda, a_gstep, B_hi, B_lo, ldb, b_gstep, C, ldc, c_gstep, bias=None, bias_gstep=0,
                        accumulate=False, b_kstride=64):
    """G equal-shape products side by side along N in one launch (cruse_gemm_bf16_nt_groups): the GRU groups of a layer.
    bias: the first group's bias tensor (the others bias_gstep floats apart)."""
    for t_ in (A_hi, A_lo, B_hi, B_lo):
        if t_ is not None and t_.dtype != torch.bfloat16:
            raise RuntimeError("gemm_bf16_nt_groups needs bf16 planes")
    if C.dtype != torch.float32:
        raise RuntimeError("gemm_bf16_nt_groups: f32 result")
    check(lib.cruse_gemm_bf16_nt_groups(M, N, K, G, _p(A_hi), _p(A_lo), lda, a_gstep, _p(B_hi), _p(B_lo), ldb, b_kstride, b_gstep,
                                        _p(C), ldc, c_gstep, _p(bias), bias_gstep, 1 if accumulate else 0, _stream()))
    return C


def uniform_stride(tensors) -> Optional[int]:
    """element stride between equally shaped f32 tensors if it is the same for all consecutive pairs (the per-group parameters in the flat
    buffer), else None"""
    if len(tensors) < 2:
        return 0
    d = [tensors[i + 1].data_ptr() - tensors[i].data_ptr() for i in range(len(tensors) - 1)]
    if any(x != d[0] for x in d) or d[0] <= 0 or d[0] % 4:
        return None
    return d[0] // 4


def gemm_bf16_nt_seg(M, N, K, A_hi, A_lo, a_off, lda, B_hi, B_lo, b_off, ldb, C, c_off, ldc, seg, bias=None, accumulate=False,
                     b_kstride=64):
    """gemm_bf16_nt / gemm_bf16x3_nt (A_lo / B_lo None: plain bf16) on the rows of ONE TIME CHUNK: seg = (seg_len, seg_stride,
    seg_off), M = B * seg_len (cruse_gemm_bf16_nt_seg)."""
    check(lib.cruse_gemm_bf16_nt_seg(M, N, K, _at(A_hi, a_off), _at(A_lo, a_off), lda, _at(B_hi, b_off),
                                     _at(B_lo, b_off), ldb, b_kstride, _at(C, c_off, 4), ldc, _p(bias),
                                     1 if accumulate else 0, seg[0], seg[1], seg[2], _stream()))


def cast_bf16(x, out=None):
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16) if out is None else out
    check(lib.cruse_cast_bf16(_p(x), _p(y), x.numel(), _stream()))
    return y


def ktile_bf16(x, rows, cols, split=False, out=None):
    """x [rows, cols] f32 -> K-tiled bf16 [ceil(cols/64), rows, 64] (k = column index, zero padded): no transposition.
    split: returns (hi, lo) planes with x ~= hi + lo.  out = (y, lo or None): write into these."""
    if out is not None:
        y, lo = out
    else:
        y = torch.empty((cols + 63) // 64, rows, 64, device=x.device, dtype=torch.bfloat16)
        lo = torch.empty_like(y) if split else None
    check(lib.cruse_ktile_bf16(_p(x), rows, cols, cols, _p(y), _p(lo), _stream()))
    return (y, lo) if split else y


def ktile_f16(x, rows, cols, split=False):
    """x [rows, cols] f32 -> K-tiled IEEE f16 [ceil(cols/64), rows, 64] (the layout of ktile_bf16): the B operand of gemm_f16_nt.
    split: returns (hi, lo) with lo = f16(x - hi) (cruse_ktile_f16_split): the planes of gemm_f16_nt(B_lo=...)"""
    y = torch.empty((cols + 63) // 64, rows, 64, device=x.device, dtype=torch.float16)
    if split:
        lo = torch.empty_like(y)
        check(lib.cruse_ktile_f16_split(_p(x), rows, cols, cols, _p(y), _p(lo), _stream()))
        return y, lo
    check(lib.cruse_ktile_f16(_p(x), rows, cols, cols, _p(y), _stream()))
    return y


_OUT16 = {torch.float16: 1, torch.bfloat16: 2}        # CRUSE_DT_F16 / CRUSE_DT_BF16


def _gemm_nt_out16(M, N, K, A_hi, A_lo, a_off, lda, a_kstride, B_hi, B_lo, b_off, ldb, b_kstride, C, c_off, ldc, bias, operands_f16):
    """2-byte result rows (cruse_gemm_nt_out16): C is an f16 / bf16 tensor -- the gi rows gru_seq_fwd reads in that dtype"""
    check(lib.cruse_gemm_nt_out16(M, N, K, _at(A_hi, a_off), _at(A_lo, a_off), lda, a_kstride, _at(B_hi, b_off), _at(B_lo, b_off), ldb, b_kstride,
                                  _at(C, c_off), ldc, _p(bias), 1 if operands_f16 else 0, _OUT16[C.dtype], _stream()))
    return C


def gemm_f16_nt(M, N, K, A, a_off, lda, B, b_off, ldb, C, c_off, ldc, bias=None, a_kstride=64, b_kstride=64, B_lo=None):
    """C[M,N] = A[M,K] . B[N,K]^T + bias on IEEE-f16 operands (cruse_gemm_f16_nt; offsets in elements): the forward gate projection
    in one pass.  B_lo: the low plane of B (ktile_f16(split=True)) -- two passes on the same accumulators (cruse_gemm_f16x2_nt)."""
    if A.dtype != torch.float16 or B.dtype != torch.float16 or (B_lo is not None and B_lo.dtype != torch.float16):
        raise RuntimeError("gemm_f16_nt needs f16 operands")
    if C.dtype in _OUT16:
        return _gemm_nt_out16(M, N, K, A, None, a_off, lda, a_kstride, B, B_lo, b_off, ldb, b_kstride, C, c_off, ldc, bias, True)
    if C.dtype != torch.float32:
        raise RuntimeError("gemm_f16_nt: the result is f32, or f16 / bf16 rows (cruse_gemm_nt_out16)")
    if B_lo is not None:
        check(lib.cruse_gemm_f16x2_nt(M, N, K, _at(A, a_off), lda, a_kstride, _at(B, b_off), _at(B_lo, b_off), ldb,
                                      b_kstride, _at(C, c_off, 4), ldc, _p(bias), _stream()))
        return C
    check(lib.cruse_gemm_f16_nt(M, N, K, _at(A, a_off), lda, a_kstride, _at(B, b_off), ldb, b_kstride,
                                _at(C, c_off, 4), ldc, _p(bias), _stream()))
    return C


def cast_bf16_padded(x, pad=64, split=False):
    """bf16 copy of x followed by `pad` zero elements, so a GEMM whose K is rounded up to 64 may read past the last row.
    split: returns (hi, lo) planes with x ~= hi + lo (both padded)."""
    n = x.numel()
    buf = torch.empty(n + pad, device=x.device, dtype=torch.bfloat16)
    lo = torch.empty(n + pad, device=x.device, dtype=torch.bfloat16) if split else None
    if pad:
        buf[n:].zero_()
        if split:
            lo[n:].zero_()
    check(lib.cruse_cast_bf16_split(_p(x), _p(buf), _p(lo), n, _stream()))
    return (buf, lo) if split else buf


def gemm_bf16x3_nt(M, N, K, A_hi, A_lo, a_off, lda, B_hi, B_lo, b_off, ldb, C, c_off, ldc, bias=None, accumulate=False,
                   a_kstride=64, b_kstride=64):
    """Split-bf16 form of gemm_bf16_nt: (A_hi + A_lo) . (B_hi + B_lo)^T without the lo.lo term; A_lo = None drops
    the A_lo.B_hi term too (two passes: only B's rounding is corrected)."""
    for t_ in (A_hi, A_lo, B_hi, B_lo):
        if t_ is not None and t_.dtype != torch.bfloat16:
            raise RuntimeError("gemm_bf16x3_nt needs bf16 planes")
    if C.dtype in _OUT16 and not accumulate:
        return _gemm_nt_out16(M, N, K, A_hi, A_lo, a_off, lda, a_kstride, B_hi, B_lo, b_off, ldb, b_kstride, C, c_off, ldc, bias, False)
    if C.dtype != torch.float32:
        raise RuntimeError("gemm_bf16x3_nt needs an f32 result (f16 / bf16 rows without accumulation: cruse_gemm_nt_out16)")
    check(lib.cruse_gemm_bf16x3_nt(M, N, K, _at(A_hi, a_off), _at(A_lo, a_off), lda, a_kstride, _at(B_hi, b_off), _at(B_lo, b_off), ldb, b_kstride,
                                   _at(C, c_off, 4), ldc, _p(bias), 1 if accumulate else 0, _stream()))


GEMM_FORMS = ("plain", "x3", "f16", "f16x2", "out16", "atr", "groups", "slabs", "slabs_cat", "seg")       # CRUSE_GEMM_FORM_*
GEMM_PLANE_A_LO, GEMM_PLANE_B_LO, GEMM_PLANES_UNALIGNED = 1, 2, 4
_GEMM_PLAN_KEYS = ("mode", "nst", "f16", "atr", "grid", "lds_bytes", "splitk", "kt_chunk", "xcdk", "tiles_m", "tiles_n", "nunits", "inner", "m_out",
                   "slab", "reduce_grid")


def gemm_bf16_plan(form, M, N, K, lda, a_kstride, ldb, b_kstride, ldc, planes=0, bias=False, accumulate=False, splitk=1, operands_f16=False,
                   out_dtype=0, extras=()) -> dict:
    """what a call of the bf16 / f16 GEMM entry points launches (cruse_gemm_bf16_plan; host-only): the kernel (mode, stages, f16, atr), its grid and
    LDS bytes and the tile geometry.  form: one of GEMM_FORMS, the entry point whose checks run first; planes: bit set of GEMM_PLANE_*; extras: the
    form's own numbers (cruse_hip.h) -- atr (a_mb_stride, n_mb), groups (G, a_gstep, b_gstep, c_gstep, bias_gstep), slabs (scratch_bytes),
    slabs_cat (scratch_bytes, nprob, Ms[3], a_rows[3]), seg (seg_len, seg_stride, seg_off).  "raw" is the array as the library wrote it."""
    out = (ctypes.c_int * len(_GEMM_PLAN_KEYS))()
    x = (ctypes.c_longlong * max(len(extras), 8))(*[int(v) for v in extras])
    check(lib.cruse_gemm_bf16_plan(GEMM_FORMS.index(form), M, N, K, lda, a_kstride, ldb, b_kstride, ldc, planes, 1 if bias else 0,
                                   1 if accumulate else 0, splitk, 1 if operands_f16 else 0, out_dtype, ctypes.cast(x, ctypes.c_void_p),
                                   ctypes.cast(out, ctypes.c_void_p)))
    return dict(zip(_GEMM_PLAN_KEYS, out), raw=list(out))


def transpose_bf16(x, rows, cols, shift_T=0, out=None):
    """x [rows, cols] f32 -> K-tiled time-major bf16 [ceil(rows/64), cols, 64] (zero-padded frames);
    shift_T > 0 reads row r-1 within each clip."""
    ldT = (rows + 63) // 64 * 64
    y = torch.empty(ldT // 64, cols, 64, device=x.device, dtype=torch.bfloat16) if out is None else out
    check(lib.cruse_transpose_bf16(_p(x), rows, cols, cols, _p(y), ldT, shift_T, _stream()))
    return y


# ---------------------------------------------------------------- GRU recurrence
def _ptr_array(ts: Sequence[torch.Tensor]):
    arr = (ctypes.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = _p(t)
    return arr


STEP_SLOT0 = 100            # slots STEP_SLOT0 .. +STEP_SLOTS-1: the scratches gru_step_ws_clear() clears with ONE launch
STEP_SLOTS = 4


def _gru_ws(B, G, Hg, dev, slot: int):
    """-> (panel scratch pointer, status word pointer).  slot 0 is the library's classic workspace (sticky header +
    panels); slots > 0 -- concurrent recurrences on other streams -- get their own panel scratch and share slot 0's
    status word, so one word still guards the optimizer step.  Slots STEP_SLOT0.. are carved from one buffer
    (gru_step_ws_clear)."""
    nbytes = lib.cruse_gru_ws_bytes(B, G, Hg)
    status = gru_header(dev).data_ptr()
    if slot == 0:
        return _ws("gru", nbytes, dev).data_ptr() + 256, status
    if STEP_SLOT0 <= slot < STEP_SLOT0 + STEP_SLOTS:
        per = (nbytes - 256 + 255) // 256 * 256
        buf = _ws(("gru_step", per), per * STEP_SLOTS, dev)
        return buf.data_ptr() + (slot - STEP_SLOT0) * per, status
    panels = _ws(("gru_panels", slot), nbytes - 256, dev)
    return panels.data_ptr(), status


def gru_step_ws_clear(B, G, Hg, dev) -> None:
    """One launch clears the panel scratches of slots STEP_SLOT0 .. STEP_SLOT0 + STEP_SLOTS - 1: the (up to) four recurrences of
    a training step then run with zeroed=True -- no memset launch in front of each (4 x ~14 us on the main stream)."""
    nbytes = lib.cruse_gru_ws_bytes(B, G, Hg)
    per = (nbytes - 256 + 255) // 256 * 256
    zero_(_ws(("gru_step", per), per * STEP_SLOTS, torch.device(dev)))


def _off(t: torch.Tensor, elems: int) -> int:
    return t.data_ptr() + elems * t.element_size()


def gru_seq_fwd(gi, w_hh: List[torch.Tensor], b_hh: List[torch.Tensor], B, T, G, Hg, prec, save=True, slot=0, xcd_rot=0,
                h0=None, out=None, chunk=None, wide=False, zeroed=False):
    """-> (h, coef, an, z); the last three are None when save is False (inference).  slot / xcd_rot: see
    cruse_gru_seq_fwd_on (concurrent recurrences).
    h0 [B, G*Hg] ("cat" layout: feature = group*Hg + unit): initial state (cust_conv.py:305-325); None = 0.
    chunk = (t0, n): run only frames [t0, t0+n) of the [B,T] tensors into `out` = (h, coef, an, z) from the call that ran
    the frames before them -- the initial state is then h[:, t0-1] (h0 for t0 == 0).  Consecutive chunks reproduce the
    single launch (cruse_gru_seq_fwd_ex; bit for bit in f32 / bf16x3 and against launches given an h0 -- not bf16 at Hg 160 / 320 against h0 = None, see there).  wide: chains of 16 clips (half the workgroups; same results).
    zeroed: the slot's scratch is already clear
    (gru_step_ws_clear)."""
    if gi.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"gru_seq_fwd: gi must be f32 (or f16 rows: cruse_gru_seq_fwd_gi16), got {gi.dtype}")
    if gi.dtype == torch.float16 and (h0 is not None or chunk is not None or wide):
        raise RuntimeError("gru_seq_fwd: f16 gi rows are served for whole sequences from h0 = 0 on chains of 8 clips")
    dev = gi.device
    H = G * Hg
    if out is not None:
        h, coef, an, z = out
    else:
        h = torch.empty(B, T, H, device=dev, dtype=torch.float32)
        if save:
            cdt = torch.bfloat16 if prec_code(prec) == PREC_BF16 else torch.float32
            coef = torch.empty(B, T, 3 * H, device=dev, dtype=cdt)
            an = torch.empty_like(h); z = torch.empty_like(h)
        else:
            coef = an = z = None
    t0, n = chunk if chunk is not None else (0, T)
    if not (0 <= t0 and n > 0 and t0 + n <= T):
        raise RuntimeError(f"gru_seq_fwd: chunk ({t0}, {n}) outside [0, {T})")
    h0p, h0s = None, 0
    if t0 > 0:
        h0p, h0s = _off(h, (t0 - 1) * H), T * H
    elif h0 is not None:
        if wide:
            raise RuntimeError("gru_seq_fwd: wide chains take no caller-supplied h0 (their hand-off needs |h| < 1); chunk "
                               "continuations are fine")
        if tuple(h0.shape) != (B, H) or h0.dtype != torch.float32:
            raise RuntimeError(f"gru_seq_fwd: h0 must be f32 [{B}, {H}], got {tuple(h0.shape)}")
        _p(h0)
        h0p, h0s = h0.data_ptr(), H
    panels, status = _gru_ws(B, G, Hg, dev, slot)
    wa, ba = _ptr_array(w_hh), _ptr_array(b_hh)
    _p(gi); _p(h); _p(coef); _p(an); _p(z)
    opt = lambda t_, k: None if t_ is None else _off(t_, t0 * k)
    if gi.dtype == torch.float16:
        check(lib.cruse_gru_seq_fwd_gi16(gi.data_ptr(), 1, ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ba, ctypes.c_void_p), h.data_ptr(),
                                         None if coef is None else coef.data_ptr(), None if an is None else an.data_ptr(),
                                         None if z is None else z.data_ptr(), B, T, T, G, Hg, prec_code(prec), panels, 1 if zeroed else 0,
                                         status, xcd_rot, _stream()))
        return h, coef, an, z
    check(lib.cruse_gru_seq_fwd_ex(_off(gi, t0 * 3 * H), ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ba, ctypes.c_void_p),
                                   _off(h, t0 * H), opt(coef, 3 * H), opt(an, H), opt(z, H), h0p, h0s, B, n, T, G, Hg,
                                   prec_code(prec), 16 if wide else 0, panels, 1 if zeroed else 0,
                                   status, xcd_rot, _stream()))
    return h, coef, an, z


def dgi_buffer(rows, G, Hg, device, slabs=3):
    """bf16 [rows, G, slabs, Hg] gate-gradient rows (slabs 3: r, z, n_i; 4: + n_h, see cruse_gru_seq_bwd_ex), followed by the
    zero K-padding the dX GEMM may read (K = 3*Hg rounded to 64; with 4 slabs the run-over lands in the n_h slab)."""
    n = rows * G * slabs * Hg
    pad = 64 if ((3 * Hg) % 64 and slabs == 3) else 0
    buf = torch.empty(n + pad, device=device, dtype=torch.bfloat16)
    if pad:
        buf[n:].zero_()
    return buf[:n].view(rows, G, slabs, Hg)


def gru_seq_bwd(dout, w_hh: List[torch.Tensor], coef, z, B, T, G, Hg, prec, slot=0, xcd_rot=0, an=None, want_dgi=False,
                out=None, chunk=None, dg_slabs=3, wide=False, zeroed=False):
    """dout [B,T,H] -> dh [B,T,H] (total gradient reaching every h_t).  want_dgi (CRUSE_PREC_BF16, with the a_n rows):
    -> (dh, dgi) with dgi = dh * (c_r, c_z, a_n) in bf16 written by the recurrence itself (cruse_gru_seq_bwd_on).
    chunk = (t0, n): only frames [t0, t0+n), into out = dh (or (dh, dgi)); chunks are run from the LAST to the first, and
    every chunk but the last picks the gradient carried across its end up from dh[:, t0+n] (cruse_gru_seq_bwd_ex)."""
    H = G * Hg
    dgi = None
    if out is not None:
        dh, dgi = out if want_dgi else (out, None)
    else:
        dh = torch.empty_like(dout)
        if want_dgi:
            dgi = dgi_buffer(B * T, G, Hg, dout.device, dg_slabs)
    if want_dgi and (an is None or prec_code(prec) != PREC_BF16):
        raise RuntimeError("gru_seq_bwd: want_dgi needs the a_n rows and the bf16 mode")
    t0, n = chunk if chunk is not None else (0, T)
    if not (0 <= t0 and n > 0 and t0 + n <= T):
        raise RuntimeError(f"gru_seq_bwd: chunk ({t0}, {n}) outside [0, {T})")
    carry = 1 if t0 + n < T else 0
    steps = n + carry                                   # a carried chunk re-visits frame t0+n to pick up its dh
    panels, status = _gru_ws(B, G, Hg, dout.device, slot)
    wa = _ptr_array(w_hh)
    _p(dout); _p(coef); _p(z); _p(dh); _p(an); _p(dgi)
    check(lib.cruse_gru_seq_bwd_ex(_off(dout, t0 * H), ctypes.cast(wa, ctypes.c_void_p), _off(coef, t0 * 3 * H), _off(z, t0 * H),
                                   _off(dh, t0 * H), _off(an, t0 * H) if want_dgi else None,
                                   None if dgi is None else _off(dgi, t0 * dg_slabs * H), dg_slabs, carry, B, steps, T, G, Hg, prec_code(prec),
                                   16 if wide else 0, panels, 1 if zeroed else 0, status, xcd_rot, _stream()))
    return (dh, dgi) if want_dgi else dh


def gru_gate_grads(dh, coef, an, rows, G, Hg, prec):
    if (coef.dtype == torch.bfloat16) != (prec_code(prec) == PREC_BF16):
        raise RuntimeError("gru_gate_grads: coef dtype does not match the precision mode")
    dgi = torch.empty(coef.shape, device=coef.device, dtype=torch.float32)
    dgh = torch.empty_like(dgi)
    check(lib.cruse_gru_gate_grads(_p(dh), _p(coef), _p(an), _p(dgi), _p(dgh), rows, G, Hg, prec_code(prec), _stream()))
    return dgi, dgh


def gru_gate_grads_bf16(dh, coef, an, rows, G, Hg, db_ih, db_hh, want_dgi=True, want_dgT=True):
    """bf16 gate gradients for gemm_bf16_nt: returns (dgi [rows,G,3,Hg] bf16, dgT [ldT/64,G,4,Hg,64] bf16, ldT) and
    accumulates the bias gradients into the per-group tensors db_ih[g], db_hh[g].  want_dgi / want_dgT False: that output
    is not made (None) -- the recurrence may have written dgi itself (gru_seq_bwd(want_dgi=True))."""
    if coef.dtype != torch.bfloat16:
        raise RuntimeError("gru_gate_grads_bf16 needs the bf16 coefficients of CRUSE_PREC_BF16")
    ldT = (rows + 63) // 64 * 64
    dgi = dgi_buffer(rows, G, Hg, dh.device) if want_dgi else None
    dgT = torch.empty(ldT // 64, G, 4, Hg, 64, device=dh.device, dtype=torch.bfloat16) if want_dgT else None
    check(lib.cruse_gru_gate_grads_bf16(_p(dh), _p(coef), _p(an), _p(dgi), _p(dgT), ldT, _ptr_array(db_ih),
                                        _ptr_array(db_hh), rows, G, Hg, _stream()))
    return dgi, dgT, ldT


def gru_status() -> int:
    """0 if no recurrence hand-off EVER timed out on any device of this process (synchronises).  The status word is
    sticky: neither the library nor later launches clear it (gru_status_reset and the per-step latch of step_health do)."""
    bad = 0
    for h in _gru_hdr.values():
        bad |= int(h[:4].view(torch.int32).item())
    return bad


def gru_status_word(device, B: int = 0, G: int = 0, Hg: int = 0) -> torch.Tensor:
    """The device status word itself (uint8[4] view of gru_header) -- handed to step_health / adam_step as skip_flag so that
    a step whose recurrence timed out never reaches the parameters.  (B, G, Hg are accepted for the round-3 callers.)"""
    return gru_header(device)[:4]


def gru_status_reset() -> None:
    for h in _gru_hdr.values():
        h.zero_()


def check_gru_status() -> None:
    """Raise (CRUSE_E_TIMEOUT) if a recurrence hand-off timed out since the last reset: the outputs of that launch
    were garbage.  Call once per epoch / before a checkpoint (synchronises)."""
    if gru_status() != 0:
        raise RuntimeError("cruse_hip error -5 (CRUSE_E_TIMEOUT): a GRU hand-off timed out -- the persistent recurrence "
                           "kernel's workgroups were not co-resident (another process or kernel holding CUs?); the "
                           "affected optimizer steps were skipped")


# ---------------------------------------------------------------- mask + loss, misc
def mask_loss(mask, nre, nim, cmag, rows, Fn, Fs, alpha=2.0, beta=1.0, want_dmask=False, want_dlogit=False,
              want_est=False):
    dev = mask.device
    loss_sum = torch.empty(1, device=dev, dtype=torch.float64)
    dmask = torch.empty(rows, Fn, device=dev, dtype=torch.float32) if want_dmask else None
    dlogit = torch.empty(rows, Fn, device=dev, dtype=torch.float32) if want_dlogit else None
    er = torch.empty(rows, Fs, device=dev, dtype=torch.float32) if want_est else None
    ei = torch.empty(rows, Fs, device=dev, dtype=torch.float32) if want_est else None
    check(lib.cruse_mask_loss_fwd(_p(mask), _p(nre), _p(nim), _p(cmag), rows, Fn, Fs, alpha, beta, _p(loss_sum),
                                  _p(dmask), _p(dlogit), _p(er), _p(ei), _stream()))
    return loss_sum, dmask, dlogit, er, ei


def mask_head_eligible(C, F1, Fs) -> bool:
    """shapes cruse_mask_head_fwd_bwd takes: up to 16 channels in rows of at most 640 floats, whole float4 per channel"""
    return 1 <= C <= 16 and F1 % 4 == 0 and C * F1 <= 640 and Fs == 2 * F1 + 1


def mask_head(bn: BnIn, w, bias, nre, nim, cmag, B, T, C, F1, Fs, alpha=2.0, beta=1.0, bwd_replicas=None, max_blocks=0, out=None):
    """The mask head of the training step in one launch (cruse_mask_head_fwd_bwd): bn_finalize_act_fwd of the VIRTUAL u = relu(bn(bn.y_pre))
    + bn.add, conv_scatter2(u, w, bias, sigmoid), mask_loss and the data gradient conv_gather(dlogit, w, bn_bwd of that BatchNorm), with
    the bits of those four calls.  bn.mean / bn.rstd and the running statistics are written as by the first of them.
    -> (u [B,T,C,F1], mask [B*T, 2*F1], loss_sum [1] f64, dlogit [B*T, 2*F1], du [B,T,C,F1], backward sums [replicas][2*C] f64).
    loss_sum and the sums come from the step's cleared arena when one is active: they are then valid until the next step begins.
    out: (u, mask, dlogit, du) to write into (tests)."""
    dev = bn.y_pre.device
    rows = B * T
    if out is None:
        u = torch.empty(B, T, C, F1, device=dev, dtype=torch.float32)
        mask = torch.empty(rows, 2 * F1, device=dev, dtype=torch.float32)
        dlogit = torch.empty(rows, 2 * F1, device=dev, dtype=torch.float32)
        du = torch.empty(B, T, C, F1, device=dev, dtype=torch.float32)
    else:
        u, mask, dlogit, du = out
    nrep = BN_STAT_REPLICAS if bwd_replicas is None else int(bwd_replicas)
    loss_sum, lz = ARENA.take(1, dev)
    sums, sz = ARENA.take(2 * C * nrep, dev)
    check(lib.cruse_mask_head_fwd_bwd(_p(bn.y_pre), _p(bn.sums), bn.nrep, bn.eps, bn.momentum, _p(bn.gamma), _p(bn.beta), _p(bn.add), _p(w), _p(bias),
                                      _p(nre), _p(nim), _p(cmag), B, T, C, F1, Fs, alpha, beta, _p(u), _p(bn.mean), _p(bn.rstd), _p(bn.rm), _p(bn.rv),
                                      _p(mask), _p(dlogit), _p(du), _p(loss_sum), lz, _p(sums), nrep, sz, max_blocks, _stream()))
    return u, mask, loss_sum, dlogit, du, sums


def mask_apply(mask, nre, nim, rows, Fn, Fs):
    er = torch.empty(rows, Fs, device=mask.device, dtype=torch.float32)
    ei = torch.empty_like(er)
    check(lib.cruse_mask_apply(_p(mask), _p(nre), _p(nim), rows, Fn, Fs, _p(er), _p(ei), _stream()))
    return er, ei


def mask_apply_bwd(dre, dim, nre, nim, mask, rows, Fn, Fs, through_sigmoid=True):
    out = torch.empty(rows, Fn, device=mask.device, dtype=torch.float32)
    check(lib.cruse_mask_apply_bwd(_p(dre), _p(dim), _p(nre), _p(nim), _p(mask), rows, Fn, Fs,
                                   1 if through_sigmoid else 0, _p(out), _stream()))
    return out


def mask_sdnr(mask, cre, cim, nre, nim, rows, Fn, Fs, B, snr_db, beta_db=20.0, want_dmask=False, want_dlogit=False):
    """sdnr (loss_func/loss.py:151-175) with the mask as gain -> (loss_sum f64[1] (divide by B*Fs), dmask, dlogit)."""
    dev = mask.device
    loss_sum = torch.empty(1, device=dev, dtype=torch.float64)
    dmask = torch.empty(rows, Fn, device=dev, dtype=torch.float32) if want_dmask else None
    dlogit = torch.empty(rows, Fn, device=dev, dtype=torch.float32) if want_dlogit else None
    check(lib.cruse_mask_sdnr_fwd(_p(mask), _p(cre), _p(cim), _p(nre), _p(nim), rows, Fn, Fs, B, snr_db, beta_db,
                                  _p(loss_sum), _p(dmask), _p(dlogit), _stream()))
    return loss_sum, dmask, dlogit


def sisnr_fwd(x, s, eps=1e-8):
    """-> (loss f64[1], coef [B,4]) for si_snr_loss(x, s) of train_base/loss.py:7-25."""
    B, L = x.shape
    if s.shape != x.shape:
        raise RuntimeError(f"Dimension mismatch when calculate si_snr, {tuple(x.shape)} vs {tuple(s.shape)}")
    mom = torch.empty(B, 5, device=x.device, dtype=torch.float64)
    loss = torch.empty(1, device=x.device, dtype=torch.float64)
    coef = torch.empty(B, 4, device=x.device, dtype=torch.float32)
    check(lib.cruse_sisnr_fwd(_p(x), _p(s), B, L, eps, _p(mom), _p(loss), _p(coef), _stream()))
    return loss, coef


def sisnr_bwd(x, s, coef, grad_scale=1.0):
    dx = torch.empty_like(x)
    B, L = x.shape
    check(lib.cruse_sisnr_bwd(_p(x), _p(s), _p(coef), B, L, grad_scale, _p(dx), _stream()))
    return dx


def wave_l1_mse(est, ref, mse: bool, want_grad=True):
    """-> (loss_sum f64[1], dest or None): torch.nn.L1Loss / MSELoss(reduction="mean") terms on waveforms -- the loss is
    loss_sum / est.numel(), dest its gradient wrt est (train_base/loss.py:3-4)."""
    if est.shape != ref.shape:
        raise RuntimeError(f"Dimension mismatch when calculate {'mse' if mse else 'l1'} loss, {tuple(est.shape)} vs {tuple(ref.shape)}")
    n = est.numel()
    loss = torch.empty(1, device=est.device, dtype=torch.float64)
    dest = torch.empty_like(est) if want_grad else None
    check(lib.cruse_wave_l1_mse(_p(est), _p(ref), n, 1 if mse else 0, 1.0 / n, _p(loss), _p(dest), _stream()))
    return loss, dest


MRSPEC_MIN_N, MRSPEC_MAX_N, MRSPEC_MAX_R = 128, 2048, 8


def mrspec_args(n_ffts, gamma=0.3, factor=1.0, f_complex=None):
    """-> (n_ffts tuple, gamma, factor, f_complex: None or a tuple of one weight per resolution), as MultResSpecLoss's constructor reads
    them (test/test_loss.py:198-210: None or 0 = no complex term, a scalar = that weight for every resolution, a list = one each).
    ValueError naming the argument for what cruse_mrspec_loss would refuse."""
    try:
        ns = tuple(int(n) for n in n_ffts)
    except TypeError:
        raise ValueError(f"n_ffts must be a sequence of FFT sizes, got {n_ffts!r}") from None
    if not 1 <= len(ns) <= MRSPEC_MAX_R:
        raise ValueError(f"n_ffts must hold 1..{MRSPEC_MAX_R} sizes, got {len(ns)}")
    for n in ns:
        if n < MRSPEC_MIN_N or n > MRSPEC_MAX_N or n & (n - 1):
            raise ValueError(f"n_ffts: {n} is not a power of two in [{MRSPEC_MIN_N}, {MRSPEC_MAX_N}]")
    gamma, factor = float(gamma), float(factor)
    if not gamma > 0.0:
        raise ValueError(f"gamma must be positive, got {gamma!r}")
    if isinstance(f_complex, (list, tuple)):
        fc = tuple(float(v) for v in f_complex)
        if len(fc) != len(ns):
            raise ValueError(f"f_complex has {len(fc)} values for {len(ns)} resolutions (n_ffts)")
    elif f_complex is None or f_complex == 0:
        fc = None
    else:
        fc = (float(f_complex),) * len(ns)
    return ns, gamma, factor, fc


def mrspec_ws_bytes(B, L, n_ffts) -> int:
    """cruse_mrspec_ws_bytes(B, L, n_ffts): 0 for a shape the call refuses"""
    arr = (ctypes.c_int * len(n_ffts))(*[int(n) for n in n_ffts])
    return int(lib.cruse_mrspec_ws_bytes(int(B), int(L), ctypes.cast(arr, ctypes.c_void_p), len(n_ffts)))


def mrspec_loss(est, ref, n_ffts, gamma=0.3, factor=1.0, f_complex=None, want_grad=True, grad_scale=1.0):
    """The multi-resolution spectral loss (MultResSpecLoss, test/test_loss.py:193-229) of waveforms est, ref [B,L] f32
    -> (loss f64[1], dloss/dest * grad_scale [B,L] or None).  R + 2 launches (R + 1 without the gradient), deterministic."""
    ns, gamma, factor, fc = mrspec_args(n_ffts, gamma, factor, f_complex)
    if est.dim() != 2 or est.shape != ref.shape:
        raise RuntimeError(f"Dimension mismatch when calculate the multi-resolution spectral loss, {tuple(est.shape)} vs {tuple(ref.shape)}")
    B, L = est.shape
    if L <= max(ns) // 2:
        raise ValueError(f"clips of {L} samples are too short for n_ffts {ns}: reflect padding needs more than {max(ns) // 2}")
    R = len(ns)
    n_arr = (ctypes.c_int * R)(*ns)
    fc_arr = (ctypes.c_float * R)(*fc) if fc is not None else None
    need = int(lib.cruse_mrspec_ws_bytes(B, L, ctypes.cast(n_arr, ctypes.c_void_p), R))
    if need == 0:
        check(-1)
    ws = _ws(("mrspec", _stream()), need, est.device, zero=False)
    loss = torch.empty(1, device=est.device, dtype=torch.float64)
    dest = torch.empty_like(est) if want_grad else None
    check(lib.cruse_mrspec_loss(_p(est), _p(ref), B, L, ctypes.cast(n_arr, ctypes.c_void_p), R, gamma, factor,
                                ctypes.cast(fc_arr, ctypes.c_void_p) if fc_arr is not None else None, _p(ws), need, _p(loss), _p(dest),
                                float(grad_scale), _stream()))
    return loss, dest


def deepfilter_fwd(xr, xi, hr, hi, f_dim, t_dim, out=None):
    B, F, T = xr.shape
    o_r, o_i = (torch.empty_like(xr), torch.empty_like(xr)) if out is None else out
    check(lib.cruse_deepfilter_fwd(_p(xr), _p(xi), _p(hr), _p(hi), B, F, T, f_dim, t_dim, _p(o_r), _p(o_i), _stream()))
    return o_r, o_i


def deepfilter_bwd(dor, doi, xr, xi, hr, hi, f_dim, t_dim):
    B, F, T = xr.shape
    outs = [torch.empty_like(xr) for _ in range(4)]
    check(lib.cruse_deepfilter_bwd(_p(dor), _p(doi), _p(xr), _p(xi), _p(hr), _p(hi), B, F, T, f_dim, t_dim,
                                   *[_p(o) for o in outs], _stream()))
    return outs


def df_head_apply(mask, nre, nim, t_dim=1, f_dim=5, out=None):
    """The DeepFilter head of a trained config-4 model in one launch (cruse_df_head_apply): mask [B*T, Fn] (any shape with B*T*Fn
    elements, such as unet_2's [B,1,T,Fn]), nre / nim [B,T,Fs] -> (ere, eim) [B,T,Fs], the (2*t_dim+1) x (2*f_dim+1) neighbourhood
    sum of mask * N with bins Fn..Fs-1 of the product zero.  The bits of mask_apply(mask, ones, zeros) + deepfilter_fwd as
    engine._deepfilter_loss composes them.  out: (ere, eim) to write into."""
    if nre.dim() != 3 or nim.shape != nre.shape:
        raise RuntimeError(f"df_head_apply: the spectrum planes must both be [B,T,Fs], got {tuple(nre.shape)} and {tuple(nim.shape)}")
    B, T, Fs = nre.shape
    rows = B * T
    Fn = mask.numel() // rows if rows > 0 else 0
    if rows <= 0 or Fn * rows != mask.numel():
        raise RuntimeError(f"df_head_apply: mask {tuple(mask.shape)} is not [B*T, Fn] for the spectrum {tuple(nre.shape)}")
    for name, t in (("mask", mask), ("nre", nre), ("nim", nim)):
        _f32(t, f"df_head_apply {name}")
    if out is None:
        ere = torch.empty(B, T, Fs, device=nre.device, dtype=torch.float32)
        eim = torch.empty_like(ere)
    else:
        ere, eim = out
        for name, t in (("ere", ere), ("eim", eim)):
            if _f32(t, f"df_head_apply {name}").numel() != rows * Fs:
                raise RuntimeError(f"df_head_apply: {name} {tuple(t.shape)} is not [B,T,Fs] = {(B, T, Fs)}")
    check(lib.cruse_df_head_apply(_p(mask), _p(nre), _p(nim), B, T, Fn, Fs, int(t_dim), int(f_dim), _p(ere), _p(eim), _stream()))
    return ere, eim


def sigmoid_bwd(dmask, mask):
    out = torch.empty_like(mask)
    check(lib.cruse_sigmoid_bwd(_p(dmask), _p(mask), _p(out), mask.numel(), _stream()))
    return out


def axpby(out, x, y, a, b):
    check(lib.cruse_axpby(_p(out), _p(x), _p(y), a, b, out.numel(), _stream()))
    return out


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, max_norm=0.0, gsumsq=None,
              skip_flag=None, loss_check=None, skipped=None, loss_sum=None, loss_scale=1.0, loss_acc=None):
    """Fused Adam over flat buffers; the optional device-side guards are described at cruse_adam_step_guarded.
    skip_flag: a uint8[4k] / int32[k] tensor of k status words (any non-zero word skips the step).  `step` counts the CALLS;
    with `skipped` the bias corrections use step - skipped[0].  loss_acc f64[2] += (loss_sum * loss_scale, 1) when applied."""
    nw = 0 if skip_flag is None else skip_flag.numel() * skip_flag.element_size() // 4
    if loss_acc is not None and (loss_acc.dtype != torch.float64 or loss_acc.numel() < 2):
        raise RuntimeError("adam_step: loss_acc must be an f64[2] tensor (sum, applied steps)")
    check(lib.cruse_adam_step_guarded(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step,
                                      grad_scale, max_norm, _p(gsumsq), _p(skip_flag), nw, _p(loss_check), _p(skipped),
                                      _p(loss_sum), float(loss_scale), _p(loss_acc), _stream()))


def step_health(gru_status, loss_sum, health, loss_acc=None, loss_scale=1.0) -> None:
    """health[0] = latched-and-cleared GRU status word, health[1] = non-finite loss; loss_acc += loss_sum * loss_scale
    (cruse_step_health).  health: int32[2]."""
    if health.dtype != torch.int32 or health.numel() < 2:
        raise RuntimeError("step_health needs an int32[2] health tensor")
    check(lib.cruse_step_health(_p(gru_status), _p(loss_sum), _p(health), _p(loss_acc), float(loss_scale), _stream()))


def gru_plan(B: int, groups: int, Hg: int, prec="bf16", fwd: bool = True) -> dict:
    """the launch plan of the recurrence for this shape (cruse_gru_plan): which kernels a batch size runs on"""
    out = (ctypes.c_int * 6)()
    check(lib.cruse_gru_plan(int(B), int(groups), int(Hg), prec_code(prec), 1 if fwd else 0, ctypes.cast(out, ctypes.c_void_p)))
    return {"clips_per_chain": out[0], "chains_per_group": out[1], "chains_per_launch": out[2], "launches": out[3],
            "workgroups_per_chain": out[4], "wide": bool(out[5])}


def cu_hog(nblocks: int, microseconds: float, clock_ghz: float = 2.1) -> None:
    """Test / probe rig: `nblocks` workgroups hold one CU each (128 KB of LDS) for about `microseconds` on the current stream
    (cruse_cu_hog) -- what a collective's channels or another tenant do to the persistent recurrences."""
    check(lib.cruse_cu_hog(int(nblocks), int(microseconds * 1e3 * clock_ghz), _stream()))


def zero_(t: torch.Tensor) -> torch.Tensor:
    """stream-ordered zero fill (kernel node; see cruse_zero)."""
    check(lib.cruse_zero(_p(t), t.numel() * t.element_size(), _stream()))
    return t


def accum_f64(acc: torch.Tensor, x: torch.Tensor) -> None:
    if acc.dtype != torch.float64 or x.dtype != torch.float64 or acc.numel() != x.numel():
        raise RuntimeError("accum_f64 needs two f64 tensors of the same size")
    check(lib.cruse_accum_f64(_p(acc), _p(x), acc.numel(), _stream()))


def counters_add(counters: Sequence[torch.Tensor], v: int = 1) -> None:
    """every int64 scalar tensor in `counters` += v with ONE launch (BatchNorm num_batches_tracked)."""
    for c in counters:
        if c.dtype != torch.int64:
            raise RuntimeError("counters_add needs int64 tensors")
    for i in range(0, len(counters), 32):
        part = counters[i:i + 32]
        check(lib.cruse_counters_add(ctypes.cast(_ptr_array(part), ctypes.c_void_p), len(part), v, _stream()))


def sumsq(x, out=None, accumulate=False):
    """sum of squares (f64[1]) of a flat f32 tensor: the squared total gradient norm of clip_grad_norm_."""
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float64)
    check(lib.cruse_sumsq(_p(x), x.numel(), _p(out), 1 if accumulate else 0, _stream()))
    return out


# ======================================================================================================================
# frame-by-frame streaming of unet_2 (cruse_stream_*; cruse_amd/inferencer/streaming.py drives the chain)
# ======================================================================================================================
STREAM_LAYOUT_NAMES = (
    [f"ch{k}" for k in range(5)] + [f"F{k}" for k in range(5)] + ["H"]
    + [f"{n}{k}" for n in ("encW", "encB", "skW", "decW", "decB") for k in range(5)]
    + ["ln1g", "ln1b", "ln2g", "ln2b", "wtotal", "st_hist", "st_tail"] + [f"st_prev{k}" for k in range(4)]
    + ["st_h1", "st_h2", "st_stride", "wk_re", "wk_im", "wk_x"] + [f"wk_skip{k}" for k in range(5)]
    + ["wk_h1n", "wk_h2n", "wk_mask", "wk_stride"])
STREAM_SKIP, STREAM_STORE, STREAM_FRAME, STREAM_FRAME0, STREAM_END = 0, 1, 2, 3, 4
STREAM_MAX_HG = 1024        # widest GRU group of cruse_stream_gru / _gru_proj_n / _gru_rec_n (16 slices of 64 lanes)


def stream_layout(ch) -> Dict[str, int]:
    """Offsets (floats) of the packed weights and of the per-slot state / work rows of the streaming kernels."""
    arr = (ctypes.c_int * len(STREAM_LAYOUT_NAMES))()
    check(lib.cruse_stream_layout(*[int(c) for c in ch], arr))
    return dict(zip(STREAM_LAYOUT_NAMES, list(arr)))


def stream_tables(device) -> torch.Tensor:
    tab = torch.empty(1120, device=device, dtype=torch.float32)
    check(lib.cruse_stream_tables(_p(tab), _stream()))
    return tab


# sample formats of the _io entry points (in_fmt / out_fmt of the header); the plain entry points are f32 on both sides
STREAM_FMT_F32, STREAM_FMT_S16 = 0, 1


def _stream_fmt(t: torch.Tensor, name: str) -> int:
    if t.dtype == torch.float32:
        return STREAM_FMT_F32
    if t.dtype == torch.int16:
        return STREAM_FMT_S16
    raise RuntimeError(f"{name}: expected float32 or int16 samples, got {t.dtype}")


def _stream_out(out: torch.Tensor, lim, clip, name: str):
    """(out_fmt, lim, clip) of a decode or head call; (STREAM_FMT_F32, None, None) is what the plain entry points serve"""
    fmt = _stream_fmt(out, name)
    if lim is not None and (lim.dtype != torch.float32 or lim.numel() != out.shape[0]):
        raise RuntimeError(f"{name}: lim must be float32 with one entry per slot ({out.shape[0]}), got {lim.dtype} x {lim.numel()}")
    if clip is not None and (clip.dtype != torch.int32 or clip.numel() != out.shape[0]):
        raise RuntimeError(f"{name}: clip must be int32 with one entry per slot ({out.shape[0]}), got {clip.dtype} x {clip.numel()}")
    return fmt, _p(lim), _p(clip)


def atten_lim_gain(db) -> float:
    """The linear gain of an attenuation limit of `db` dB (DeepFilterNet's atten_lim_db): 10^(-db / 20); None or inf -> 0 (no limit),
    0 -> 1 (the input passes through).  The output of a limited slot is gain * noisy + (1 - gain) * enhanced."""
    if db is None:
        return 0.0
    db = float(db)
    if db != db or db < 0.0:
        raise ValueError(f"attenuation limit must be a non-negative number of dB, inf or None, got {db}")
    return 0.0 if db == float("inf") else 10.0 ** (-db / 20.0)


def _stream_dims(ctl, hops, io, work):
    """the int arguments in front of the channels: S, or (hops given: a packet call) S, hops, the block stride of io, work_frames"""
    return (ctl.numel(),) if hops is None else (ctl.shape[1], int(hops), io.shape[1], work.shape[1])


def _stream_encode(name, ctl, hops, ch, blocks, tab, w, state, work) -> None:
    """cruse_<name> for float32 blocks, cruse_<name>_io for int16; hops: None for the single hop"""
    fmt = _stream_fmt(blocks, name)
    fn, io = (getattr(lib, f"cruse_{name}"), ()) if fmt == STREAM_FMT_F32 else (getattr(lib, f"cruse_{name}_io"), (fmt,))
    dims = _stream_dims(ctl, hops, blocks, work)
    check(fn(_p(ctl), *dims, *[int(c) for c in ch], _p(blocks), *io, _p(tab), _p(w), _p(state), _p(work), _stream()))


def stream_encode(mode, ch, blocks, tab, w, state, work) -> None:
    """blocks [S, 160]: float32, or int16 PCM (read as v / 32768, cruse_stream_encode_io)"""
    _stream_encode("stream_encode", mode, None, ch, blocks, tab, w, state, work)


def _f16_args(name, pack16):
    """the f32 entry point `name`, or its f16-operand twin with pack16 after `pack` in its parameter list"""
    return (getattr(lib, name), ()) if pack16 is None else (getattr(lib, name + "_f16"), (_p(pack16),))


def stream_gru(mode, layer, groups, Hg, x, x_off, hprev, h_off, pack, hout, o_off, ln_g=None, ln_b=None, ln_eps=1e-5, pack16=None) -> None:
    """One GGRU layer, one step, for every slot whose mode computes a frame; layer 2 applies LN1 (ln_g, ln_b) to layer 1's row.
    x / hprev / hout are [S, stride] row tensors read / written at the given float offsets.  pack16 (stream_pack_f16): run the
    f16-operand MFMA kernel; `pack` (f32) still supplies the biases."""
    fn, p16 = _f16_args("cruse_stream_gru", pack16)
    check(fn(_p(mode), mode.numel(), layer, groups, Hg, _p(x), x.shape[1], x_off, _p(ln_g), _p(ln_b), float(ln_eps), _p(hprev),
             hprev.shape[1], h_off, _p(pack), *p16, _p(hout), hout.shape[1], o_off, _stream()))


# the perceptual post-filter (cruse_mask_postfilter, cruse_stream_decode_pf / _n_pf; the reference's utils/utils.py:345-362)
POST_FILTER_KINDS = {"iam": 1, "envelope": 2}


def post_filter_kind(kind) -> int:
    """the pf_kind of the header for "iam" / "envelope"; anything else raises ValueError"""
    if kind not in POST_FILTER_KINDS:
        raise ValueError(f"post-filter kind must be one of {tuple(POST_FILTER_KINDS)}, got {kind!r}")
    return POST_FILTER_KINDS[kind]


def post_filter_tau(tau) -> float:
    """tau as a float; negative or NaN raises ValueError (0: the filter is off)"""
    tau = float(tau)
    if tau != tau or tau < 0.0 or tau == float("inf"):
        raise ValueError(f"post-filter tau must be a finite non-negative number, got {tau}")
    return tau


def post_filter(mask: torch.Tensor, tau=0.02, kind: str = "iam", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's postfiltering ("iam", utils/utils.py:345-349) / envelope_postfiltering ("envelope", :352-362) of a mask with values
    in [0, 1], in closed form, one pointwise kernel: float32, contiguous, any shape.  tau: a number (checked: >= 0), or a
    float32 device tensor [B] for a mask [B, ...] (one tau per clip; its values must be >= 0, which is not checked: no synchronisation).
    tau == 0 returns the mask's bits.  out: a contiguous float32 tensor of the mask's shape to write (it may be the mask).
    Inference only: a mask that requires grad raises."""
    k = post_filter_kind(kind)
    if mask.requires_grad:
        raise RuntimeError("post_filter is inference-only (no backward kernel): the mask requires grad")
    if mask.dtype != torch.float32 or not mask.is_contiguous() or mask.numel() < 1:
        raise RuntimeError(f"post_filter: mask must be a non-empty contiguous float32 tensor, got {mask.dtype} {tuple(mask.shape)}")
    if torch.is_tensor(tau):
        if tau.dtype != torch.float32 or tau.device != mask.device or tau.dim() != 1 or not tau.is_contiguous() or mask.dim() < 1 \
                or tau.numel() != mask.shape[0]:
            raise RuntimeError(f"post_filter: a tensor tau must be float32 [{mask.shape[0] if mask.dim() else 1}] on the mask's device, got "
                               f"{tau.dtype} {tuple(tau.shape)} on {tau.device}")
        F = mask.numel() // mask.shape[0]
        rows, per = mask.shape[0], 1
        if F < 1:
            raise RuntimeError(f"post_filter: empty mask {tuple(mask.shape)}")
    else:
        tau = torch.full((1,), post_filter_tau(tau), dtype=torch.float32, device=mask.device)
        rows, F, per = 1, mask.numel(), 0
    if out is None:
        out = torch.empty_like(mask)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape != mask.shape or out.device != mask.device:
        raise RuntimeError(f"post_filter: out must be contiguous float32 {tuple(mask.shape)} on the mask's device, got {out.dtype} "
                           f"{tuple(out.shape)}")
    check(lib.cruse_mask_postfilter(k, _p(mask), rows, F, _p(tau), per, _p(out), _stream()))
    return out


STREAM_DECODERS = ("transposed", "upsample")     # convkxf's modes: ConvTranspose2d levels (unet_2), FreqUpsample + Conv2d levels


def _stream_decode(name, ctl, hops, ch, tab, w, ln_eps, state, work, out, lim, clip, pf, decoder) -> None:
    """The decode call of stream_decode / stream_decode_n: "upsample" is cruse_<name>_up in every form; else a post-filter selects _pf, else
    int16 output, a limit or a counter _io, else the plain entry point.  hops: None for the single hop"""
    if decoder not in STREAM_DECODERS:
        raise ValueError(f"{name}: decoder must be one of {STREAM_DECODERS}, got {decoder!r}")
    io = _stream_out(out, lim, clip, name)
    pfa = (0, None)
    if pf is not None:                                    # (pf_kind, tau [S] f32)
        kind, tau = pf
        if tau.dtype != torch.float32 or tau.numel() != out.shape[0] or not tau.is_contiguous():
            raise RuntimeError(f"{name}: pf tau must be float32 with one entry per slot ({out.shape[0]}), got {tau.dtype} x {tau.numel()}")
        pfa = (int(kind), _p(tau))
    if decoder == "upsample":
        suffix, tail = "_up", (*io, *pfa)
    elif pf is not None:
        suffix, tail = "_pf", (*io, *pfa)
    elif out.dtype != torch.float32 or lim is not None or clip is not None:
        suffix, tail = "_io", io
    else:
        suffix, tail = "", ()
    fn = getattr(lib, f"cruse_{name}{suffix}")
    check(fn(_p(ctl), *_stream_dims(ctl, hops, out, work), *[int(c) for c in ch], _p(tab), _p(w), float(ln_eps), _p(state), _p(work),
             _p(out), *tail, _stream()))


def stream_decode(mode, ch, tab, w, ln_eps, state, work, out, lim=None, clip=None, pf=None, decoder="transposed") -> None:
    """out [S, 160]: float32, or int16 PCM (clamp(rint(y * 32768))); lim [S] f32: per-slot attenuation-limit gains (atten_lim_gain);
    clip [S] int32: += the clamped samples per slot (int16 out only).  Any of them selects cruse_stream_decode_io.
    pf = (pf_kind, tau [S] f32): the perceptual post-filter on the mask before the limit (cruse_stream_decode_pf).
    decoder = "upsample": w holds the [Cout][Cin][3] decoder weights of CRUSE4MagAddSkipUpsample; every form is cruse_stream_decode_up."""
    _stream_decode("stream_decode", mode, None, ch, tab, w, ln_eps, state, work, out, lim, clip, pf, decoder)


# packets: up to `hops` blocks per slot in one chain (cruse_stream_*_n).  pk is the [2, S] int32 device tensor of the header
# (row 0: blocks held, clamped to 2; row 1: blocks consumed); work is [S, work_frames, wk_stride], one row per frame.
def stream_packet_layout(ch) -> Dict[str, int]:
    """max_hops: the largest `hops` (work_frames - 1) whose rows fit the LDS of the packet kernels for these channels; wk_stride:
    floats of a frame's work row in a packet (the single-hop row, then e1 | e2 | e3 at wk_e1..wk_e3)."""
    arr = (ctypes.c_int * 5)()
    check(lib.cruse_stream_packet_layout(*[int(c) for c in ch], arr))
    return dict(zip(("max_hops", "wk_stride", "wk_e1", "wk_e2", "wk_e3"), list(arr)))


def stream_encode_n(pk, hops, ch, blocks, tab, w, state, work) -> None:
    """blocks [S, in_hops, 160]: float32, or int16 PCM (cruse_stream_encode_n_io)"""
    _stream_encode("stream_encode_n", pk, hops, ch, blocks, tab, w, state, work)


def stream_gru_proj_n(pk, hops, layer, groups, Hg, work, x_off, pack, gi, ln_g=None, ln_b=None, ln_eps=1e-5, pack16=None) -> None:
    """gi [S, work_frames, 3H] (f32) <- the layer's input products of every frame's work row at float offset x_off"""
    fn, p16 = _f16_args("cruse_stream_gru_proj_n", pack16)
    check(fn(_p(pk), pk.shape[1], int(hops), work.shape[1], layer, groups, Hg, _p(work), work.shape[2], x_off, _p(ln_g), _p(ln_b),
             float(ln_eps), _p(pack), *p16, _p(gi), _stream()))


def stream_gru_rec_n(pk, hops, frame, groups, Hg, gi, state, st_off, pack, work, h_off, pack16=None) -> None:
    fn, p16 = _f16_args("cruse_stream_gru_rec_n", pack16)
    check(fn(_p(pk), pk.shape[1], int(hops), work.shape[1], int(frame), groups, Hg, _p(gi), _p(state), state.shape[1], st_off, _p(pack),
             *p16, _p(work), work.shape[2], h_off, _stream()))


def stream_decode_n(pk, hops, ch, tab, w, ln_eps, state, work, out, lim=None, clip=None, pf=None, decoder="transposed") -> None:
    """out [S, out_hops, 160]: float32 or int16 PCM; lim / clip as stream_decode (cruse_stream_decode_n_io); pf as stream_decode
    (cruse_stream_decode_n_pf); decoder as stream_decode (cruse_stream_decode_n_up)"""
    _stream_decode("stream_decode_n", pk, hops, ch, tab, w, ln_eps, state, work, out, lim, clip, pf, decoder)


STREAM_BOUNDARY_ENTRIES = ("encode", "encode_io", "decode", "decode_io", "decode_pf", "decode_up", "encode_n", "encode_n_io", "decode_n",
                           "decode_n_io", "decode_n_pf", "decode_n_up", "df_head", "df_head_n")        # CRUSE_STREAM_ENTRY_*
_STREAM_PLAN_KEYS = ("family", "dec", "s16", "lim", "pf", "grid", "block", "lds_bytes", "wk_stride", "rowmax", "wcap")


def stream_boundary_plan(entry: str, *args) -> dict:
    """what cruse_stream_<entry>(*args, stream) launches (cruse_stream_boundary_plan; host-only): the kernel family and template instance,
    grid, block, dynamic LDS bytes and the packet geometry, "raw" the array as the library wrote it.  entry: one of STREAM_BOUNDARY_ENTRIES;
    args: of a pointer only "is it None (or 0)" counts, ln_eps is not looked at.  A call the entry point refuses raises its RuntimeError."""
    sig = SIGNATURES[f"cruse_stream_{entry}"][0][:-1]
    if len(args) != len(sig):
        raise ValueError(f"stream_boundary_plan: cruse_stream_{entry} takes {len(sig)} arguments in front of the stream, got {len(args)}")
    ints = [int(v) for c, v in zip(sig, args) if c == "i"]
    nulls = sum(1 << i for i, v in enumerate(v for c, v in zip(sig, args) if c == "p") if not v)
    out = (ctypes.c_int * len(_STREAM_PLAN_KEYS))()
    check(lib.cruse_stream_boundary_plan(STREAM_BOUNDARY_ENTRIES.index(entry), (ctypes.c_int * len(ints))(*ints), nulls, out))
    return dict(zip(_STREAM_PLAN_KEYS, out), raw=list(out))


# the DeepFilter(1, 5) head at the end of a chain (cruse_stream_df_head / _df_head_n): one frame behind decode, state rows of its own
STREAM_DF_LAYOUT_NAMES = ("p2", "p1", "n1", "tail", "count", "plane", "stride")
STREAM_DF_DIMS = (1, 5)     # the (t_dim, f_dim) instance the streaming kernels are built for
STREAM_DF_ROW = 2 * 161     # floats of an inspection row: E re | im


def stream_df_layout() -> Dict[str, int]:
    """Offsets (floats) in a df_state row: P[t-2], P[t-1], N[t-1] (re plane, im plane `plane` floats on), the overlap-add tail, the
    count of rows taken; `stride`: floats of a row."""
    arr = (ctypes.c_int * len(STREAM_DF_LAYOUT_NAMES))()
    check(lib.cruse_stream_df_layout(arr))
    return dict(zip(STREAM_DF_LAYOUT_NAMES, list(arr)))


def stream_df_head(mode, work, lay, tab, df_state, df_work, out, lim=None, clip=None, drain=False, df_dims=STREAM_DF_DIMS) -> None:
    """After stream_decode: every slot whose mode computes a frame takes the mask and the noisy spectrum of its row of work [S, wk_stride]
    (lay: wk_re / wk_im / wk_mask of stream_layout), writes E[t-1] to df_work [S, >= 322] and its block to out [S, 160] (float32 or
    int16; lim / clip as stream_decode).  drain: slots whose mode is END take a zero row instead (the clip's last E).  df_state
    [S, >= stream_df_layout()["stride"]] f32."""
    fmt, plim, pclip = _stream_out(out, lim, clip, "stream_df_head")
    _f32(df_work, "df_work")
    # rows may be a strided view (one row of several per slot): the kernel takes the row stride
    if not df_work.is_cuda or df_work.dim() != 2 or df_work.shape[0] != mode.numel() or df_work.shape[1] < STREAM_DF_ROW or df_work.stride(1) != 1:
        raise RuntimeError(f"stream_df_head: df_work must be [{mode.numel()}, >= {STREAM_DF_ROW}] rows of contiguous floats on the device, got "
                           f"{tuple(df_work.shape)} with strides {df_work.stride()}")
    check(lib.cruse_stream_df_head(_p(mode), mode.numel(), int(bool(drain)), _p(_f32(work, "work")), work.shape[1], int(lay["wk_re"]),
                                   int(lay["wk_im"]), int(lay["wk_mask"]), _p(tab), _p(_f32(df_state, "df_state")), df_state.shape[1],
                                   df_work.data_ptr(), df_work.stride(0), _p(out), fmt, plim, pclip, int(df_dims[0]), int(df_dims[1]),
                                   _stream()))


def stream_df_head_n(pk, hops, work, lay, tab, df_state, df_work, out, lim=None, clip=None, df_dims=STREAM_DF_DIMS) -> None:
    """After stream_decode_n: the same step for the frames of every slot's packet, in order.  work [S, work_frames, wk_stride];
    df_work [S, >= hops, 322]: one row per emitted E; out [S, out_hops, 160]: the emitted blocks from index 0."""
    fmt, plim, pclip = _stream_out(out, lim, clip, "stream_df_head_n")
    if df_work.dim() != 3 or df_work.shape[0] != pk.shape[1] or df_work.shape[2] != STREAM_DF_ROW or work.dim() != 3 or out.dim() != 3:
        raise RuntimeError(f"stream_df_head_n: expected work [S, frames, stride], out [S, hops, 160] and df_work [{pk.shape[1]}, rows, "
                           f"{STREAM_DF_ROW}], got {tuple(work.shape)}, {tuple(out.shape)}, {tuple(df_work.shape)}")
    check(lib.cruse_stream_df_head_n(_p(pk), pk.shape[1], int(hops), out.shape[1], work.shape[1], _p(_f32(work, "work")), work.shape[2],
                                     int(lay["wk_re"]), int(lay["wk_im"]), int(lay["wk_mask"]), _p(tab), _p(_f32(df_state, "df_state")),
                                     df_state.shape[1], _p(_f32(df_work, "df_work")), df_work.shape[1], _p(out), fmt, plim, pclip,
                                     int(df_dims[0]), int(df_dims[1]), _stream()))


# level meters and voice activity at the end of a chain (cruse_stream_meter / _meter_n): rows [L_in dBFS, L_out dBFS, p, vad]
STREAM_METER_LAYOUT_NAMES = ("p", "stride", "acc", "row")
STREAM_METER_ROW = 4        # floats of a meter row
# the reference's activitydetector constants (utils/utils.py:143-154): 50 ms windows, logistic of a + b + 10 log10(sum of squares)
_VAD_REF = dict(a=-1.0, b=0.2, window_samples=800, alpha_att=0.8, alpha_rel=0.05, target_level=-25.0, threshold=0.13, hops_per_window=5)


def stream_vad_defaults() -> Dict[str, float]:
    """The per-hop constants that reproduce the reference's activitydetector for a clip at its -25 dBFS target, in float64.
    The reference normalises the clip to target_level = -25 dBFS and takes x = a + b + 10 log10(sum of 800 squared samples)
    = a + b + 10 log10(800) + L, L the window's mean-square level in dB.  Here x = L_out - level_db on absolute levels, so for a clip that
    already sits at the target, level_db = -25 - (a + b + 10 log10(800)) - (-25) = -(a + b + 10 log10(800)) = -28.23 with a = -1, b = 0.2.
    One 50 ms window is five 10 ms hops: the per-hop attack 1 - (1 - 0.8)^(1/5) and release 1 - (1 - 0.05)^(1/5) reach, after five hops
    towards a constant p_raw, what the reference's constants reach in one window."""
    import math
    r = _VAD_REF
    n = r["hops_per_window"]
    level = r["target_level"] - (r["a"] + r["b"] + 10.0 * math.log10(r["window_samples"])) - r["target_level"]
    return {"level_db": level, "threshold": r["threshold"], "attack": 1.0 - (1.0 - r["alpha_att"]) ** (1.0 / n),
            "release": 1.0 - (1.0 - r["alpha_rel"]) ** (1.0 / n)}


def stream_meter_layout() -> Dict[str, int]:
    """p: the offset of p_prev in a meter_state row; stride: floats of that row; acc: doubles of a meter_acc row; row: floats of a meter row"""
    arr = (ctypes.c_int * len(STREAM_METER_LAYOUT_NAMES))()
    check(lib.cruse_stream_meter_layout(arr))
    return dict(zip(STREAM_METER_LAYOUT_NAMES, list(arr)))


def _stream_meter_args(name, S, vad_par, meter_state, meter_acc, out, lim, pf):
    """the checked tail of a meter call: (lim, pf_kind, pf_tau, vad_par, meter_state, st_stride, meter_acc, out, out_stride)"""
    if vad_par.dtype != torch.float32 or tuple(vad_par.shape) != (S, 4):
        raise RuntimeError(f"{name}: vad_par must be float32 [{S}, 4], got {vad_par.dtype} {tuple(vad_par.shape)}")
    if meter_acc.dtype != torch.float64 or tuple(meter_acc.shape) != (S, 4):
        raise RuntimeError(f"{name}: meter_acc must be float64 [{S}, 4], got {meter_acc.dtype} {tuple(meter_acc.shape)}")
    if lim is not None and (lim.dtype != torch.float32 or lim.numel() != S):
        raise RuntimeError(f"{name}: lim must be float32 with one entry per slot ({S}), got {lim.dtype} x {lim.numel()}")
    kind, tau = (0, None) if pf is None else pf
    if tau is not None and (tau.dtype != torch.float32 or tau.numel() != S):
        raise RuntimeError(f"{name}: pf tau must be float32 with one entry per slot ({S}), got {tau.dtype} x {tau.numel()}")
    # the rows of a slot may be a strided view (one row of several per slot): the kernel takes the slot stride
    if out.dtype != torch.float32 or not out.is_cuda or out.dim() not in (2, 3) or out.shape[0] != S or out.shape[-1] != STREAM_METER_ROW \
            or out.stride(-1) != 1 or (out.dim() == 3 and out.stride(1) != STREAM_METER_ROW):
        raise RuntimeError(f"{name}: out must be float32 [{S}, {STREAM_METER_ROW}] or [{S}, rows, {STREAM_METER_ROW}] meter rows on the "
                           f"device, got {out.dtype} {tuple(out.shape)} with strides {out.stride()}")
    return (_p(lim), int(kind), _p(tau), _p(vad_par), _p(_f32(meter_state, "meter_state")), meter_state.shape[1], _p(meter_acc),
            out.data_ptr(), out.stride(0))


def stream_meter(mode, work, lay, tab, vad_par, meter_state, meter_acc, out, lim=None, pf=None) -> None:
    """After stream_decode: every slot whose mode computes a frame reads the noisy spectrum and the mask of its row of work [S, wk_stride]
    (lay: wk_re / wk_im / wk_mask of stream_layout) and writes [L_in dBFS, L_out dBFS, p, vad] to out[s] (out [S, 4], possibly a strided
    view), p_prev to meter_state [S, >= stream_meter_layout()["stride"]] and its counts and sums to meter_acc [S, 4] f64; a FRAME0 slot
    resets both and writes no row.  vad_par [S, 4] f32: level_db, threshold, attack, release.  lim / pf: those of the stream_decode call,
    so that L_out is the level of what decode put out."""
    S = mode.numel()
    tail = _stream_meter_args("stream_meter", S, vad_par, meter_state, meter_acc, out, lim, pf)
    check(lib.cruse_stream_meter(_p(mode), S, _p(_f32(work, "work")), work.shape[1], int(lay["wk_re"]), int(lay["wk_im"]),
                                 int(lay["wk_mask"]), _p(tab), *tail, _stream()))


def stream_meter_n(pk, hops, work, lay, tab, vad_par, meter_state, meter_acc, out, lim=None, pf=None) -> None:
    """After stream_decode_n: the same for the frames of every slot's packet, in order.  work [S, work_frames, wk_stride]; out
    [S, out_hops, 4]: one row per output block of the slot, from index 0 (a clip's frame 0 yields neither)."""
    S = pk.shape[1]
    if work.dim() != 3 or out.dim() != 3:
        raise RuntimeError(f"stream_meter_n: expected work [S, frames, stride] and out [S, out_hops, {STREAM_METER_ROW}], got "
                           f"{tuple(work.shape)}, {tuple(out.shape)}")
    tail = _stream_meter_args("stream_meter_n", S, vad_par, meter_state, meter_acc, out, lim, pf)
    check(lib.cruse_stream_meter_n(_p(pk), S, int(hops), out.shape[1], work.shape[1], _p(_f32(work, "work")), work.shape[2],
                                   int(lay["wk_re"]), int(lay["wk_im"]), int(lay["wk_mask"]), _p(tab), *tail, _stream()))


# 8 / 32 / 48 kHz I/O around the 16 kHz chains (cruse_stream_resample_*). taps: stream_resample_taps(io_rate); rs_state [S, >= the two
# history sizes of inferencer.resample.history(io_rate)] f32: the slots' converter histories, zero at the start of a clip.
def stream_resample_taps(io_rate: int, device) -> torch.Tensor:
    """the f32 device table of the converters' low-pass (inferencer.resample.design, float64 rounded once)"""
    from .inferencer.resample import design
    return torch.from_numpy(design(io_rate)[1]).to(torch.float32).to(device)


def _rs_rows(lo: torch.Tensor, io: torch.Tensor, S: int, io_rate: int, name: str) -> None:
    """lo: the 16 kHz tensor [S, (hops,) 160], io: the io_rate tensor [S, (hops,) io_rate / 100] -- the kernels take the widths on trust"""
    B = int(io_rate) // 100
    if (lo.shape[0] != S or io.shape[0] != S or lo.dim() != io.dim() or lo.shape[-1] != 160 or io.shape[-1] != B
            or (lo.dim() == 3 and lo.shape[1] != io.shape[1])):
        raise RuntimeError(f"{name}: expected [{S}, (hops,) 160] and [{S}, (hops,) {B}] samples at io_rate {io_rate}, got "
                           f"{tuple(lo.shape)} and {tuple(io.shape)}")


def stream_resample_in(mode, io_rate, x, taps, rs_state, blocks) -> None:
    """x [S, io_rate / 100] (float32 or int16 PCM) -> blocks [S, 160] f32 for every slot whose mode is STORE or FRAME"""
    _rs_rows(blocks, x, mode.numel(), io_rate, "stream_resample_in")
    check(lib.cruse_stream_resample_in(_p(mode), mode.numel(), int(io_rate), _p(x), _stream_fmt(x, "stream_resample_in"), _p(taps),
                                       _p(_f32(rs_state, "rs_state")), rs_state.shape[1], _p(_f32(blocks, "blocks")), _stream()))


def stream_resample_out(mode, io_rate, out16, taps, rs_state, y, clip=None) -> None:
    """out16 [S, 160] f32 -> y [S, io_rate / 100] (float32 or int16 PCM, clip [S] int32 += the clamped samples) for every slot whose
    mode is FRAME or END"""
    _rs_rows(out16, y, mode.numel(), io_rate, "stream_resample_out")
    check(lib.cruse_stream_resample_out(_p(mode), mode.numel(), int(io_rate), _p(_f32(out16, "out16")), _p(taps), _p(_f32(rs_state, "rs_state")),
                                        rs_state.shape[1], _p(y), _stream_fmt(y, "stream_resample_out"), _p(clip), _stream()))


def stream_resample_in_n(pk, hops, io_rate, x, taps, rs_state, blocks) -> None:
    """x [S, in_hops, io_rate / 100] -> blocks [S, in_hops, 160] f32: the pk[1, s] blocks each slot consumes"""
    _rs_rows(blocks, x, pk.shape[1], io_rate, "stream_resample_in_n")
    check(lib.cruse_stream_resample_in_n(_p(pk), pk.shape[1], int(hops), x.shape[1], int(io_rate), _p(x), _stream_fmt(x, "stream_resample_in_n"),
                                         _p(taps), _p(_f32(rs_state, "rs_state")), rs_state.shape[1], _p(_f32(blocks, "blocks")), _stream()))


def stream_resample_out_n(pk, hops, io_rate, out16, taps, rs_state, y, clip=None) -> None:
    """out16 [S, out_hops, 160] f32 -> y [S, out_hops, io_rate / 100]: the output blocks each slot's packet yields"""
    _rs_rows(out16, y, pk.shape[1], io_rate, "stream_resample_out_n")
    check(lib.cruse_stream_resample_out_n(_p(pk), pk.shape[1], int(hops), y.shape[1], int(io_rate), _p(_f32(out16, "out16")), _p(taps),
                                          _p(_f32(rs_state, "rs_state")), rs_state.shape[1], _p(y), _stream_fmt(y, "stream_resample_out_n"),
                                          _p(clip), _stream()))


# the layer's fragment-ordered f16 weights for the f16-operand MFMA GRU (the pack16 argument of stream_gru / _gru_proj_n / _gru_rec_n)
def stream_pack_f16(w_ih: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """W_ih, W_hh [g, 3*Hg, Hg] (any float dtype / device) -> the flat f16 pack16 of the header, on the inputs' device:
    [ih | hh][g][gate][UT][KS][lane][8], units padded to 16 and K to 32 with zeros."""
    g, three_hg, Hg = w_ih.shape
    assert three_hg == 3 * Hg and w_hh.shape == w_ih.shape, (w_ih.shape, w_hh.shape)
    UT, KS = (Hg + 15) // 16, (Hg + 31) // 32
    w = torch.stack([w_ih, w_hh]).detach().float().reshape(2, g, 3, Hg, Hg)
    p = torch.zeros(2, g, 3, UT * 16, KS * 32, dtype=torch.float32, device=w.device)
    p[..., :Hg, :Hg] = w
    # unit = ut*16 + r, k = ks*32 + q*8 + j, lane = q*16 + r
    p = p.reshape(2, g, 3, UT, 16, KS, 4, 8).permute(0, 1, 2, 3, 5, 6, 4, 7)
    return p.contiguous().reshape(-1).to(torch.float16)


# ======================================================================================================================
# validation metrics (cruse_si_sdr, cruse_stoi*; cruse_amd/metrics.py caches the tables and the workspace)
# ======================================================================================================================
STOI_LAYOUT_NAMES = ("L10", "nF", "nGs", "nSB", "x10", "e", "nk", "kept", "tob", "part", "total")
STOI_TABLE_FLOATS = 1540


def _clip_pair(ref: torch.Tensor, est: torch.Tensor, name: str):
    if ref.dim() != 2 or ref.shape != est.shape:
        raise RuntimeError(f"{name}: expected two [B, L] tensors of one shape, got {tuple(ref.shape)} and {tuple(est.shape)}")
    return _p(_f32(ref, name)), _p(_f32(est, name)), ref.shape[0], ref.shape[1]


def _clip_lengths(lengths: torch.Tensor, B: int, device, name: str) -> torch.Tensor:
    """lengths of a ragged batch: int32 [B] on the clips' device, read by the kernels only"""
    if not isinstance(lengths, torch.Tensor):
        raise RuntimeError(f"{name}: lengths must be an int32 device tensor [{B}] (cruse_amd.metrics takes host sequences)")
    return _i32(lengths, B, device, f"{name}: lengths")


def si_sdr(ref: torch.Tensor, est: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SI-SDR in dB of every clip of est [B, L] against ref [B, L] -> [B] f32; with lengths (int32 [B] on the device) clip b is its
    first lengths[b] samples (cruse_si_sdr_ragged: clamped to [0, L], nothing beyond is loaded, 0 scores NaN)"""
    r, e, B, L = _clip_pair(ref, est, "si_sdr")
    out = torch.empty(B, device=ref.device, dtype=torch.float32)
    if lengths is None:
        check(lib.cruse_si_sdr(r, e, B, L, _p(out), _stream()))
    else:
        check(lib.cruse_si_sdr_ragged(r, e, B, L, _p(_clip_lengths(lengths, B, ref.device, "si_sdr")), _p(out), _stream()))
    return out


def stoi_layout(B: int, L: int) -> Dict[str, int]:
    """Sizes of the STOI stages and the offsets (4-byte units) of the stage arrays in the workspace of cruse_stoi(B, L)."""
    arr = (ctypes.c_int * len(STOI_LAYOUT_NAMES))()
    check(lib.cruse_stoi_layout(int(B), int(L), arr))
    return dict(zip(STOI_LAYOUT_NAMES, list(arr)))


def stoi_tables(device) -> torch.Tensor:
    tab = torch.empty(STOI_TABLE_FLOATS, device=device, dtype=torch.float32)
    check(lib.cruse_stoi_tables(_p(tab), _stream()))
    return tab


def stoi_workspace(B: int, L: int, device) -> torch.Tensor:
    """an f32 tensor of cruse_stoi_ws_bytes(B, L) bytes (raises where the shape is refused)"""
    n = stoi_layout(B, L)["total"]
    assert 4 * n == lib.cruse_stoi_ws_bytes(int(B), int(L))
    return torch.empty(n, device=device, dtype=torch.float32)


def stoi(ref: torch.Tensor, est: torch.Tensor, tab: torch.Tensor, ws: torch.Tensor, out: Optional[torch.Tensor] = None,
         lengths: Optional[torch.Tensor] = None, extended: bool = False) -> torch.Tensor:
    """classic STOI of every clip of est [B, L] against ref [B, L], both at 16 kHz -> [B] f32; the stages stay in ws (stoi_layout).
    With lengths (int32 [B] on the device: clip b is its first lengths[b] samples) or extended (ESTOI) the call is cruse_stoi_ragged,
    with the same tables and workspace; extended without lengths scores the whole rows."""
    r, e, B, L = _clip_pair(ref, est, "stoi")
    if out is None:
        out = torch.empty(B, device=ref.device, dtype=torch.float32)
    nbytes = ws.numel() * ws.element_size()
    if lengths is None and not extended:
        check(lib.cruse_stoi(r, e, B, L, _p(_f32(tab, "stoi")), _p(ws), nbytes, _p(_f32(out, "stoi")), _stream()))
        return out
    if lengths is None:
        lengths = torch.full((B,), L, device=ref.device, dtype=torch.int32)
    check(lib.cruse_stoi_ragged(r, e, B, L, _p(_clip_lengths(lengths, B, ref.device, "stoi")), 1 if extended else 0, _p(_f32(tab, "stoi")),
                                _p(ws), nbytes, _p(_f32(out, "stoi")), _stream()))
    return out


SDR_CHUNK = 2048            # CRUSE_SDR_CHUNK (include/cruse_hip.h): samples of a correlation chunk and outputs of a projection tile
SDR_MAX_TAPS = 1024         # CRUSE_SDR_MAX_TAPS


def sdr_workspace(B: int, L: int, K: int, device) -> torch.Tensor:
    """a float64 tensor of cruse_sdr_ws_bytes(B, L, K) bytes (raises where the shape is refused)"""
    n = lib.cruse_sdr_ws_bytes(int(B), int(L), int(K))
    if n == 0:
        raise RuntimeError(f"sdr_workspace: cruse_hip error -1: {(lib.cruse_last_error() or b'').decode()}")
    return torch.empty(n // 8, device=device, dtype=torch.float64)


def sdr(ref: torch.Tensor, est: torch.Tensor, ws: torch.Tensor, filter_len: int = 512, out: Optional[torch.Tensor] = None,
        lengths: Optional[torch.Tensor] = None, dbg: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bss_eval SDR in dB (one source, filter_len taps) of every clip of est [B, L] against ref [B, L] -> [B]
    f32.  ws: sdr_workspace(B, L, filter_len, device).  lengths: int32 [B] on the device, clip b is its first lengths[b] samples.
    dbg: float64 [B, 3 K + 2] on the device, receives raa, rab, C and the energies of s_target and of the error per clip."""
    r, e, B, L = _clip_pair(ref, est, "sdr")
    K = int(filter_len)
    need = lib.cruse_sdr_ws_bytes(B, L, K)
    if need == 0:
        check(-1)
    if ws.numel() * ws.element_size() < need:
        raise RuntimeError(f"sdr: workspace of {ws.numel() * ws.element_size()} bytes, cruse_sdr_ws_bytes({B}, {L}, {K}) = {need}")
    if out is None:
        out = torch.empty(B, device=ref.device, dtype=torch.float32)
    elif out.numel() != B:
        raise RuntimeError(f"sdr: out of {out.numel()} elements for {B} clip(s)")
    if dbg is not None and (dbg.dtype != torch.float64 or dbg.numel() != B * (3 * K + 2)):
        raise RuntimeError(f"sdr: dbg must be float64 [{B}, {3 * K + 2}], got {dbg.dtype} {tuple(dbg.shape)}")
    ln = None if lengths is None else _p(_clip_lengths(lengths, B, ref.device, "sdr"))
    check(lib.cruse_sdr(r, e, ln, B, L, K, _p(ws), _p(_f32(out, "sdr")), _p(dbg), _stream()))
    return out


# ======================================================================================================================
# biquad cascade (cruse_biquad_cascade; cruse_amd/acoustics/audio_aug.py designs the sections, data.DevicePairs applies them)
# ======================================================================================================================
BIQUAD_CHUNK = 32           # CRUSE_BIQUAD_CHUNK (include/cruse_hip.h): consecutive samples a lane holds
BIQUAD_TILE = 32768         # CRUSE_BIQUAD_TILE: samples a workgroup holds; a longer clip goes through tiles in order
BIQUAD_MAX_SECTIONS = 8


def biquad_cascade(x: torch.Tensor, coef: torch.Tensor, clamp: bool = True, out: Optional[torch.Tensor] = None,
                   ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """S biquad sections in order over every clip of x [B, L] f32 -> [B, L] f32: scipy.signal.lfilter in float64 from rest, with
    clamp the output of every section clipped to [-1, 1].  coef: float64 on the device, [S, 6] (shared) or [B, S, 6], rows
    (b0 b1 b2 a0 a1 a2).  ws: a workspace of cruse_biquad_ws_bytes(B, L, S) bytes, taken here when None (0 bytes for every shape today;
    the parameter lets a caller that captures the call into a graph own the buffer, and the tests guard it with sentinels)."""
    if x.dim() != 2:
        raise RuntimeError(f"biquad_cascade: x must be [B, L], got {tuple(x.shape)}")
    B, L = x.shape
    if coef.dtype != torch.float64:
        raise RuntimeError(f"biquad_cascade: coefficients must be float64 (DESIGN section 14), got {coef.dtype}")
    if coef.dim() == 2 and coef.shape[1] == 6:
        S, stride = coef.shape[0], 0
    elif coef.dim() == 3 and coef.shape[0] == B and coef.shape[2] == 6:
        S, stride = coef.shape[1], 6 * coef.shape[1]
    else:
        raise RuntimeError(f"biquad_cascade: coefficients {tuple(coef.shape)} must be [S, 6] or [{B}, S, 6]")
    if coef.device != x.device:
        raise RuntimeError(f"biquad_cascade: coefficients on {coef.device}, samples on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise RuntimeError(f"biquad_cascade: out {tuple(out.shape)} != x {tuple(x.shape)}")
    need = lib.cruse_biquad_ws_bytes(int(B), int(L), int(S))
    if ws is None and need:
        ws = torch.empty(need, device=x.device, dtype=torch.uint8)
    if ws is not None and ws.numel() * ws.element_size() < need:
        raise RuntimeError(f"biquad_cascade: workspace of {ws.numel() * ws.element_size()} bytes, {need} needed")
    check(lib.cruse_biquad_cascade(_p(_f32(x, "biquad_cascade")), _p(coef), stride, B, L, S, 1 if clamp else 0, _p(ws),
                                   _p(_f32(out, "biquad_cascade")), _stream()))
    return out


# ======================================================================================================================
# FFT convolution with a bank of filters (cruse_fftconv_*; data.add_reverb and data.DevicePairs apply room impulse responses with it)
# ======================================================================================================================
FFTCONV_PART = 2048         # CRUSE_FFTCONV_PART (include/cruse_hip.h): samples per partition; one spectrum is 8 * FFTCONV_PART bytes


class FftConvFilters:
    """A prepared filter bank: `spec` (uint8, cruse_fftconv_spec_bytes), the NR filters of R taps it came from, and whether it holds
    the early spectra."""

    def __init__(self, spec: torch.Tensor, NR: int, R: int, early: bool):
        self.spec, self.NR, self.R, self.early = spec, NR, R, early


_FFTCONV_WS: Dict[tuple, torch.Tensor] = {}


def _i32(t: torch.Tensor, n: int, device, name: str) -> torch.Tensor:
    if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != n or t.device != device:
        raise RuntimeError(f"{name}: expected int32 [{n}] on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def fft_conv_prepare(h: torch.Tensor, early_len: Optional[torch.Tensor] = None, spec: Optional[torch.Tensor] = None) -> FftConvFilters:
    """h [R] or [NR, R] f32 on the device -> the spectra cruse_fftconv_apply reads.  early_len: int32 [NR] on the device; the bank then
    also holds every filter cut to its first clamp(early_len, 0, R) taps.  spec: a caller's uint8 buffer (taken here when None)."""
    if h.dim() not in (1, 2) or h.numel() == 0:
        raise RuntimeError(f"fft_conv_prepare: filters must be [R] or [NR, R], got {tuple(h.shape)}")
    h2 = h.reshape(1, -1) if h.dim() == 1 else h
    NR, R = h2.shape
    if early_len is not None:
        _i32(early_len, NR, h.device, "fft_conv_prepare: early_len")
    need = lib.cruse_fftconv_spec_bytes(int(NR), int(R), 0 if early_len is None else 1)
    if spec is None:
        spec = torch.empty(need, device=h.device, dtype=torch.uint8)
    nbytes = spec.numel() * spec.element_size()
    check(lib.cruse_fftconv_prepare(_p(_f32(h2, "fft_conv_prepare")), NR, R, _p(early_len), _p(spec), nbytes, _stream()))
    return FftConvFilters(spec, NR, R, early_len is not None)


def fft_conv_apply(x: torch.Tensor, bank: FftConvFilters, h_index: Optional[torch.Tensor] = None, want_early: bool = False,
                   out: Optional[torch.Tensor] = None, out_early: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None):
    """x [B, L] f32 -> fftconvolve(x[b], h[f(b)])[:L] per clip (and, with want_early, the same through the early filters: a pair).
    f(b) = h_index[b] (int32 [B] on the device; negative or >= NR: the clip passes through unchanged); without h_index the bank holds
    one filter for all clips or one per clip.  The input-spectrum workspace is cached per (device, B, L) unless `ws` is given."""
    if x.dim() != 2:
        raise RuntimeError(f"fft_conv_apply: x must be [B, L], got {tuple(x.shape)}")
    B, L = x.shape
    if want_early and not bank.early:
        raise RuntimeError("fft_conv_apply: the bank was prepared without early_len")
    if bank.spec.device != x.device:
        raise RuntimeError(f"fft_conv_apply: filters on {bank.spec.device}, samples on {x.device}")
    if h_index is not None:
        _i32(h_index, B, x.device, "fft_conv_apply: h_index")
    need = lib.cruse_fftconv_ws_bytes(int(B), int(L))
    if ws is None:
        key = (x.device, int(B), int(L))
        ws = _FFTCONV_WS.get(key)
        if ws is None:
            ws = _FFTCONV_WS[key] = torch.empty(need, device=x.device, dtype=torch.uint8)
    outs = []
    for o in (out, out_early if want_early else None):
        if o is not None and o.shape != x.shape:
            raise RuntimeError(f"fft_conv_apply: out {tuple(o.shape)} != x {tuple(x.shape)}")
        outs.append(torch.empty_like(x) if o is None else _f32(o, "fft_conv_apply"))
    y, ye = outs[0], outs[1] if want_early else None
    check(lib.cruse_fftconv_apply(_p(_f32(x, "fft_conv_apply")), B, L, _p(bank.spec), bank.spec.numel() * bank.spec.element_size(), bank.NR, bank.R,
                                  _p(h_index), _p(ws), ws.numel() * ws.element_size(), _p(y), _p(ye), _stream()))
    return (y, ye) if want_early else y


def fft_conv_causal(x: torch.Tensor, h: torch.Tensor, early_len: Optional[torch.Tensor] = None):
    """scipy.signal.fftconvolve(x, h)[:L] per clip in one call: x [B, L], h [R] (shared) or [B, R]; with early_len (int32 [1] or [B])
    a pair (y, y_early)."""
    if h.dim() == 2 and h.shape[0] != x.shape[0]:
        raise RuntimeError(f"fft_conv_causal: filters {tuple(h.shape)} must be [R] or [{x.shape[0]}, R]")
    return fft_conv_apply(x, fft_conv_prepare(h, early_len), want_early=early_len is not None)


def peak_scale(x: torch.Tensor, ref: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """x[b] / (max |ref[b]| + eps) per clip, x and ref [B, L] f32: snr_mix's peak normalisation of `ref` applied to `x`"""
    if x.dim() != 2 or x.shape != ref.shape:
        raise RuntimeError(f"peak_scale: expected two [B, L] tensors of one shape, got {tuple(x.shape)} and {tuple(ref.shape)}")
    y = torch.empty_like(x)
    check(lib.cruse_peak_scale(_p(_f32(x, "peak_scale")), _p(_f32(ref, "peak_scale")), x.shape[0], x.shape[1], float(eps), _p(y), _stream()))
    return y


# ======================================================================================================================
# recordings -> training clips (cruse_resample_poly, cruse_assemble_clips; filepairs.DeviceFilePairs preloads and batches with them)
# ======================================================================================================================
RESAMPLE_TILE = 1024        # CRUSE_RESAMPLE_TILE (include/cruse_hip.h): consecutive outputs of one clip a workgroup owns
_RESAMPLE_TAPS: Dict[tuple, torch.Tensor] = {}


def resample_taps(up: int, down: int, device) -> torch.Tensor:
    """the phase-major f32 table [up, stride] of the reduced ratio up / down on `device` (resample_design), built once"""
    key = (torch.device(device), int(up), int(down))
    if key not in _RESAMPLE_TAPS:
        from . import resample_design as D
        table = D.phase_table(D.design(up, down).astype("float32"), up)
        _RESAMPLE_TAPS[key] = torch.from_numpy(table).to(device)
    return _RESAMPLE_TAPS[key]


def _host_i64(a, name: str):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
    if a.ndim != 1 or a.shape[0] < 2:
        raise RuntimeError(f"{name}: expected int64 [B + 1] offsets on the host, got shape {a.shape}")
    return a


def resample_poly(src: torch.Tensor, off_in, off_out, up: int, down: int, out: torch.Tensor, channels: int = 1, channel: int = 0,
                  off_in_dev: Optional[torch.Tensor] = None, off_out_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.signal.resample_poly(clip, up, down, window=resample_design.design(up, down)) for every clip of a ragged batch, in one
    launch.  src: flat f32 (mono) or int16 PCM interleaved over `channels`, of which `channel` is read (x / 32768); clip b is the
    frames [off_in[b], off_in[b + 1]) and fills out[off_out[b] : off_out[b + 1]], ceil(L up / down) samples.  off_in / off_out: int64
    [B + 1] HOST arrays (the library judges them and sizes the grid from them); their device copies are made here unless given.
    up / down are reduced here; up = down = 1 is the conversion alone (bit-exact)."""
    import math
    import numpy as np
    hi, ho = _host_i64(off_in, "resample_poly: off_in"), _host_i64(off_out, "resample_poly: off_out")
    if hi.shape != ho.shape:
        raise RuntimeError(f"resample_poly: off_in {hi.shape} and off_out {ho.shape} differ")
    B = hi.shape[0] - 1
    if src.dim() != 1 or src.dtype not in (torch.float32, torch.int16):
        raise RuntimeError(f"resample_poly: src must be flat float32 or int16, got {src.dtype} {tuple(src.shape)}")
    if out.dim() != 1 or out.device != src.device:
        raise RuntimeError(f"resample_poly: out must be flat float32 on {src.device}, got {tuple(out.shape)} on {out.device}")
    up, down = int(up), int(down)
    g = math.gcd(up, down) if up > 0 and down > 0 else 1
    up, down = up // g, down // g
    if np.any(np.diff(hi) < 0) or np.any(np.diff(ho) < 0) or hi[0] < 0 or ho[0] < 0:
        pass                                                   # the library refuses these by name (CRUSE_E_SHAPE)
    elif int(hi[-1]) * max(int(channels), 1) > src.numel() or int(ho[-1]) > out.numel():
        raise RuntimeError(f"resample_poly: offsets end at {int(hi[-1])} frames / {int(ho[-1])} outputs, beyond src ({src.numel()} values, "
                           f"{channels} channels) or out ({out.numel()})")
    di = torch.from_numpy(hi).to(src.device) if off_in_dev is None else off_in_dev
    do = torch.from_numpy(ho).to(src.device) if off_out_dev is None else off_out_dev
    for d in (di, do):
        if d.dtype != torch.int64 or d.shape != (B + 1,) or d.device != src.device:
            raise RuntimeError(f"resample_poly: device offsets must be int64 [{B + 1}] on {src.device}")
    taps, ntap, stride = None, 0, 0
    if (up, down) != (1, 1) and 1 <= up <= 1024 and 1 <= down <= 1024:
        taps = resample_taps(up, down, src.device)
        ntap, stride = 32 * max(up, down) + 1, taps.shape[1]
    check(lib.cruse_resample_poly(_p(src), 0 if src.dtype == torch.float32 else 1, int(channels), int(channel), hi.ctypes.data, ho.ctypes.data,
                                  _p(di), _p(do), B, up, down, _p(taps), ntap, stride, _p(_f32(out, "resample_poly")), _stream()))
    return out


def check_clip_plan(seg, seg_first, B: int, L: int, pool_len: int) -> None:
    """Refuse a malformed plan of assemble_clips from the HOST arrays it was built from (the device never validates): seg int64
    [nseg, 3] rows (src, dst, len), seg_first [B + 1] ascending from 0 to nseg; per clip len >= 1, dst ascending without overlap inside
    [0, L), and [src, src + len) inside the pool."""
    import numpy as np
    seg, first = np.asarray(seg), np.asarray(seg_first)
    if seg.ndim != 2 or seg.shape[1] != 3 or seg.dtype != np.int64:
        raise ValueError(f"clip plan: seg must be int64 [nseg, 3], got {seg.dtype} {seg.shape}")
    if first.shape != (B + 1,) or first[0] != 0 or first[-1] != seg.shape[0] or np.any(np.diff(first) < 0):
        raise ValueError(f"clip plan: seg_first must rise from 0 to {seg.shape[0]} over {B + 1} entries, got {first.tolist()}")
    if seg.shape[0] == 0:
        return
    src, dst, ln = seg[:, 0], seg[:, 1], seg[:, 2]
    if np.any(ln < 1) or np.any(dst < 0) or np.any(dst + ln > L):
        raise ValueError(f"clip plan: a segment is empty or leaves the clip [0, {L})")
    if np.any(src < 0) or np.any(src + ln > pool_len):
        raise ValueError(f"clip plan: a segment leaves the pool [0, {pool_len})")
    inner = np.ones(seg.shape[0], dtype=bool)
    inner[first[:-1][np.diff(first) > 0]] = False              # the first segment of every clip has no predecessor
    if np.any((dst[1:] < (dst + ln)[:-1]) & inner[1:]):
        raise ValueError("clip plan: the segments of a clip overlap or are not ascending in dst")


def assemble_clips(pool: torch.Tensor, seg, seg_first, L: int, out: Optional[torch.Tensor] = None, seg_dev: Optional[torch.Tensor] = None,
                   first_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, dst + j] = pool[src + j] over the segments of clip b, 0.0 elsewhere -> [B, L] f32: utterances stitched with silence gaps
    and cropped (filepairs.plan_clip).  pool: flat f32 on the device.  seg / seg_first: the plan on the HOST (numpy int64 [nseg, 3] and
    int [B + 1]), judged here by check_clip_plan; seg_dev (int64 [nseg, 3]) / first_dev (int32 [B + 1]) are its device copies where the
    caller has staged them already (a pinned ring), made here otherwise."""
    import numpy as np
    seg = np.ascontiguousarray(seg)
    first = np.ascontiguousarray(np.asarray(seg_first, dtype=np.int32))
    B, L = first.shape[0] - 1, int(L)
    if pool.dim() != 1:
        raise RuntimeError(f"assemble_clips: the pool must be flat, got {tuple(pool.shape)}")
    check_clip_plan(seg, first, B, L, pool.numel())
    nseg = seg.shape[0]
    if seg_dev is None:
        seg_dev = torch.from_numpy(seg).to(pool.device)
    if first_dev is None:
        first_dev = torch.from_numpy(first).to(pool.device)
    if seg_dev.dtype != torch.int64 or seg_dev.numel() != 3 * nseg or seg_dev.device != pool.device:
        raise RuntimeError(f"assemble_clips: seg_dev must be int64 [{nseg}, 3] on {pool.device}")
    _i32(first_dev, B + 1, pool.device, "assemble_clips: first_dev")
    if out is None:
        out = torch.empty(B, L, device=pool.device, dtype=torch.float32)
    elif out.shape != (B, L) or out.device != pool.device:
        raise RuntimeError(f"assemble_clips: out {tuple(out.shape)} on {out.device}, expected {(B, L)} on {pool.device}")
    check(lib.cruse_assemble_clips(_p(_f32(pool, "assemble_clips")), _p(seg_dev) if nseg else None, _p(first_dev), nseg, B, L,
                                   _p(_f32(out, "assemble_clips")), _stream()))
    return out


# ======================================================================================================================
# grouped linears and band pooling (cruse_grouped_linear_*, cruse_band_*; model/based_model/cust_conv.py builds GroupedLinearEinsum,
# GroupedLinear, SqueezedGRU(_S) and the ERB products on them)
# ======================================================================================================================
GL_CAT, GL_SHUFFLED = 0, 1
BAND_MAX_F = 2048           # CRUSE_BAND_MAX_F (include/cruse_hip.h)


def _gl_dims(w_shape, layout: str):
    """(G, Ig, Hg) and the element strides (group, in, out) of a contiguous weight: "gih" = [G, Ig, Hg] (GroupedLinearEinsum),
    "ghi" = [G, Hg, Ig] (the stacked nn.Linear weights of GroupedLinear)."""
    if len(w_shape) != 3:
        raise RuntimeError(f"grouped_linear: the weight must be [G, ., .], got {tuple(w_shape)}")
    if layout == "gih":
        G, Ig, Hg = (int(v) for v in w_shape)
        return G, Ig, Hg, (Ig * Hg, Hg, 1)
    if layout == "ghi":
        G, Hg, Ig = (int(v) for v in w_shape)
        return G, Ig, Hg, (Hg * Ig, 1, Ig)
    raise RuntimeError(f"grouped_linear: unknown weight layout {layout!r} (\"gih\" or \"ghi\")")


def _gl_rows(t: torch.Tensor, width: int, name: str) -> int:
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1:
        raise RuntimeError(f"grouped_linear: {name} must be [rows >= 1, {width}], got {tuple(t.shape)}")
    return int(t.shape[0])


def grouped_linear(x: torch.Tensor, w: torch.Tensor, layout: str = "gih", bias: Optional[torch.Tensor] = None, relu: bool = False,
                   shuffle: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [rows, G * Ig] -> y [rows, G * Hg]: group g maps its slice of x through its own [Ig -> Hg] weight (+ bias [G * Hg], group-major;
    then ReLU), one launch for all groups.  shuffle: the outputs go where GroupedLinear(shuffle=True)'s view(-1, Hg, G).transpose(-1, -2)
    puts them, in the store index."""
    G, Ig, Hg, (sg, si, so) = _gl_dims(w.shape, layout)
    rows = _gl_rows(x, G * Ig, "x")
    if bias is not None and bias.numel() != G * Hg:
        raise RuntimeError(f"grouped_linear: bias of {bias.numel()} elements, expected {G * Hg}")
    if out is None:
        out = torch.empty(rows, G * Hg, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (rows, G * Hg):
        raise RuntimeError(f"grouped_linear: out {tuple(out.shape)} != {(rows, G * Hg)}")
    check(lib.cruse_grouped_linear_fwd(_p(_f32(x, "grouped_linear")), _p(_f32(w, "grouped_linear")), sg, si, so,
                                       _p(None if bias is None else _f32(bias, "grouped_linear")), rows, G, Ig, Hg, 1 if relu else 0,
                                       GL_SHUFFLED if shuffle else GL_CAT, _p(_f32(out, "grouped_linear")), _stream()))
    return out


def grouped_linear_bwd_dx(dy: torch.Tensor, w: torch.Tensor, layout: str = "gih", y: Optional[torch.Tensor] = None,
                          shuffle: bool = False) -> torch.Tensor:
    """dx [rows, G * Ig] of grouped_linear; y: the saved output when the forward applied ReLU (its sign is the mask), else None."""
    G, Ig, Hg, (sg, si, so) = _gl_dims(w.shape, layout)
    rows = _gl_rows(dy, G * Hg, "dy")
    if y is not None and y.shape != dy.shape:
        raise RuntimeError(f"grouped_linear_bwd_dx: y {tuple(y.shape)} != dy {tuple(dy.shape)}")
    dx = torch.empty(rows, G * Ig, device=dy.device, dtype=torch.float32)
    check(lib.cruse_grouped_linear_bwd_dx(_p(_f32(dy, "grouped_linear_bwd_dx")), _p(None if y is None else _f32(y, "grouped_linear_bwd_dx")),
                                          _p(_f32(w, "grouped_linear_bwd_dx")), sg, si, so, rows, G, Ig, Hg, 0 if y is None else 1,
                                          GL_SHUFFLED if shuffle else GL_CAT, _p(dx), _stream()))
    return dx


def grouped_linear_bwd_dw(dy: torch.Tensor, x: torch.Tensor, w_shape, layout: str = "gih", y: Optional[torch.Tensor] = None,
                          shuffle: bool = False, want_db: bool = False, ws: Optional[torch.Tensor] = None):
    """(dw in the shape and layout of the weight, db [G * Hg] or None) of grouped_linear, all groups in one call; the row split and the
    order of its sums depend on the shape alone.  ws: cruse_grouped_linear_dw_ws_bytes bytes, taken here when None."""
    G, Ig, Hg, (sg, si, so) = _gl_dims(tuple(w_shape), layout)
    rows = _gl_rows(dy, G * Hg, "dy")
    if _gl_rows(x, G * Ig, "x") != rows:
        raise RuntimeError(f"grouped_linear_bwd_dw: x has {x.shape[0]} rows, dy {rows}")
    if y is not None and y.shape != dy.shape:
        raise RuntimeError(f"grouped_linear_bwd_dw: y {tuple(y.shape)} != dy {tuple(dy.shape)}")
    dw = torch.empty(tuple(w_shape), device=dy.device, dtype=torch.float32)
    db = torch.empty(G * Hg, device=dy.device, dtype=torch.float32) if want_db else None
    need = lib.cruse_grouped_linear_dw_ws_bytes(rows, G, Ig, Hg)
    if ws is None and need:
        ws = torch.empty(need // 4, device=dy.device, dtype=torch.float32)
    nbytes = 0 if ws is None else ws.numel() * ws.element_size()
    check(lib.cruse_grouped_linear_bwd_dw(_p(_f32(dy, "grouped_linear_bwd_dw")), _p(None if y is None else _f32(y, "grouped_linear_bwd_dw")),
                                          _p(_f32(x, "grouped_linear_bwd_dw")), rows, G, Ig, Hg, 0 if y is None else 1,
                                          GL_SHUFFLED if shuffle else GL_CAT, _p(dw), sg, si, so, _p(db), _p(ws), nbytes, _stream()))
    return dw, db


class GroupedLinearFn(torch.autograd.Function):
    """grouped_linear with its three gradients; x [rows, G * Ig], w in `layout`, bias [G * Hg] or None."""

    @staticmethod
    def forward(ctx, x, w, bias, layout, relu, shuffle):
        x, w = x.contiguous(), w.contiguous()
        y = grouped_linear(x, w, layout, None if bias is None else bias.contiguous(), relu, shuffle)
        ctx.cfg = (layout, bool(relu), bool(shuffle), tuple(w.shape), None if bias is None else tuple(bias.shape))
        if any(ctx.needs_input_grad[:3]):
            ng = ctx.needs_input_grad
            # x only for the weight gradient, w only for the input gradient, y only as the ReLU mask
            ctx.save_for_backward(x if (ng[1] or ng[2]) else None, w if ng[0] else None, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        layout, relu, shuffle, w_shape, b_shape = ctx.cfg
        dy = dy.contiguous()
        ng = ctx.needs_input_grad
        dx = grouped_linear_bwd_dx(dy, w, layout, y, shuffle) if ng[0] else None
        dw = db = None
        if ng[1] or ng[2]:
            dw, db = grouped_linear_bwd_dw(dy, x, w_shape, layout, y, shuffle, want_db=bool(ng[2]))
            if db is not None:
                db = db.view(b_shape)
        return dx, dw if ng[1] else None, db, None, None, None


def _band_args(t: torch.Tensor, starts: torch.Tensor, width: int, name: str):
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1:
        raise RuntimeError(f"{name}: expected [rows >= 1, {width}], got {tuple(t.shape)}")
    if starts.dtype != torch.int32 or starts.dim() != 1 or starts.numel() < 2 or starts.device != t.device:
        raise RuntimeError(f"{name}: the band table must be int32 [n_bands + 1] on {t.device}")
    return int(t.shape[0]), int(starts.numel()) - 1


def band_pool(x: torch.Tensor, starts: torch.Tensor, mean: bool) -> torch.Tensor:
    """y[r, b] = w_b * sum of x[r, starts[b]:starts[b + 1]], w_b = 1 / width_b with `mean`, else 1.  x [rows, F] -> [rows, n_bands]."""
    F = int(x.shape[-1])
    rows, nb = _band_args(x, starts, F, "band_pool")
    y = torch.empty(rows, nb, device=x.device, dtype=torch.float32)
    check(lib.cruse_band_pool(_p(_f32(x, "band_pool")), _p(starts), rows, F, nb, 1 if mean else 0, _p(y), _stream()))
    return y


def band_expand(m: torch.Tensor, starts: torch.Tensor, F: int, mean: bool) -> torch.Tensor:
    """y[r, f] = w_b * m[r, b] for the band b that holds bin f (0 where none does).  m [rows, n_bands] -> [rows, F]: band_pool's adjoint."""
    rows, nb = _band_args(m, starts, int(starts.numel()) - 1, "band_expand")
    y = torch.empty(rows, int(F), device=m.device, dtype=torch.float32)
    check(lib.cruse_band_expand(_p(_f32(m, "band_expand")), _p(starts), rows, int(F), nb, 1 if mean else 0, _p(y), _stream()))
    return y


class BandPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, starts, mean):
        ctx.starts, ctx.mean, ctx.F = starts, bool(mean), int(x.shape[-1])
        return band_pool(x.contiguous(), starts, mean)

    @staticmethod
    def backward(ctx, dy):
        return band_expand(dy.contiguous(), ctx.starts, ctx.F, ctx.mean), None, None


class BandExpandFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m, starts, F, mean):
        ctx.starts, ctx.mean = starts, bool(mean)
        return band_expand(m.contiguous(), starts, F, mean)

    @staticmethod
    def backward(ctx, dy):
        return band_pool(dy.contiguous(), ctx.starts, ctx.mean), None, None, None


# ---------------------------------------------------------------- DeepFilterNet's input features (cruse_df_feat)
DF_FEAT_TC = 64                          # CRUSE_DF_FEAT_TC: the kernel's frame tile (tests place their lengths around it)
DF_ERB_INIT = (-60.0, -90.0)             # DeepFilterNet's published initial ERB mean, linspace over the bands (not in the reference)
DF_UNIT_INIT = (0.001, 0.0001)           # ExponentialUnitNorm.UNIT_NORN_INIT (test/test_norm.py:43), linspace over the bins


def df_feat_states(B: int, nb_erb: int, nb_df: int, device):
    """(erb_state [B, nb_erb], unit_state [B, nb_df]) at their defaults, linspace(*DF_ERB_INIT) and linspace(*DF_UNIT_INIT); None for a
    feature of size 0"""
    def lin(init, n):
        return None if n == 0 else torch.linspace(init[0], init[1], n, dtype=torch.float32).to(device).repeat(int(B), 1)
    return lin(DF_ERB_INIT, int(nb_erb)), lin(DF_UNIT_INIT, int(nb_df))


def _df_planes(re: torch.Tensor, im: torch.Tensor):
    """(re, im, bin stride, frame stride) of two [B,T,F] planes that cruse_df_feat reads in place: element (b, t, f) at
    (b T + t) frame_stride + f bin_stride.  Planar tensors and the [..., 0] / [..., 1] views of an interleaved one are; anything else is
    copied."""
    B, T, F = re.shape

    def strides(t):
        es = t.stride(2) if F > 1 else 1
        fs = t.stride(1) if T > 1 else (t.stride(0) if B > 1 else (F - 1) * es + 1)
        ok = es >= 1 and fs >= (F - 1) * es + 1 and (B == 1 or T <= 1 or t.stride(0) == T * fs)
        return es, fs, ok
    er, fr, okr = strides(re)
    ei, fi, oki = strides(im)
    if okr and oki and (er, fr) == (ei, fi):
        return re, im, er, fr
    return re.contiguous(), im.contiguous(), 1, F


def df_feat(re: torch.Tensor, im: torch.Tensor, starts: Optional[torch.Tensor], nb_df: int, alpha: float,
            erb_state: Optional[torch.Tensor] = None, unit_state: Optional[torch.Tensor] = None, log_eps: float = 1e-10,
            erb_scale: float = 40.0, unit_eps: float = 1e-14, out=None, ws=None):
    """DeepFilterNet's two input features of a spectrum re, im [B,T,F] -> (feat_erb [B,T,nb_erb], feat_spec [B,T,nb_df,2]), one kernel
    (include/cruse_hip.h states the formulas).  starts: the int32 [nb_erb + 1] device band table (cust_conv._band_table), or None: no ERB
    feature, feat_erb is None.  nb_df = 0: feat_spec is None.  erb_state [B,nb_erb] / unit_state [B,nb_df]: the state before the first
    frame, overwritten with the state after the last; absent, the call starts from df_feat_states' defaults in a temporary.  re, im may
    be the [..., 0] and [..., 1] views of an interleaved [B,T,F,2] tensor: they are read in place.  out = (feat_erb, feat_spec): write
    into these.  ws: accepted and unused, the kernel needs no workspace.  Inference only: an input that requires grad raises."""
    if re.requires_grad or im.requires_grad:
        raise RuntimeError("df_feat is inference-only (no backward kernel): the spectrum requires grad")
    if re.dim() != 3 or im.shape != re.shape or re.dtype != torch.float32 or im.dtype != torch.float32 or re.device != im.device:
        raise RuntimeError(f"df_feat: re and im must be float32 [B,T,F] of one shape and device, got {re.dtype} {tuple(re.shape)} and "
                           f"{im.dtype} {tuple(im.shape)}")
    B, T, F = (int(v) for v in re.shape)
    if B < 1 or F < 1 or F > BAND_MAX_F:
        raise RuntimeError(f"df_feat: B = {B}, F = {F}: at least one clip and 1..{BAND_MAX_F} bins")
    nb_df = int(nb_df)
    if nb_df < 0 or nb_df > F:
        raise RuntimeError(f"df_feat: nb_df = {nb_df} outside 0..F = {F}")
    nb_erb = 0
    if starts is not None:
        if starts.dtype != torch.int32 or starts.dim() != 1 or starts.numel() < 2 or starts.device != re.device or not starts.is_contiguous():
            raise RuntimeError(f"df_feat: the band table must be contiguous int32 [nb_erb + 1] on {re.device}")
        nb_erb = int(starts.numel()) - 1
        if nb_erb > F:
            raise RuntimeError(f"df_feat: nb_erb = {nb_erb} bands over F = {F} bins")
    if nb_erb == 0 and nb_df == 0:
        raise RuntimeError("df_feat: no output is requested (starts is None and nb_df = 0)")
    alpha = float(alpha)
    if not 0.0 <= alpha < 1.0:
        raise RuntimeError(f"df_feat: alpha = {alpha} outside [0, 1)")
    dflt = None
    states = []
    for name, st, n in (("erb_state", erb_state, nb_erb), ("unit_state", unit_state, nb_df)):
        if n == 0:
            st = None
        elif st is None:
            dflt = dflt or df_feat_states(B, nb_erb, nb_df, re.device)
            st = dflt[len(states)]
        elif st.dtype != torch.float32 or tuple(st.shape) != (B, n) or not st.is_contiguous() or st.device != re.device:
            raise RuntimeError(f"df_feat: {name} must be contiguous float32 [{B}, {n}] on {re.device}, got {st.dtype} {tuple(st.shape)}")
        states.append(st)
    outs = []
    for i, (name, shape) in enumerate((("feat_erb", (B, T, nb_erb)), ("feat_spec", (B, T, nb_df, 2)))):
        o = None if out is None else out[i]
        if shape[2] == 0:
            o = None
        elif o is None:
            o = torch.empty(shape, device=re.device, dtype=torch.float32)
        elif o.dtype != torch.float32 or tuple(o.shape) != shape or not o.is_contiguous() or o.device != re.device:
            raise RuntimeError(f"df_feat: out {name} must be contiguous float32 {list(shape)} on {re.device}, got {o.dtype} {tuple(o.shape)}")
        outs.append(o)
    if not re.is_cuda:
        raise RuntimeError("cruse_amd ops need tensors on the HIP device (no CPU fallback)")
    if T == 0:                                                            # nothing to write, the states stay
        return outs[0], outs[1]
    re, im, es, fs = _df_planes(re, im)
    check(lib.cruse_df_feat(re.data_ptr(), im.data_ptr(), es, fs, B, T, F, _p(starts), nb_erb, nb_df, alpha, float(log_eps), float(erb_scale),
                            float(unit_eps), _p(states[0]), _p(states[1]), _p(outs[0]), _p(outs[1]), _stream()))
    return outs[0], outs[1]


# ======================================================================================================================
# per-file statistics of a pool of recordings (cruse_screen_clips, cruse_rt60; cruse_amd/screen.py builds the reference's list builder
# dataset/preprocess_dataset.py on them)
# ======================================================================================================================
SCREEN_COLUMNS = ("peak", "n_clipped", "rms", "n_windows", "n_active", "activity")
RT60_COLUMNS = ("rt60", "t_peak", "edc_floor_db")


class RaggedPlan:
    """Where the utterances of a flat pool lie: the HOST tables (judged here: 0 <= start, 0 <= len, start + len <= pool_len) and their
    device copies, made once; the per-window-size prefix tables and the workspaces of the two kernels are built on first use and kept,
    so a call that is handed its plan allocates and copies nothing (it captures into a HIP graph)."""

    def __init__(self, pool_len: int, start, length, device):
        import numpy as np
        dev_in = [t if isinstance(t, torch.Tensor) and t.is_cuda else None for t in (start, length)]
        host = [np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in (start, length)]
        host = [h.astype(np.int64) if h.size == 0 else h for h in host]       # an empty list has no integer type of its own
        for h, name in zip(host, ("start", "length")):
            if h.ndim != 1 or h.dtype.kind not in "iu":
                raise ValueError(f"screen: {name} must be a flat integer table, got {h.dtype} {h.shape}")
        self.start_h, self.len_h = (h.astype(np.int64) for h in host)
        if self.start_h.shape != self.len_h.shape:
            raise ValueError(f"screen: start {self.start_h.shape} and length {self.len_h.shape} differ")
        if np.any(self.start_h < 0) or np.any(self.len_h < 0) or np.any(self.start_h + self.len_h > int(pool_len)):
            raise ValueError(f"screen: an utterance leaves the pool [0, {int(pool_len)})")
        self.n, self.pool_len, self.device = int(self.start_h.shape[0]), int(pool_len), torch.device(device)
        self.max_len = int(self.len_h.max()) if self.n else 0
        dev = []
        for t, h in zip(dev_in, (self.start_h, self.len_h)):
            if t is None or t.dtype != torch.int64 or not t.is_contiguous():
                t = torch.from_numpy(h).to(self.device)
            dev.append(t)
        self.start, self.length = dev
        self._windows = {}
        self._rt60_ws = None

    def windows(self, window: int):
        """-> (win_first int64 [n + 1] on the device, total windows, the window pass's workspace)"""
        import numpy as np
        window = int(window)
        if window not in self._windows:
            first = np.concatenate([[0], np.cumsum(-(-self.len_h // max(window, 1)))]).astype(np.int64)
            total = int(first[-1])
            nbytes = lib.cruse_screen_ws_bytes(self.n, total)
            if nbytes < 0:
                raise RuntimeError(f"screen_clips: {self.n} utterances in {total} windows of {window} samples are refused "
                                   "(cruse_screen_ws_bytes)")
            self._windows[window] = (torch.from_numpy(first).to(self.device), total,
                                     torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device))
        return self._windows[window]

    def rt60_ws(self):
        if self._rt60_ws is None:
            nbytes = lib.cruse_rt60_ws_bytes(self.n, self.max_len)
            if nbytes < 0:
                raise RuntimeError(f"rt60: {self.n} responses of up to {self.max_len} samples are refused (cruse_rt60_ws_bytes)")
            self._rt60_ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        return self._rt60_ws


def ragged_plan(pool: torch.Tensor, start, length) -> RaggedPlan:
    """start / length: host sequences or numpy arrays (validated, copied to the device once), or int64 device tensors (read back once
    for the validation, then used as they are)"""
    if pool.dim() != 1:
        raise RuntimeError(f"screen: the pool must be flat, got {tuple(pool.shape)}")
    return RaggedPlan(pool.numel(), start, length, pool.device)


def _screen_out(out, n: int, cols: int, device, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty(n, cols, device=device, dtype=torch.float64)
    if out.shape != (n, cols) or out.dtype != torch.float64 or out.device != device:
        raise RuntimeError(f"{name}: out must be float64 [{n}, {cols}] on {device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    return out


def _screen_plan(pool, start, length, plan, name):
    _f32(pool, name)
    if plan is None:
        plan = ragged_plan(pool, start, length)
    elif plan.pool_len != pool.numel() or plan.device != pool.device:
        raise RuntimeError(f"{name}: the plan was made for a pool of {plan.pool_len} samples on {plan.device}")
    return plan


def screen_clips(pool: torch.Tensor, start=None, length=None, sr: int = 16000, clip_threshold: float = 0.999, target_dB_FS: float = -25.0,
                 activity_threshold: float = 0.13, plan: Optional[RaggedPlan] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per utterance pool[start[i] : start[i] + length[i]] -> float64 [n, 6] on the device, columns SCREEN_COLUMNS: peak = max |x| and
    n_clipped = #{|x| > clip_threshold} (feature.is_clipped is n_clipped > 0), rms (feature.tailor_dB_FS), and n_windows, n_active,
    activity = feature.activity_detector's perc_active over windows of int(sr * 0.05) samples, in float64 (include/cruse_hip.h states the
    formulas).  An empty utterance gives 0, 0, 0, 0, 0, NaN.  `plan`: ragged_plan(pool, start, length) made beforehand -- with it and
    `out` the call copies and allocates nothing."""
    plan = _screen_plan(pool, start, length, plan, "screen_clips")
    out = _screen_out(out, plan.n, len(SCREEN_COLUMNS), pool.device, "screen_clips")
    if plan.n == 0:
        return out
    window = int(sr * 0.05)
    first, total, ws = plan.windows(window)
    check(lib.cruse_screen_clips(_p(pool), _p(plan.start), _p(plan.length), _p(first), plan.n, total, window, float(clip_threshold),
                                 float(target_dB_FS), float(activity_threshold), _p(ws), _p(out), _stream()))
    return out


def rt60(pool: torch.Tensor, start=None, length=None, sr: int = 16000, lo_db: float = -5.0, hi_db: float = -25.0,
         plan: Optional[RaggedPlan] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reverberation time of every impulse response pool[start[i] : start[i] + length[i]] -> float64 [n, 3] on the device, columns
    RT60_COLUMNS: from the peak t_peak on, Schroeder's backward integral E[t] = sum_{m >= t} h[m]^2, D = 10 log10(E / E[t_peak]), a
    least-squares line through D where lo_db >= D > hi_db, rt60 = -60 / (slope sr); edc_floor_db = D at the last sample.  The defaults
    are T20 (ISO 3382-2).  NaN for an empty or all-zero response, a range of fewer than 2 points and a decay that never reaches hi_db.

    Departure from the reference's utils.cal_rt60 (utils/utils.py:270-320), which cannot run (stats.Linregress; a band mask that zeroes
    every bin below hifreq): its 15 third-octave brick-wall bands, 2500-sample smoothing of |h| in dB and median over bands are not
    restated.  The quantity here is the BROADBAND T20 of the energy decay curve; banded RT60 is not built."""
    plan = _screen_plan(pool, start, length, plan, "rt60")
    out = _screen_out(out, plan.n, len(RT60_COLUMNS), pool.device, "rt60")
    if plan.n == 0:
        return out
    check(lib.cruse_rt60(_p(pool), _p(plan.start), _p(plan.length), plan.n, plan.max_len, int(sr), float(lo_db), float(hi_db),
                         _p(plan.rt60_ws()), _p(out), _stream()))
    return out
