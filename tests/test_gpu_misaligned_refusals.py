"""GPU: the alignment refusals of the C ABI, each triggered by a call that violates that requirement alone.

One test per refusal site.  The call is otherwise valid and made on device buffers; the one operand starts a few bytes after a 16-byte
boundary (tests/misalign.py, which asserts the residue).  Asserted of every call: the documented code comes back (CRUSE_E_ALIGN; the h0
requirement of the forward recurrence documents CRUSE_E_SHAPE), cruse_last_error() names the entry point and the operand (where one
check covers several operands its message lists them all, so the name alone does not tell which one was off), and after a device sync every output
and workspace still holds the sentinel it was filled with -- the refusal came before anything was launched.  DESIGN.md (alignment audit)
lists the sites."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from misalign import place  # noqa: E402

pytestmark = pytest.mark.gpu
E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -3
DT_F16, DT_BF16 = 1, 2


@pytest.fixture(scope="module")
def hip():
    from cruse_amd._lib import lib
    return lib


def st():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def f32(n, k=0):
    """n floats of input, the view k floats after a 16-byte boundary"""
    return place(np.linspace(-1.0, 1.0, n, dtype=np.float32), k)


def u16(n, k=0):
    return place(np.full(n, 0x3F80, np.uint16), k)


def out(n, k=0, dtype=np.float32):
    """an output or workspace of n elements, left as sentinels"""
    return place(np.zeros(n, dtype), k, sentinel=True)


def refused(hip, name, args, code, names, outs):
    rc = getattr(hip, name)(*args, st())
    msg = (hip.cruse_last_error() or b"").decode()
    sync()
    assert rc == code, (name, rc, msg)
    assert all(n in msg for n in names), (name, msg, names)
    assert all(o.untouched() for o in outs), (name, msg, "an output or workspace was written")


def each(names, misaligned):
    """(operand, {operand: offset}) for each operand misaligned alone"""
    return [(n, {**dict.fromkeys(names, 0), n: misaligned[n] if isinstance(misaligned, dict) else misaligned}) for n in names]


def test_wave_l1_mse(hip):                                     # tdloss.hip, cruse_wave_l1_mse
    n = 64
    for who, k in each(("est", "ref", "dest"), 1):
        ls, dest = out(1, dtype=np.float64), out(n, k["dest"])
        refused(hip, "cruse_wave_l1_mse", (f32(n, k["est"]).ptr, f32(n, k["ref"]).ptr, n, 0, 1.0, ls.ptr, dest.ptr), E_ALIGN, ("wave_l1_mse", who),
                (ls, dest))


def test_sumsq(hip):                                           # pointwise.hip, cruse_sumsq
    o = out(1, dtype=np.float64)
    refused(hip, "cruse_sumsq", (f32(64, 1).ptr, 64, o.ptr, 0), E_ALIGN, ("sumsq", "x"), (o,))


def test_layernorm_forward_refuses_before_it_launches(hip):   # pointwise.hip, cruse_ln_fwd_c: the two checks that used to follow the launch
    rows, H = 8, 64
    x, gamma, beta = f32(rows * H), f32(H), f32(H)

    def call(copy_k, copy_dtype, ig, seg, code, names):
        y, yc, mean, rstd = out(rows * H), out(rows * H, copy_k, np.uint16), out(rows), out(rows)
        refused(hip, "cruse_ln_fwd_c", (x.ptr, gamma.ptr, beta.ptr, None, y.ptr, yc.ptr, copy_dtype, mean.ptr, rstd.ptr, rows, H, ig, 1e-5) + seg,
                code, names, (y, yc, mean, rstd))
    for k in (1, 2, 3):
        call(k, DT_BF16, 1, (4, 8, 2), E_ALIGN, ("ln_fwd", "y_bf16"))       # row segments with a copy the vector kernel cannot write itself
        call(k, DT_F16, 1, (0, 0, 0), E_DTYPE, ("ln_fwd", "f16 copy"))      # the f16 copy, which the separate pass does not make
    call(0, DT_F16, 2, (0, 0, 0), E_DTYPE, ("ln_fwd", "f16 copy"))          # ... nor does the interleaved form


def gemm_operands(M=64, N=64, K=128):
    return M, N, K, u16(M * K), u16(N * K)


def test_gemm_bf16_operands(hip):                              # gemm_bf16.hip, gemm_run: 16-byte aligned rows and k-tiles
    M, N, K = 64, 64, 128
    for who, k in each(("A", "B"), 4):
        C = out(M * N)
        refused(hip, "cruse_gemm_bf16_nt", (M, N, K, u16(M * K, k["A"]).ptr, K, 64, u16(N * K, k["B"]).ptr, K, 64, C.ptr, N, None, 0, 1), E_ALIGN,
                ("gemm_bf16_nt", f"{who} must be 16-byte aligned"), (C,))


def test_gemm_bf16_slab_scratch(hip):                          # gemm_bf16.hip, gemm_run: the slab form's scratch
    M, N, K, A, B = gemm_operands()
    nbytes = hip.cruse_gemm_bf16_slab_bytes(M, N, 2)
    C, scratch = out(M * N), out(nbytes // 4, 1)
    refused(hip, "cruse_gemm_bf16_nt_slabs", (M, N, K, A.ptr, K, 64, B.ptr, K, 64, C.ptr, N, 2, scratch.ptr, nbytes), E_ALIGN,
            ("gemm_bf16_nt", "slab scratch"), (C, scratch))


def test_gemm_bf16_low_planes(hip):                            # gemm_bf16.hip, gemm_enter: the four forms that take low planes
    M, N, K, A, B = gemm_operands()
    lo = u16(N * K, 4)
    C = out(M * N)
    refused(hip, "cruse_gemm_bf16x3_nt", (M, N, K, A.ptr, None, K, 64, B.ptr, lo.ptr, K, 64, C.ptr, N, None, 0), E_ALIGN,
            ("gemm_bf16x3_nt", "low planes"), (C,))
    C16 = out(M * N, dtype=np.uint16)
    refused(hip, "cruse_gemm_nt_out16", (M, N, K, A.ptr, None, K, 64, B.ptr, lo.ptr, K, 64, C16.ptr, N, None, 0, DT_BF16), E_ALIGN,
            ("gemm_nt_out16", "low planes"), (C16,))
    refused(hip, "cruse_gemm_bf16_nt_groups", (M, N, K, 1, A.ptr, None, K, 0, B.ptr, lo.ptr, K, 64, 0, C.ptr, N, N, None, 0, 0), E_ALIGN,
            ("gemm_bf16_nt_groups", "low planes"), (C,))
    refused(hip, "cruse_gemm_bf16_nt_seg", (M, N, K, A.ptr, None, K, B.ptr, lo.ptr, K, 64, C.ptr, N, None, 0, 32, 32, 0), E_ALIGN,
            ("gemm_bf16_nt_seg", "low planes"), (C,))


def test_cast_bf16(hip):                                       # gemm_bf16.hip, cruse_cast_bf16_split
    n = 64
    for who, k in each(("x", "y", "y_lo"), 1):
        y, lo = out(n, k["y"], np.uint16), out(n, k["y_lo"], np.uint16)
        refused(hip, "cruse_cast_bf16_split", (f32(n, k["x"]).ptr, y.ptr, lo.ptr, n), E_ALIGN, ("cast_bf16", who), (y, lo))


def test_transpose_bf16(hip):                                  # gemm_bf16.hip, cruse_transpose_bf16
    rows, cols = 10, 8
    yT = out(64 * cols, 4, np.uint16)
    refused(hip, "cruse_transpose_bf16", (f32(rows * cols).ptr, rows, cols, cols, yT.ptr, 64, 0), E_ALIGN, ("transpose_bf16", "yT"), (yT,))


def test_ktile(hip):                                           # gemm_bf16.hip, cruse_ktile_bf16 and ktile_f16_impl
    rows, cols = 4, 64
    x = f32(rows * cols)
    for who, k in each(("y", "y_lo"), 1):
        y, lo = out(rows * cols, k["y"], np.uint16), out(rows * cols, k["y_lo"], np.uint16)
        refused(hip, "cruse_ktile_bf16", (x.ptr, rows, cols, cols, y.ptr, lo.ptr), E_ALIGN, ("ktile_bf16", who), (y, lo))
        refused(hip, "cruse_ktile_f16_split", (x.ptr, rows, cols, cols, y.ptr, lo.ptr), E_ALIGN, ("ktile_f16", who), (y, lo))


def test_mask_head(hip):                                       # mask_head.hip, cruse_mask_head_fwd_bwd
    B, T, C, F1 = 1, 2, 4, 8
    Fs, n, rows = 2 * F1 + 1, B * T * C * F1, B * T
    sums, gamma, beta, w, spec = place(np.ones(2 * C)), f32(C), f32(C), f32(C * 3), f32(rows * Fs)
    for who, k in each(("v", "skip", "u", "du", "mask", "dlogit"), 1):
        u, du, mean, rstd = out(n, k["u"]), out(n, k["du"]), out(C), out(C)
        mask, dlogit = out(rows * 2 * F1, k["mask"]), out(rows * 2 * F1, k["dlogit"])
        loss, bsums = out(1, dtype=np.float64), out(2 * C, dtype=np.float64)
        refused(hip, "cruse_mask_head_fwd_bwd",
                (f32(n, k["v"]).ptr, sums.ptr, 1, 1e-5, 0.1, gamma.ptr, beta.ptr, f32(n, k["skip"]).ptr, w.ptr, None, spec.ptr, spec.ptr, spec.ptr,
                 B, T, C, F1, Fs, 2.0, 1.0, u.ptr, mean.ptr, rstd.ptr, None, None, mask.ptr, dlogit.ptr, du.ptr, loss.ptr, 0, bsums.ptr, 1, 0, 0),
                E_ALIGN, ("mask_head", who), (u, du, mean, rstd, mask, dlogit, loss, bsums))


def test_gru_initial_state(hip):                               # gru.hip, gru_seq_fwd_impl: h0 (documented as CRUSE_E_SHAPE)
    B, T, G, Hg = 2, 3, 1, 32
    w, b = f32(3 * Hg * Hg), f32(3 * Hg)
    wa, ba = (ctypes.c_void_p * 1)(w.ptr), (ctypes.c_void_p * 1)(b.ptr)
    h, coef, an, z = out(B * T * Hg), out(B * T * 3 * Hg), out(B * T * Hg), out(B * T * Hg)
    ws, status = out(hip.cruse_gru_ws_bytes(B, G, Hg), dtype=np.uint8), out(64)
    refused(hip, "cruse_gru_seq_fwd_ex",
            (f32(B * T * 3 * Hg).ptr, ctypes.cast(wa, ctypes.c_void_p), ctypes.cast(ba, ctypes.c_void_p), h.ptr, coef.ptr, an.ptr, z.ptr, f32(B * Hg, 1).ptr,
             Hg, B, T, T, G, Hg, 0, 0, ws.ptr, 0, status.ptr, 0), E_SHAPE, ("gru_seq_fwd", "h0"), (h, coef, an, z, ws, status))


def test_gru_gate_grads_bf16(hip):                             # gru.hip, cruse_gru_gate_grads_bf16
    rows, G, Hg, ldT = 5, 1, 32, 64
    for who, k in each(("dh", "an", "coef", "dgi", "dgT"), dict(dh=1, an=1, coef=1, dgi=1, dgT=4)):
        dgi, dgT = out(rows * 3 * Hg, k["dgi"], np.uint16), out(ldT * 4 * Hg, k["dgT"], np.uint16)
        refused(hip, "cruse_gru_gate_grads_bf16", (f32(rows * Hg, k["dh"]).ptr, u16(rows * 3 * Hg, k["coef"]).ptr, f32(rows * Hg, k["an"]).ptr, dgi.ptr,
                                                   dgT.ptr, ldT, None, None, rows, G, Hg), E_ALIGN, ("gru_gate_grads_bf16", who), (dgi, dgT))


def test_biquad_coefficients(hip):                             # biquad.hip, cruse_biquad_cascade: f64 coefficients 4 bytes off
    B, L, S = 1, 100, 2
    y = out(B * L)
    refused(hip, "cruse_biquad_cascade", (f32(B * L).ptr, f32(2 * 6 * S, 1).ptr, 0, B, L, S, 0, None, y.ptr), E_ALIGN, ("biquad_cascade", "coef"), (y,))


def test_fftconv_spectra_and_workspace(hip):                   # fftconv.hip, cruse_fftconv_prepare and cruse_fftconv_apply
    B, L, NR, R = 1, 64, 1, 8
    nspec, nws = hip.cruse_fftconv_spec_bytes(NR, R, 0), hip.cruse_fftconv_ws_bytes(B, L)
    assert nspec > 0 and nws > 0
    spec = out(nspec // 4, 1)
    refused(hip, "cruse_fftconv_prepare", (f32(NR * R).ptr, NR, R, None, spec.ptr, nspec), E_ALIGN, ("fftconv_prepare", "spec"), (spec,))
    for who, k in each(("spec", "ws"), 1):
        spec, ws, y = out(nspec // 4, k["spec"]), out(nws // 4, k["ws"]), out(B * L)
        refused(hip, "cruse_fftconv_apply", (f32(B * L).ptr, B, L, spec.ptr, nspec, NR, R, None, ws.ptr, nws, y.ptr, None), E_ALIGN,
                ("fftconv_apply", who), (spec, ws, y))


def test_df_feat_spectrum_output(hip):                         # df_feat.hip, cruse_df_feat: the interleaved (re, im) pairs
    B, T, F, nb_df = 1, 2, 8, 4
    state, feat = out(B * nb_df), out(B * T * nb_df * 2, 1)
    refused(hip, "cruse_df_feat", (f32(B * T * F).ptr, f32(B * T * F).ptr, 1, F, B, T, F, None, 0, nb_df, 0.9, 1e-10, 1.0, 1e-10, None, state.ptr, None,
                                   feat.ptr), E_ALIGN, ("df_feat", "feat_spec"), (state, feat))


def test_stoi_workspace(hip):                                  # metrics.hip, stoi_run (cruse_stoi and cruse_stoi_ragged share it)
    B, L = 1, 4000
    nws = hip.cruse_stoi_ws_bytes(B, L)
    assert nws > 0
    ws, o = out(nws // 4 + 1, 1), out(B)
    refused(hip, "cruse_stoi", (f32(B * L).ptr, f32(B * L).ptr, B, L, f32(64).ptr, ws.ptr, nws, o.ptr), E_ALIGN, ("stoi", "workspace"), (ws, o))


def test_sdr_workspace_and_debug_buffer(hip):                  # sdr.hip, cruse_sdr
    B, L, K = 1, 600, 8
    nws = hip.cruse_sdr_ws_bytes(B, L, K)
    assert nws > 0
    for who, k in each(("workspace", "dbg"), 1):
        ws, o, dbg = out(nws // 4 + 1, k["workspace"]), out(B), out(2 * B * (3 * K + 2), k["dbg"])
        refused(hip, "cruse_sdr", (f32(B * L).ptr, f32(B * L).ptr, None, B, L, K, ws.ptr, o.ptr, dbg.ptr), E_ALIGN, ("sdr", who), (ws, o, dbg))


def test_snr_mix_scratch(hip):                                 # extras.hip, cruse_snr_mix
    B, L = 2, 100
    scratch, noisy = out(B * 6, 1), out(B * L)
    refused(hip, "cruse_snr_mix", (f32(B * L).ptr, f32(B * L).ptr, f32(B).ptr, B, L, 1e-8, scratch.ptr, None, None, noisy.ptr), E_ALIGN,
            ("snr_mix", "scratch"), (scratch, noisy))


def test_resample_tap_table(hip):                              # resample.hip, cruse_resample_poly
    L, up, down = 50, 2, 1
    ntap, stride = 32 * up + 1, 36                             # T = ceil((32 q + 1) / up) = 33 taps per phase, rows a multiple of 4 floats apart
    hin, hout = (ctypes.c_longlong * 2)(0, L), (ctypes.c_longlong * 2)(0, L * up)
    din, dout = place(np.array([0, L], np.int64).view(np.float64)), place(np.array([0, L * up], np.int64).view(np.float64))
    o = out(L * up)
    refused(hip, "cruse_resample_poly", (f32(L).ptr, 0, 1, 0, ctypes.cast(hin, ctypes.c_void_p), ctypes.cast(hout, ctypes.c_void_p), din.ptr, dout.ptr, 1, up, down,
                                         f32(up * stride, 1).ptr, ntap, stride, o.ptr), E_ALIGN, ("resample_poly", "tap table"), (o,))


def test_grouped_linear_weight_gradient_workspace(hip):        # grouped_linear.hip, cruse_grouped_linear_bwd_dw
    rows, G, Ig, Hg = 1024, 1, 8, 8
    need = hip.cruse_grouped_linear_dw_ws_bytes(rows, G, Ig, Hg)
    assert need > 0                                            # several row parts: the shape does use the workspace
    ws, dw, db = out(need + 16, 2, np.uint8), out(Ig * Hg), out(Hg)
    refused(hip, "cruse_grouped_linear_bwd_dw", (f32(rows * Hg).ptr, None, f32(rows * Ig).ptr, rows, G, Ig, Hg, 0, 0, dw.ptr, Ig * Hg, Hg, 1, db.ptr, ws.ptr,
                                                 need), E_ALIGN, ("grouped_linear_bwd_dw", "workspace"), (ws, dw, db))


def test_f64_sum_buffers(hip):
    """the double* sums, on which the kernels do 8-byte atomics and loads: 4 bytes off is refused by every entry point that takes one
    (pointwise.hip, tdloss.hip, mask_head.hip); every caller in the package passes them from the allocator"""
    rows, C, F = 4, 4, 8
    n = rows * C * F
    y, vec = f32(n), f32(C)

    def d(k=1):                                               # 2 * C doubles, 4 bytes off
        return out(4 * C + 2, k)
    s, o = d(), out(n)
    refused(hip, "cruse_bn_stats", (y.ptr, rows, C, F, s.ptr, 0), E_ALIGN, ("bn_stats", "sums"), (s,))
    s, m, r = d(), out(C), out(C)
    refused(hip, "cruse_bn_finalize", (s.ptr, rows * F, C, 1e-5, 0.1, m.ptr, r.ptr, None, None), E_ALIGN, ("bn_finalize", "sums"), (m, r))
    s, m, r = d(), out(C), out(C)
    refused(hip, "cruse_bn_finalize_act_fwd", (y.ptr, s.ptr, 1, rows * F, 1e-5, 0.1, vec.ptr, vec.ptr, None, o.ptr, None, m.ptr, r.ptr, None, None, rows,
                                               C, F, 1), E_ALIGN, ("bn_finalize_act_fwd", "sums"), (o, m, r))
    s = d()
    refused(hip, "cruse_bn_act_bwd_reduce", (y.ptr, y.ptr, vec.ptr, vec.ptr, vec.ptr, vec.ptr, rows, C, F, 1, s.ptr, 0), E_ALIGN,
            ("bn_act_bwd_reduce", "sums"), (s,))
    s, dy, dg, db = d(), out(n), out(C), out(C)
    refused(hip, "cruse_bn_act_bwd_apply", (y.ptr, y.ptr, vec.ptr, vec.ptr, vec.ptr, vec.ptr, s.ptr, 1, rows, C, F, 1, 1, 0, dy.ptr, 0, dg.ptr, db.ptr, None),
            E_ALIGN, ("bn_act_bwd_apply", "sums"), (dy, dg, db))
    Fn, Fs = 8, 9
    ls, dm, dl = out(4, 1), out(rows * Fn), out(rows * Fn)
    refused(hip, "cruse_mask_loss_fwd", (f32(rows * Fn).ptr, f32(rows * Fs).ptr, f32(rows * Fs).ptr, f32(rows * Fs).ptr, rows, Fn, Fs, 2.0, 1.0, ls.ptr,
                                         dm.ptr, dl.ptr, None, None), E_ALIGN, ("mask_loss", "loss_sum"), (ls, dm, dl))
    ls = out(4, 1)
    refused(hip, "cruse_sumsq", (f32(64).ptr, 64, ls.ptr, 0), E_ALIGN, ("sumsq", "out"), (ls,))
    acc = out(10, 1)
    refused(hip, "cruse_accum_f64", (acc.ptr, place(np.ones(4)).ptr, 4), E_ALIGN, ("accum_f64", "acc"), (acc,))
    ls, dest = out(4, 1), out(64)
    refused(hip, "cruse_wave_l1_mse", (f32(64).ptr, f32(64).ptr, 64, 0, 1.0, ls.ptr, dest.ptr), E_ALIGN, ("wave_l1_mse", "loss_sum"), (ls, dest))


def test_mask_head_f64_sums(hip):                              # mask_head.hip: bn_sums, loss_sum, bwd_sums (8-byte atomics)
    B, T, C, F1 = 1, 2, 4, 8
    Fs, n, rows = 2 * F1 + 1, B * T * C * F1, B * T
    gamma, beta, w, spec, v = f32(C), f32(C), f32(C * 3), f32(rows * Fs), f32(n)
    for who, k in each(("bn_sums", "loss_sum", "bwd_sums"), 1):
        u, du, mean, rstd = out(n), out(n), out(C), out(C)
        mask, dlogit = out(rows * 2 * F1), out(rows * 2 * F1)
        sums, loss, bsums = f32(4 * C + 2, k["bn_sums"]), out(4, k["loss_sum"]), out(4 * C + 2, k["bwd_sums"])
        refused(hip, "cruse_mask_head_fwd_bwd",
                (v.ptr, sums.ptr, 1, 1e-5, 0.1, gamma.ptr, beta.ptr, v.ptr, w.ptr, None, spec.ptr, spec.ptr, spec.ptr,
                 B, T, C, F1, Fs, 2.0, 1.0, u.ptr, mean.ptr, rstd.ptr, None, None, mask.ptr, dlogit.ptr, du.ptr, loss.ptr, 0, bsums.ptr, 1, 0, 0),
                E_ALIGN, ("mask_head", who), (u, du, mean, rstd, mask, dlogit, loss, bsums))


def test_conv_operands_with_wide_accesses(hip):
    """conv.hip, conv_aligned: the operands of the ten convolution entry points on which a kernel does 8- or 16-byte accesses without
    choosing a route from the address (f64 sums, the scatter kernels' pair stores, bn_y, in_add, the bf16 copies, the fused
    BatchNorm-backward input), each misaligned alone: refused ahead of every launch, the memset of the sums included"""
    B, T, Cin, Fin, Cout, Fout, KT, S, pad = 1, 2, 8, 16, 16, 8, 2, 2, 1
    nx, ny = B * T * Cin * Fin, B * T * Cout * Fout
    x, w, bias, cv, ci = f32(nx), f32(Cout * Cin * KT * 3), f32(Cout), f32(Cout), f32(Cin)
    geom = (B, T, Cin, Fin, Cout, Fout, KT, S, pad)

    def sums(k=0):
        return out(2 * 2 * Cout * 64 + 2, k)                  # room for every replica of the f64 sums
    y, s = out(ny), sums(1)
    refused(hip, "cruse_conv_gather_bnstats", (x.ptr, w.ptr, bias.ptr, y.ptr) + geom + (-1, s.ptr, 0), E_ALIGN, ("conv_gather_bnstats", "sums"), (y, s))
    y = out(ny, 1)                                            # scatter2: Cs 8, Fg 4 -> Cout 16, Fout 8
    refused(hip, "cruse_conv_scatter2", (f32(B * T * 8 * 4).ptr, f32(8 * Cout * 3).ptr, bias.ptr, y.ptr, B, T, 8, 4, Cout, 8, 1, 0, 0, 0, -1, 0, 0), E_ALIGN,
            ("conv_scatter2", "out"), (y,))
    for k in (1, 2):
        y, s = out(ny), sums()
        refused(hip, "cruse_conv_gather_bnbwd", (x.ptr, w.ptr, y.ptr) + geom + (0, 0, 2, f32(ny, k).ptr, cv.ptr, cv.ptr, cv.ptr, cv.ptr, 1, s.ptr, 0, 0, 0),
                E_ALIGN, ("conv_gather_bnbwd", "bn_y"), (y, s))
    for who, k in each(("in_sums", "in_add", "bf16 copy"), {"in_sums": 1, "in_add": 1, "bf16 copy": 4}):
        y, s, cp = out(ny), sums(), out(nx, k["bf16 copy"], np.uint16)
        refused(hip, "cruse_conv_gather_bnin", (x.ptr, f32(4 * Cin + 2, k["in_sums"]).ptr, 1, B * T * Fin, 1e-5, 0.1, ci.ptr, ci.ptr, None, None, None, None,
                                                f32(nx, k["in_add"]).ptr, cp.ptr, w.ptr, bias.ptr, y.ptr) + geom + (2, s.ptr, 0), E_ALIGN,
                ("conv_gather_bnin", who), (y, s, cp))
    for who, k in each(("bb_y", "bb_sums", "dy_bf16"), {"bb_y": 1, "bb_sums": 1, "dy_bf16": 4}):
        y, cp, dg = out(ny), out(nx, k["dy_bf16"], np.uint16), out(Cin)
        refused(hip, "cruse_conv_gather_bnbwd_in", (x.ptr, 0, f32(nx, k["bb_y"]).ptr, ci.ptr, ci.ptr, ci.ptr, ci.ptr, f32(4 * Cin + 2, k["bb_sums"]).ptr, 1, 1, 1,
                                                    cp.ptr, dg.ptr, dg.ptr, None, w.ptr, y.ptr) + geom + (0, 0, 2, None, None, None, None, None, 0, None, 0, 0),
                E_ALIGN, ("conv_gather_bnbwd_in", who), (y, cp, dg))
