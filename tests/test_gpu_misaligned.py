"""GPU: the kernel routes that the entry points choose from the low bits of a device pointer, on views that are NOT 16-byte aligned.

Every tensor the rest of the suite passes comes straight from torch's allocator and takes the aligned side of each
`(uintptr_t)p % 16` branch; here each operand in turn (then all of them) starts 1..3 floats (1..7 two-byte elements) after a 16-byte
boundary inside a sentinel-padded buffer (tests/misalign.py), which asserts the residue and, after the call, that both pads are intact.
The reference is float64 numpy on the same inputs; the bar of an entry point is the one its aligned test already holds
(test_gpu_abi_ref.py: cruse_gemm 2e-5 / 1e-5 bf16 on operands rounded alike, cruse_ln_fwd 3e-6 and 8e-3 for the bf16 copy, cruse_ln_bwd
2e-5; test_gpu_kernels.py: cruse_gemm_bf16_nt rel-L2 1e-6 and untouched margins, cruse_transpose_bf16 bit-exact;
test_gpu_grouped_linear.py: bands 1e-6; test_gpu_extras.py: upsample / downsum exact).  The 2-byte result rows of cruse_gemm_nt_out16 are
f32 sums rounded once at the store: |err| <= 2^-p |want| (p = 8 bf16, 11 f16: one rounding) + 1e-6 max |want| (the rel-L2 bar of the f32
result, which may move a value across a rounding boundary).  Each case prints its error / bar, the aligned one (all offsets 0) first.
Only operands whose alignment the host (or, for the GEMM result, the kernel) tests are moved; the refusals are in
test_gpu_misaligned_refusals.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from misalign import bf16_bits, bf16_round, bf16_value, max_rel, place, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu
DT_F16, DT_BF16 = 1, 2


@pytest.fixture(scope="module")
def hip():
    from cruse_amd._lib import lib
    return lib


def st():
    return torch.cuda.current_stream().cuda_stream


def run(hip, name, *args):
    rc = getattr(hip, name)(*args, st())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, hip.cruse_last_error())


def rnd(g, *shape, scale=1.0, shift=0.0):
    return np.ascontiguousarray((g.standard_normal(shape) * scale + shift).astype(np.float32))


class Tally:
    """prints error / bar of every case and keeps the worst ratio of the aligned and of the offset cases"""
    def __init__(self, what):
        self.what, self.worst, self.n = what, {"aligned": 0.0, "offset": 0.0}, {"aligned": 0, "offset": 0}

    def judge(self, case, offs, err, bar):
        kind = "offset" if any(offs.values()) else "aligned"
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        self.worst[kind] = max(self.worst[kind], ratio)
        self.n[kind] += 1
        print(f"{self.what} {case} offsets {offs}: error {err:.3e} / bar {bar:.1e} = {ratio:.3f}")
        assert err <= bar, (self.what, case, offs, err, bar)

    def done(self):
        print(f"{self.what}: worst error / bar aligned {self.worst['aligned']:.3f}, offset {self.worst['offset']:.3f}")
        assert self.n["aligned"] > 0 and self.n["offset"] > 0, self.n                  # both sides of the branch were run


def one_then_all(names, ks=(1,), zero=True):
    """offset dicts: all 0, each name alone at every k, then every name together at every k"""
    out = [dict.fromkeys(names, 0)] if zero else []
    for n in names:
        for k in ks:
            out.append({**dict.fromkeys(names, 0), n: k})
    for k in ks:
        out.append(dict.fromkeys(names, k))
    return out


def up4(n):
    return (n + 3) // 4 * 4


# ---- cruse_gemm: vecA / vecB = ld % 4 == 0 and a 16-byte aligned base (gemm.hip, cruse_gemm) -------------------------------------------
@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_operand_offsets_and_leading_dimensions(hip, tA, tB):
    M, N, K = 65, 33, 36
    g = np.random.default_rng(10 + 2 * tA + tB)
    ra, ca = (K, M) if tA else (M, K)                      # stored rows x used columns of A, of B
    rb, cb = (N, K) if tB else (K, N)
    ldc = N + 3
    bias, C0 = rnd(g, N), rnd(g, M, ldc)
    cases = [(o, up4(ca), up4(cb)) for o in one_then_all(("A", "B", "C"), (1, 2, 3))]
    cases += [(dict(A=0, B=0, C=0, lda=1), up4(ca) + 1, up4(cb)), (dict(A=0, B=0, C=0, ldb=1), up4(ca), up4(cb) + 1)]   # ld % 4 != 0, aligned base
    stored = {}
    tally = Tally(f"cruse_gemm tA={tA} tB={tB}")
    for offs, lda, ldb in cases:
        if (lda, ldb) not in stored:
            stored[(lda, ldb)] = (rnd(g, ra, lda), rnd(g, rb, ldb))
        As, Bs = stored[(lda, ldb)]
        for prec, bar in ((0, 2e-5), (2, 1e-5)):
            a64, b64 = (As[:, :ca], Bs[:, :cb]) if prec == 0 else (bf16_round(As[:, :ca]), bf16_round(Bs[:, :cb]))
            a64, b64 = a64.astype(np.float64), b64.astype(np.float64)
            prod = (a64.T if tA else a64) @ (b64.T if tB else b64)
            for form, use_bias, acc in (("bias", 1, 0), ("accumulate", 0, 1)):
                want = prod + (bias if use_bias else 0.0) + (C0[:, :N] if acc else 0.0)
                A, B, C, bs = place(As, offs["A"]), place(Bs, offs["B"]), place(C0, offs["C"]), place(bias)
                run(hip, "cruse_gemm", tA, tB, M, N, K, A.ptr, lda, B.ptr, ldb, C.ptr, ldc, bs.ptr if use_bias else None, acc, 1, 0, prec)
                got = C.get()
                assert all(p.pads_ok() for p in (A, B, C, bs)) and np.array_equal(got[:, N:], C0[:, N:]), (offs, prec, form)
                tally.judge(f"prec {prec} {form}", offs, max_rel(got[:, :N], want), bar)
    tally.done()


# ---- LayerNorm: the 4-byte kernels and the separate bf16 pass (pointwise.hip, cruse_ln_fwd_c / ln_bwd_impl) ---------------------------------
@pytest.mark.parametrize("H", (64, 100, 1024))
def test_layernorm_operand_offsets(hip, H):
    rows, eps = 5, 1e-5
    g = np.random.default_rng(H)
    x, res, dy = rnd(g, rows, H), rnd(g, rows, H), rnd(g, rows, H)
    gamma, beta = rnd(g, H, scale=0.3, shift=1.0), rnd(g, H, scale=0.2)
    x64 = x.astype(np.float64)
    m64 = x64.mean(1, keepdims=True)
    r64 = 1.0 / np.sqrt(((x64 - m64) ** 2).mean(1, keepdims=True) + eps)
    y64 = (x64 - m64) * r64 * gamma + beta + res
    fwd = one_then_all(("x", "y", "gamma", "beta", "res"), (1,))
    fwd = [{**o, "y_bf16": 0} for o in fwd[:-1]] + [{**fwd[0], "y_bf16": k} for k in (1, 2, 3, 4)] + [{**fwd[-1], "y_bf16": 1}, {**fwd[-1], "y_bf16": 4}]
    tally = Tally(f"cruse_ln_fwd H={H}")
    for offs in fwd:
        X, G, Bt, Rs = place(x, offs["x"]), place(gamma, offs["gamma"]), place(beta, offs["beta"]), place(res, offs["res"])
        Y = place(np.zeros((rows, H), np.float32), offs["y"], sentinel=True)
        Yb = place(np.zeros((rows, H), np.uint16), offs["y_bf16"], sentinel=True)
        Mn, Rd = place(np.zeros(rows, np.float32), sentinel=True), place(np.zeros(rows, np.float32), sentinel=True)
        run(hip, "cruse_ln_fwd", X.ptr, G.ptr, Bt.ptr, Rs.ptr, Y.ptr, Yb.ptr, Mn.ptr, Rd.ptr, rows, H, 1, eps, 0, 0, 0)
        assert all(p.pads_ok() for p in (X, G, Bt, Rs, Y, Yb, Mn, Rd)), offs
        tally.judge("y", offs, max_rel(Y.get(), y64), 3e-6)
        tally.judge("bf16 copy", offs, max_rel(bf16_value(Yb.get()), y64), 8e-3)
        tally.judge("mean", offs, max_rel(Mn.get(), m64[:, 0]), 3e-6)
        tally.judge("rstd", offs, max_rel(Rd.get(), r64[:, 0]), 3e-6)
    tally.done()
    mean, rstd = m64[:, 0].astype(np.float32), r64[:, 0].astype(np.float32)          # the saved statistics, as the backward call receives them
    xh = (x64 - mean[:, None].astype(np.float64)) * rstd[:, None].astype(np.float64)
    gd = dy.astype(np.float64) * gamma
    dx64 = rstd[:, None].astype(np.float64) * (gd - gd.mean(1, keepdims=True) - xh * (gd * xh).mean(1, keepdims=True))
    dg0, db0 = rnd(g, H), rnd(g, H)                                             # "+=": the gradient buffers already hold something
    dg64, db64 = dg0 + (dy * xh).sum(0), db0 + dy.astype(np.float64).sum(0)
    tally = Tally(f"cruse_ln_bwd H={H}")
    for offs in one_then_all(("dy", "x", "dx", "gamma"), (1,)):
        Dy, X, G = place(dy, offs["dy"]), place(x, offs["x"]), place(gamma, offs["gamma"])
        Dx = place(np.zeros((rows, H), np.float32), offs["dx"], sentinel=True)
        Mn, Rd, Dg, Db = place(mean), place(rstd), place(dg0), place(db0)
        run(hip, "cruse_ln_bwd", Dy.ptr, X.ptr, Mn.ptr, Rd.ptr, G.ptr, rows, H, 1, Dx.ptr, Dg.ptr, Db.ptr)
        assert all(p.pads_ok() for p in (Dy, X, G, Dx, Mn, Rd, Dg, Db)), offs
        tally.judge("dx", offs, max_rel(Dx.get(), dx64), 2e-5)
        tally.judge("dgamma", offs, max_rel(Dg.get(), dg64), 2e-5)
        tally.judge("dbeta", offs, max_rel(Db.get(), db64), 2e-5)
    tally.done()


# ---- bf16 GEMM epilogue: float4 / 8-byte stores or element stores, chosen in the kernel from C, ldc and the column quad (gemm_bf16.hip) -----
@pytest.mark.parametrize("M,N,K", [(65, 33, 128), (130, 100, 64)])
def test_gemm_bf16_result_offsets(hip, M, N, K):
    g = np.random.default_rng(M + N + K)
    A, B = bf16_bits(rnd(g, M, K)), bf16_bits(rnd(g, N, K, scale=K ** -0.5))
    bias = rnd(g, N)
    prod = bf16_value(A) @ bf16_value(B).T
    Ad, Bd, bs = place(A), place(B), place(bias)                # the operands stay aligned: a misaligned one is refused (test_gpu_misaligned_refusals.py)
    ld4 = up4(N) + 4
    tally = Tally(f"cruse_gemm_bf16_nt {M}x{N}x{K}")
    for offs, ldc in [(dict(C=0), ld4), (dict(C=1), ld4), (dict(C=2), ld4), (dict(C=3), ld4), (dict(C=0, ldc=1), ld4 + 1), (dict(C=1, ldc=1), ld4 + 1)]:
        C0 = rnd(g, M, ldc)
        for form, use_bias, acc in (("plain", 0, 0), ("bias", 1, 0), ("accumulate", 0, 1)):
            want = prod + (bias if use_bias else 0.0) + (C0[:, :N] if acc else 0.0)
            C = place(C0, offs["C"])
            run(hip, "cruse_gemm_bf16_nt", M, N, K, Ad.ptr, K, 64, Bd.ptr, K, 64, C.ptr, ldc, bs.ptr if use_bias else None, acc, 1)
            got = C.get()
            assert C.pads_ok() and np.array_equal(got[:, N:], C0[:, N:]), (offs, form)
            tally.judge(form, offs, rel_l2(got[:, :N], want), 1e-6)
    tally.done()
    want = prod + bias
    for dt, p, value in ((DT_BF16, 8, bf16_value), (DT_F16, 11, lambda b: b.view(np.float16).astype(np.float64))):
        tally = Tally(f"cruse_gemm_nt_out16 {M}x{N}x{K} dtype {dt}")
        for offs, ldc in [(dict(C=k), ld4) for k in (0, 1, 2, 3, 4, 5)] + [(dict(C=0, ldc=1), ld4 + 1), (dict(C=3, ldc=1), ld4 + 1)]:
            C0 = np.full((M, ldc), 0x4BCD, np.uint16)
            C = place(C0, offs["C"])
            run(hip, "cruse_gemm_nt_out16", M, N, K, Ad.ptr, None, K, 64, Bd.ptr, None, K, 64, C.ptr, ldc, bs.ptr, 0, dt)
            got = C.get()
            assert C.pads_ok() and np.array_equal(got[:, N:], C0[:, N:]), (offs, dt)
            over = np.abs(value(got[:, :N]) - want) - 2.0 ** -p * np.abs(want)       # what one rounding at the store does not explain
            tally.judge("rows", offs, float(max(over.max(), 0.0)) / np.abs(want).max(), 1e-6)
        tally.done()
    assert Ad.pads_ok() and Bd.pads_ok() and bs.pads_ok()


# ---- cruse_transpose_bf16: float4 loads along the columns or 4-byte ones (gemm_bf16.hip, transpose_bf16_kernel) ------------------------------
@pytest.mark.parametrize("rows", (70, 130))
def test_transpose_bf16_input_offsets(hip, rows):
    cols, ldT = 72, (rows + 63) // 64 * 64                  # cols % 4 == 0 (the vector form when aligned), two column blocks
    g = np.random.default_rng(rows)
    tally = Tally(f"cruse_transpose_bf16 rows={rows} (exact)")
    for ld in (cols, cols + 4):
        x = rnd(g, rows, ld)
        for shift in (0, 1, 10):                            # 1: every frame is the first of its clip, the image is all zeros
            src = np.zeros((ldT, cols), np.float32)
            if shift == 0:
                src[:rows] = x[:, :cols]
            else:
                keep = np.arange(rows) % shift != 0
                src[:rows][keep] = x[np.arange(rows)[keep] - 1, :cols]
            want = bf16_bits(src).reshape(ldT // 64, 64, cols).transpose(0, 2, 1)       # [k-tile][column][frame % 64]
            for k in (0, 1, 2, 3):
                X = place(x, k)
                Y = place(np.zeros((ldT // 64, cols, 64), np.uint16), sentinel=True)
                run(hip, "cruse_transpose_bf16", X.ptr, rows, cols, ld, Y.ptr, ldT, shift)
                assert X.pads_ok() and Y.pads_ok()
                tally.judge(f"ld {ld} shift_T {shift}", dict(x=k), float((Y.get() != want).sum()), 0.0)
    tally.done()


# ---- band pooling / expansion: 16-byte accesses on the [rows][F] side when its base allows (grouped_linear.hip) ------------------------------
@pytest.mark.parametrize("mean", (0, 1))
def test_band_pool_and_expand_offsets(hip, mean):
    rows, F = 5, 33                                           # two blocks of 4 rows; 5 * 33 floats leave a tail behind the float4 part
    starts = np.array([0, 1, 3, 8, 8, 20, 30], np.int32)      # an empty band, bins 30..32 in no band
    nb = len(starts) - 1
    g = np.random.default_rng(7 + mean)
    x, m = rnd(g, rows, F), rnd(g, rows, nb)
    width = np.diff(starts)
    wgt = np.where(width > 0, 1.0 / np.maximum(width, 1), 0.0) if mean else np.ones(nb)
    pool64 = np.stack([x[:, a:b].astype(np.float64).sum(1) for a, b in zip(starts[:-1], starts[1:])], 1) * wgt
    exp64 = np.zeros((rows, F))
    for b in range(nb):
        exp64[:, starts[b]:starts[b + 1]] = (m[:, b].astype(np.float64) * wgt[b])[:, None]
    S = place(starts)
    tally = Tally(f"cruse_band_pool mean={mean}")
    for offs in one_then_all(("x", "y"), (1, 2, 3)):
        X, Y = place(x, offs["x"]), place(np.zeros((rows, nb), np.float32), offs["y"], sentinel=True)
        run(hip, "cruse_band_pool", X.ptr, S.ptr, rows, F, nb, mean, Y.ptr)
        assert X.pads_ok() and Y.pads_ok() and S.pads_ok()
        tally.judge("y", offs, rel_l2(Y.get(), pool64), 1e-6)
    tally.done()
    tally = Tally(f"cruse_band_expand mean={mean}")
    for offs in one_then_all(("m", "y"), (1, 2, 3)):
        Mm, Y = place(m, offs["m"]), place(np.zeros((rows, F), np.float32), offs["y"], sentinel=True)
        run(hip, "cruse_band_expand", Mm.ptr, S.ptr, rows, F, nb, mean, Y.ptr)
        assert Mm.pads_ok() and Y.pads_ok() and S.pads_ok()
        tally.judge("y", offs, rel_l2(Y.get(), exp64), 1e-6)
    tally.done()


# ---- nearest upsampling along W and its gradient: float2 / float4 accesses at up = 2 on aligned tensors (generic.hip) ------------------------
def test_upsample_and_downsum_offsets(hip):
    rows, W, up = 5, 6, 2                                     # rows * W even: the vector kernels when both tensors are aligned
    g = np.random.default_rng(3)
    x, gu = rnd(g, rows, W), rnd(g, rows, W * up)
    up64 = np.repeat(x.astype(np.float64), up, axis=1)
    down64 = gu.astype(np.float64).reshape(rows, W, up).sum(2)
    tally = Tally("cruse_upsample_w (exact)")
    for offs in one_then_all(("x", "xu"), (1, 2, 3)):
        X, Y = place(x, offs["x"]), place(np.zeros((rows, W * up), np.float32), offs["xu"], sentinel=True)
        run(hip, "cruse_upsample_w", X.ptr, rows, W, up, Y.ptr, 0)
        assert X.pads_ok() and Y.pads_ok()
        tally.judge("xu", offs, max_rel(Y.get(), up64), 0.0)
    tally.done()
    tally = Tally("cruse_downsum_w (exact)")
    for offs in one_then_all(("dxu", "dx"), (1, 2, 3)):
        X, Y = place(gu, offs["dxu"]), place(np.zeros((rows, W), np.float32), offs["dx"], sentinel=True)
        run(hip, "cruse_downsum_w", X.ptr, rows, W, up, Y.ptr, 0)
        assert X.pads_ok() and Y.pads_ok()
        tally.judge("dx", offs, max_rel(Y.get(), down64.astype(np.float32)), 0.0)       # one f32 add: the float64 sum rounded once
    tally.done()
