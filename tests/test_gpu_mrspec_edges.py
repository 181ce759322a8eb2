"""GPU: cruse_mrspec_loss one resolution at a time, at the lengths where its index arithmetic changes path, against the
float64 restatement tests/mrspec_ref.py.  Companion of test_gpu_mrspec.py, whose shapes mix the resolutions and stay inside one run at N = 2048.

A workgroup owns a run of K hops (C = K * N / 4 samples) of the padded axis (L + N samples), recomputes the three frames before its run, counts a
frame's loss only in the run that owns it; mrspec_fold_kernel reflects both padded ends back.  Lengths per N (runs = ceil((L + N) / C)):
    N/2 + 1 (both reflections inside one frame), N/2 + 2, N - 1 (the two fold-back ranges overlap), N, C - N (the padded axis ends exactly on a
    run), C - N + 1 (one sample into a second run), 2C - N + H (a third run that holds one hop), 2C + 37 (three runs, L odd)
The run counts are asserted from cruse_mrspec_ws_bytes, so a change of mr_hops cannot turn these into other cases unnoticed.

Inputs: mrspec_ref.make_pair(B, L, seed); factor = f_complex = 1000 unless the test says otherwise.
Bars: loss 1e-5 relative, gradient 2e-5 rel-L2 (the bars of test_gpu_mrspec.py at gamma = 1), here also at gamma = 2 and 1.5: these run the whole
gamma != 1 branch (powf, the clamp, gphi, gr) and are well conditioned, |Y|^(gamma - 2) being bounded at the bins near zero.  On the CPU, over
the 40 shapes and seeds 0..7, the f32 restatement stays within 6.1e-7 (gamma = 2), 3.1e-7 (1.5), 1.7e-6 (1) rel-L2 of float64 in the gradient and
3.1e-7 in the loss: the bars leave the reference more than 10x of room, and every case first asserts that the f32 restatement is inside them.
Gradient segments (the first and the last N/2 samples, the 2H samples centred on every run boundary r * C - N/2 inside the clip): rel-L2 on the
segment within 4 * max(e32_segment, 5e-6), e32_segment = the f32 restatement against float64 on that segment, max over seeds 0..3.

A clip alone and in a batch: the loss is a mean over the batch, so the kernel's weights are factor / (B * bins * frames).  The B = 3 call is made
with factor = f_complex = 3000 and the three B = 1 calls with 1000: 3000 / (3 c) and 1000 / c are the same real number and the division is
correctly rounded, so every workgroup gets the same f32 weights in both, which is what lets the rows be compared bit for bit.  (With equal
weights the rows differ by the rounding of 1 / cnt, and no bit comparison is possible.)

Measured on an MI355X (seed 0; worst over all cases of a kind, error / bar):
    sweep, 120 cases      loss 2.3e-7 (N 2048, L 1026, gamma 2), gradient 3.7e-7 (N 512, L 2944, gamma 2): 0.023 of the bar;
                          per exponent 0.018 (gamma 1), 0.023 (2), 0.018 (1.5)
    segments, 200         5.1e-7 on the last N/2 of N 512, L 2944, gamma 2: 0.025 of its bar; gamma 1: 4.5e-7 (N 2048, L 2048, last N/2), 0.022.
                          e32_segment never exceeded 2.6e-6, so every segment's bar was the floor 4 * 5e-6 = 2e-5
    single terms, 20      gradient 3.5e-7, loss 2.0e-7 (N 2048, L 2049, gamma 2): 0.020
    distinct weights      loss 8.4e-8 / 1.7e-7, gradient 2.0e-7 / 2.6e-7 (gamma 1 / 2); against the sum of three calls: gradient 3.5e-8, loss 0
    R = 8                 loss 7.3e-8, gradient 1.4e-7
    alone / in a batch    rows bit-identical; loss within 1.2e-16
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mrspec_ref as R
from util import bits, embed, poison_, same_bits

pytestmark = pytest.mark.gpu

W = 1000.0                                                    # factor = f_complex unless stated
NS = (128, 256, 512, 1024, 2048)
HOPS = {128: 29, 256: 13, 512: 13, 1024: 9, 2048: 8}          # mr_hops of mrspec.hip; checked against the library in runs_of()
LOSS_BAR, GRAD_BAR = 1e-5, 2e-5
B = 2


def lengths(N):
    """label -> (L, runs the issue expects)"""
    H, C = N // 4, HOPS[N] * N // 4
    return {"N/2+1": (N // 2 + 1, 1), "N/2+2": (N // 2 + 2, 1), "N-1": (N - 1, 1), "N": (N, 1), "C-N": (C - N, 1), "C-N+1": (C - N + 1, 2),
            "2C-N+H": (2 * C - N + H, 3), "2C+37": (2 * C + 37, 3)}


LABELS = list(lengths(128))
CASES = [pytest.param(N, lab, id=f"{N}-{lab}") for N in NS for lab in LABELS]


def runs_of(N, L):
    """the run count the LIBRARY lays out for (N, L): with B = 32 the partial sums take 256 * runs bytes, already a multiple of 256"""
    from cruse_amd import ops
    need = ops.mrspec_ws_bytes(32, L, (N,))
    assert need > 0
    grads = (32 * (L + N) * 4 + 255) // 256 * 256
    assert (need - grads) % 256 == 0
    return (need - grads) // 256


@functools.lru_cache(maxsize=None)
def pair(b, L, seed):
    return R.make_pair(b, L, seed)


def weights(mode):
    """mode -> (factor, f_complex): both terms, the magnitude term alone, the complex term alone"""
    return {"both": (W, W), "mag": (W, None), "cplx": (0.0, W)}[mode]


@functools.lru_cache(maxsize=None)
def reference(N, L, gamma, seed=0, dtype=torch.float64, mode="both"):
    """(loss, grad) of the restatement on the CPU in `dtype` for B clips of L samples at resolution N; computed once, shared, never modified"""
    est, ref = pair(B, L, seed)
    factor, fc = weights(mode)
    return R.mrspec_loss_and_grad(est, ref, (N,), gamma, factor, fc, dtype=dtype)


@functools.lru_cache(maxsize=None)
def kernel(N, L, gamma, mode="both"):
    """(loss, grad) of the kernel on seed 0, on the CPU; computed once, shared, never modified"""
    from cruse_amd import ops
    est, ref = pair(B, L, 0)
    factor, fc = weights(mode)
    loss, dx = ops.mrspec_loss(est.cuda(), ref.cuda(), (N,), gamma, factor, fc)
    return loss.cpu(), dx.cpu()


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def check_against_float64(what, N, L, gamma, mode="both"):
    loss64, grad64 = reference(N, L, gamma, mode=mode)
    loss32, grad32 = reference(N, L, gamma, dtype=torch.float32, mode=mode)
    l32, g32 = rel(loss32, loss64), R.rel_l2(grad32, grad64)
    assert l32 <= LOSS_BAR and g32 <= GRAD_BAR, f"the f32 restatement itself is outside the bar: loss {l32:.2e}, gradient {g32:.2e}"
    loss, dx = kernel(N, L, gamma, mode)
    assert bool(torch.isfinite(dx).all())
    le, ge = rel(loss, loss64), R.rel_l2(dx, grad64)
    print(f"[mrspec-edges {what}] N {N} L {L} gamma {gamma} {mode}: loss rel {le:.2e} (f32 restatement {l32:.2e}, bar {LOSS_BAR:.0e}), "
          f"grad rel-L2 {ge:.2e} (f32 restatement {g32:.2e}, bar {GRAD_BAR:.0e}), ratio {max(le / LOSS_BAR, ge / GRAD_BAR):.3f}")
    assert le <= LOSS_BAR
    assert ge <= GRAD_BAR


# ---------------------------------------------------------------- 1. every resolution alone, every length, three exponents
@pytest.mark.parametrize("N,lab", CASES)
def test_run_counts_are_the_cases_meant(N, lab):
    L, runs = lengths(N)[lab]
    assert -(-(L + N) // (HOPS[N] * N // 4)) == runs
    assert runs_of(N, L) == runs, "mr_hops changed: the lengths of this file no longer sit on the run edges"
    assert L > N // 2


@pytest.mark.parametrize("gamma", [1.0, 2.0, 1.5])
@pytest.mark.parametrize("N,lab", CASES)
def test_sweep_vs_float64(N, lab, gamma):
    check_against_float64("sweep", N, lengths(N)[lab][0], gamma)


# ---------------------------------------------------------------- 2. gradient error on the edge segments
def segments(N, L, runs):
    H, C, M = N // 4, HOPS[N] * N // 4, N // 2
    segs = [("first N/2", 0, M), ("last N/2", L - M, L)]
    for r in range(1, runs):
        c = r * C - M                                         # the unpadded index of the first sample of run r
        if 0 <= c < L:
            segs.append((f"run boundary {r}", max(0, c - H), min(L, c + H)))
    return segs


def seg_rel(a, b, lo, hi):
    a, b = a[:, lo:hi].double(), b[:, lo:hi].double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("gamma", [1.0, 2.0])
@pytest.mark.parametrize("N,lab", CASES)
def test_localised_gradient_error(N, lab, gamma):
    L, runs = lengths(N)[lab]
    _, dx = kernel(N, L, gamma)
    _, grad64 = reference(N, L, gamma)
    segs = segments(N, L, runs)
    assert len(segs) == 2 + {"2C-N+H": 1, "2C+37": 2}.get(lab, 0)
    bad = []
    for name, lo, hi in segs:
        assert 0 <= lo < hi <= L
        e32 = max(seg_rel(reference(N, L, gamma, s, torch.float32)[1], reference(N, L, gamma, s)[1], lo, hi) for s in range(4))
        bar = 4 * max(e32, 5e-6)
        err = seg_rel(dx, grad64, lo, hi)
        print(f"[mrspec-edges segment] N {N} L {L} gamma {gamma} {name} [{lo}, {hi}): rel-L2 {err:.2e}, e32 {e32:.2e}, bar {bar:.2e}, "
              f"ratio {err / bar:.3f}")
        if not err <= bar:
            bad.append((name, err, bar))
    assert not bad, bad


# ---------------------------------------------------------------- 3. one term at a time
@pytest.mark.parametrize("mode", ["mag", "cplx"])
@pytest.mark.parametrize("gamma", [1.0, 2.0])
@pytest.mark.parametrize("N", NS)
def test_single_terms(N, gamma, mode):
    check_against_float64("single term", N, lengths(N)["C-N+1"][0], gamma, mode)


# ---------------------------------------------------------------- 4. weights per resolution, call order, R limits
MIX_N, MIX_W, MIX_L = (2048, 128, 512), [1000.0, 10.0, 300.0], 4200


@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_distinct_weights_per_resolution(gamma):
    from cruse_amd import ops
    est, ref = pair(B, MIX_L, 0)
    x, s = est.cuda(), ref.cuda()
    loss64, grad64 = R.mrspec_loss_and_grad(est, ref, MIX_N, gamma, W, MIX_W)
    if gamma == 1.0:                                          # the weights matter: a mixed-up index is not inside any bar
        same64, _ = R.mrspec_loss_and_grad(est, ref, MIX_N, gamma, W, [W] * 3)
        assert abs(float(loss64) - 2.1250) < 5e-4 and abs(float(same64) - 2.9387) < 5e-4
    loss, dx = ops.mrspec_loss(x, s, MIX_N, gamma, W, MIX_W)
    le, ge = rel(loss.cpu(), loss64), R.rel_l2(dx.cpu(), grad64)
    print(f"[mrspec-edges weights] gamma {gamma}: loss {float(loss):.9g} vs {float(loss64):.9g}, rel {le:.2e} (bar {LOSS_BAR:.0e}), "
          f"grad rel-L2 {ge:.2e} (bar {GRAD_BAR:.0e})")
    assert le <= LOSS_BAR and ge <= GRAD_BAR
    # the three resolutions one call each, with their own complex weights: a resolution's terms do not depend on its place in the list
    parts = [ops.mrspec_loss(x, s, (n,), gamma, W, w) for n, w in zip(MIX_N, MIX_W)]
    total = sum(p[1].double() for p in parts)
    se = R.rel_l2(dx.cpu(), total.cpu())
    sl = rel(loss.cpu(), sum(float(p[0]) for p in parts))
    print(f"[mrspec-edges weights] gamma {gamma}: against the sum of three calls: grad rel-L2 {se:.2e} (bar {GRAD_BAR:.0e}), loss rel {sl:.2e}")
    assert se <= GRAD_BAR and sl <= LOSS_BAR
    loss2, dx2 = ops.mrspec_loss(x, s, MIX_N, gamma, W, MIX_W)
    assert same_bits(loss, loss2) and same_bits(dx, dx2)


def test_eight_resolutions_with_repeats():
    from cruse_amd import ops
    n_ffts = (128, 256, 512, 1024, 2048, 128, 256, 512)
    est, ref = pair(B, MIX_L, 0)
    loss64, grad64 = R.mrspec_loss_and_grad(est, ref, n_ffts, 1.0, W, W)
    loss, dx = ops.mrspec_loss(est.cuda(), ref.cuda(), n_ffts, 1.0, W, W)
    le, ge = rel(loss.cpu(), loss64), R.rel_l2(dx.cpu(), grad64)
    print(f"[mrspec-edges R=8] loss rel {le:.2e} (bar {LOSS_BAR:.0e}), grad rel-L2 {ge:.2e} (bar {GRAD_BAR:.0e})")
    assert le <= LOSS_BAR and ge <= GRAD_BAR


def raw(est, ref, n_ffts, gamma, factor, fc, ws, ws_bytes, loss, dest, grad_scale=1.0):
    from cruse_amd import ops
    from cruse_amd._lib import lib
    R_ = len(n_ffts)
    n_arr = (ctypes.c_int * R_)(*n_ffts)
    fc_arr = (ctypes.c_float * R_)(*fc) if fc is not None else None
    b, L = est.shape
    return lib.cruse_mrspec_loss(ops._p(est), ops._p(ref), b, L, ctypes.cast(n_arr, ctypes.c_void_p), R_, gamma, factor,
                                 ctypes.cast(fc_arr, ctypes.c_void_p) if fc_arr is not None else None, ops._p(ws), ws_bytes, ops._p(loss),
                                 ops._p(dest), grad_scale, ops._stream())


@pytest.mark.parametrize("n_ffts", [(128,) * 9, ()], ids=["R=9", "R=0"])
def test_resolution_count_outside_1_to_8_is_refused(n_ffts):
    from cruse_amd import ops
    from cruse_amd._lib import lib
    est, ref = pair(B, 700, 0)
    x, s = est.cuda(), ref.cuda()
    assert ops.mrspec_ws_bytes(B, 700, n_ffts) == 0
    need = ops.mrspec_ws_bytes(B, 700, (128,) * 8)
    ws = poison_(torch.empty(need // 4, device="cuda", dtype=torch.float32))
    loss = poison_(torch.empty(1, device="cuda", dtype=torch.float64))
    dest = poison_(torch.empty(B, 700, device="cuda", dtype=torch.float32))
    pat32, pat64 = bits(poison_(torch.empty(1, device="cuda"))), bits(poison_(torch.empty(1, device="cuda", dtype=torch.float64)))
    assert raw(x, s, n_ffts, 1.0, W, [W] * len(n_ffts), ws, need, loss, dest) == -1
    assert "R=" in lib.cruse_last_error().decode()
    torch.cuda.synchronize()
    assert bool((bits(loss) == pat64).all()) and bool((bits(dest) == pat32).all()) and bool((bits(ws) == pat32).all())


# ---------------------------------------------------------------- 5. evaluation mode
@pytest.mark.parametrize("N,lab", CASES)
def test_evaluation_mode_gives_the_gradient_calls_loss_bits(N, lab):
    from cruse_amd import ops
    L = lengths(N)[lab][0]
    est, ref = pair(B, L, 0)
    loss, _ = kernel(N, L, 1.0)
    le, none = ops.mrspec_loss(est.cuda(), ref.cuda(), (N,), 1.0, W, W, want_grad=False)
    assert none is None and same_bits(le.cpu(), loss), (float(le), float(loss))


# ---------------------------------------------------------------- 6. a clip alone and in a batch
@pytest.mark.parametrize("gamma", [1.0, 2.0])
@pytest.mark.parametrize("N,L", [(2048, 2049), (128, 1893)])
def test_a_clip_alone_and_in_a_batch(N, L, gamma):
    from cruse_amd import ops
    assert runs_of(N, L) == (2 if N == 2048 else 3)
    est, ref = pair(3, L, 0)
    assert not torch.equal(est[0], est[1]) and not torch.equal(est[1], est[2])
    x, s = est.cuda(), ref.cuda()
    # weights 3000 in the batch, 1000 alone: the same f32 factor / cnt in every workgroup (module docstring)
    l3, d3 = ops.mrspec_loss(x, s, (N,), gamma, 3 * W, 3 * W)
    alone = [ops.mrspec_loss(x[i:i + 1].contiguous(), s[i:i + 1].contiguous(), (N,), gamma, W, W) for i in range(3)]
    for i, (_, di) in enumerate(alone):
        assert same_bits(d3[i:i + 1], di), f"clip {i}: {int((bits(d3[i:i + 1]) != bits(di)).sum())} of {L} gradient samples differ"
    # ... and so the batch's mean with weights 1000 is the f64 sum of the three means, each times 1/3
    total = sum(float(li) / 3.0 for li, _ in alone)
    err = abs(float(l3) / 3.0 - total) / total
    print(f"[mrspec-edges batch] N {N} L {L} gamma {gamma}: loss {float(l3) / 3.0:.17g} vs {total:.17g}, rel {err:.2e} (bar 1e-12)")
    assert err <= 1e-12


# ---------------------------------------------------------------- 7. what lies around est and ref
@pytest.mark.parametrize("lab", ["N/2+1", "C-N+1"])
@pytest.mark.parametrize("N", NS)
def test_nothing_is_read_outside_the_inputs(N, lab):
    from cruse_amd import ops
    L = lengths(N)[lab][0]
    est, ref = pair(1, L, 0)
    xe, check_e = embed(est, lead=4096, trail=4096)
    xr, check_r = embed(ref, lead=4096, trail=4096)
    assert xe.shape == (1, L) and xe.is_contiguous() and xe.data_ptr() % 4 == 0
    loss, dx = ops.mrspec_loss(xe, xr, (N,), 1.0, W, W)
    plain_loss, plain_dx = ops.mrspec_loss(est.cuda(), ref.cuda(), (N,), 1.0, W, W)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and bool(torch.isfinite(dx).all()), "a NaN from outside est / ref reached the result"
    assert same_bits(loss, plain_loss) and same_bits(dx, plain_dx)
    check_e("est")
    check_r("ref")


# ---------------------------------------------------------------- 8. grad_scale
def test_grad_scale():
    from cruse_amd import ops
    N = 256
    L = lengths(N)["C-N+1"][0]
    assert runs_of(N, L) == 2
    est, ref = pair(B, L, 0)
    x, s = est.cuda(), ref.cuda()
    l1, d1 = ops.mrspec_loss(x, s, (N,), 1.0, W, W)
    ls, ds = ops.mrspec_loss(x, s, (N,), 1.0, W, W, grad_scale=0.3)
    assert same_bits(ls, l1) and same_bits(ds, d1 * 0.3)
    l0, d0 = ops.mrspec_loss(x, s, (N,), 1.0, W, W, grad_scale=0.0)
    assert same_bits(l0, l1) and np.isfinite(float(l0)) and float(l0) > 0
    assert bool((d0 == 0).all())
