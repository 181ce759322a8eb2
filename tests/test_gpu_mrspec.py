"""GPU: cruse_mrspec_loss against the float64 restatement tests/mrspec_ref.py.

Inputs: ref = 0.1 randn, est = ref + 0.05 randn, drawn in f64 and cast to f32; factor = f_complex = 1000 unless the shape says otherwise.
Bars: loss 1e-5 relative (f32 FFT rounding ~ eps log2 N = 7e-7 at N = 2048, the mean of squares is accumulated in f64); gradient at
gamma = 1 2e-5 rel-L2 (no singular term; room for a forward plus an inverse 2048-point FFT); gradient at gamma != 1: |Y|^(gamma - 2) makes it
ill-conditioned at the few bins that happen to lie near zero for ANY f32 implementation, so the bar is measured on the restatement at test
time: e32 = max over seeds 0..7 of rel-L2(restatement in f32, restatement in f64), the kernel within 4 * max(e32, 5e-6) for seeds 0..3."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mrspec_ref as R
from util import bits, has_poison, poison_, same_bits

pytestmark = pytest.mark.gpu

# id -> (B, L, n_ffts, gamma, f_complex)
SHAPES = {
    "a": (2, 700, (128, 256), 0.3, 1000.0),                    # the fixture; L not a multiple of any hop
    "b": (3, 2049, (128, 256, 512, 1024), 0.3, 1000.0),        # several runs per clip, four resolutions summed, B odd
    "c": (2, 1300, (256,), 1.0, 1000.0),                       # the unclamped branch
    "d": (1, 1025, (2048,), 0.6, 1000.0),                      # L = N / 2 + 1: both reflections meet inside one frame
    "e": (2, 1024, (128,), 0.3, None),                         # L a multiple of the hop; magnitude term only
    "f": (2, 1300, (256,), 0.3, [1000.0]),                     # per-resolution complex weights (the list form)
}
FACTOR = 1000.0


@functools.lru_cache(maxsize=None)
def reference(sid, seed, gamma=None, dtype=torch.float64):
    """(est f32, ref f32, loss, grad) of shape `sid` on the CPU in `dtype`; computed once, shared, never modified"""
    B, L, n_ffts, g, fc = SHAPES[sid]
    est, ref = R.make_pair(B, L, seed)
    loss, grad = R.mrspec_loss_and_grad(est, ref, n_ffts, g if gamma is None else gamma, FACTOR, fc, dtype=dtype)
    return est, ref, loss, grad


def run(sid, est, ref, gamma=None, want_grad=True):
    from cruse_amd import ops
    B, L, n_ffts, g, fc = SHAPES[sid]
    loss, dx = ops.mrspec_loss(est.cuda(), ref.cuda(), n_ffts, g if gamma is None else gamma, FACTOR, fc, want_grad=want_grad)
    return loss.cpu(), None if dx is None else dx.cpu()


@pytest.mark.parametrize("sid", list(SHAPES))
def test_loss_value_vs_float64(sid):
    est, ref, loss64, _ = reference(sid, 0)
    loss, _ = run(sid, est, ref)
    err = abs(float(loss) - float(loss64)) / abs(float(loss64))
    print(f"[mrspec loss] shape {sid}: {float(loss):.9g} vs {float(loss64):.9g}, rel {err:.2e}")
    assert err <= 1e-5


def test_fixture_of_the_reference_code(golden):
    g = golden("mrspec.npz")
    est, ref = torch.from_numpy(g["est"]), torch.from_numpy(g["ref"])
    loss, dx = run("a", est, ref)
    assert abs(float(loss) - float(g["loss"])) <= 1e-5 * float(g["loss"])
    e32 = max(R.rel_l2(reference("a", s, dtype=torch.float32)[3], reference("a", s)[3]) for s in range(8))
    err = R.rel_l2(dx, torch.from_numpy(g["grad"]))
    print(f"[mrspec fixture] grad rel-L2 {err:.2e}, e32 {e32:.2e}")
    assert err <= 4 * max(e32, 5e-6)


@pytest.mark.parametrize("sid", list(SHAPES))
def test_structure_gradient_at_gamma_one(sid):
    est, ref, loss64, grad64 = reference(sid, 0, gamma=1.0)
    loss, dx = run(sid, est, ref, gamma=1.0)
    err = R.rel_l2(dx, grad64)
    print(f"[mrspec gamma=1] shape {sid}: grad rel-L2 {err:.2e}, loss rel {abs(float(loss) - float(loss64)) / float(loss64):.2e}")
    assert abs(float(loss) - float(loss64)) <= 1e-5 * float(loss64)
    assert err <= 2e-5


@pytest.mark.parametrize("sid", [s for s in SHAPES if SHAPES[s][3] != 1.0])
def test_compressed_gradient_within_the_f32_restatements_error(sid):
    e32 = max(R.rel_l2(reference(sid, s, dtype=torch.float32)[3], reference(sid, s)[3]) for s in range(8))
    bar = 4 * max(e32, 5e-6)
    errs = []
    for seed in range(4):
        est, ref, _, grad64 = reference(sid, seed)
        _, dx = run(sid, est, ref)
        assert bool(torch.isfinite(dx).all())
        errs.append(R.rel_l2(dx, grad64))
    print(f"[mrspec gamma!=1] shape {sid}: kernel rel-L2 {['%.2e' % e for e in errs]}, e32 {e32:.2e}, bar {bar:.2e}")
    assert max(errs) <= bar


def test_exact_cases():
    est, ref, _, _ = reference("a", 0)
    zero = torch.zeros_like(ref)
    for x, s, what in ((ref, ref, "est == ref"), (zero, zero, "all zero")):
        loss, dx = run("a", x, s)
        assert float(loss) == 0.0 and bool((dx == 0).all()), what
    loss, dx = run("a", zero, ref)
    assert np.isfinite(float(loss)) and float(loss) > 0 and bool(torch.isfinite(dx).all())
    loss, dx = run("a", zero, ref, gamma=1.0)
    assert np.isfinite(float(loss)) and float(loss) > 0 and bool(torch.isfinite(dx).all())


def raw(est, ref, n_ffts, gamma, fc, ws, ws_bytes, loss, dest, grad_scale=1.0):
    from cruse_amd import ops
    from cruse_amd._lib import lib
    R_ = len(n_ffts)
    n_arr = (ctypes.c_int * R_)(*n_ffts)
    fc_arr = (ctypes.c_float * R_)(*fc) if fc else None
    B, L = est.shape
    return lib.cruse_mrspec_loss(ops._p(est), ops._p(ref), B, L, ctypes.cast(n_arr, ctypes.c_void_p), R_, gamma, FACTOR,
                                 ctypes.cast(fc_arr, ctypes.c_void_p) if fc_arr else None, ops._p(ws), ws_bytes, ops._p(loss), ops._p(dest),
                                 grad_scale, ops._stream())


def test_determinism_scaling_and_evaluation_mode():
    from cruse_amd import ops
    est, ref, _, _ = reference("b", 0)
    B, L, n_ffts, g, fc = SHAPES["b"]
    l1, d1 = ops.mrspec_loss(est.cuda(), ref.cuda(), n_ffts, g, FACTOR, fc)
    l2, d2 = ops.mrspec_loss(est.cuda(), ref.cuda(), n_ffts, g, FACTOR, fc)
    assert same_bits(l1, l2) and same_bits(d1, d2)
    _, dh = ops.mrspec_loss(est.cuda(), ref.cuda(), n_ffts, g, FACTOR, fc, grad_scale=0.5)
    assert same_bits(dh, d1 * 0.5)
    # evaluation: same loss bits, no gradient buffer touched (the whole workspace behind the partial sums stays poisoned)
    need = ops.mrspec_ws_bytes(B, L, n_ffts)
    ws = poison_(torch.empty(need // 4, device="cuda", dtype=torch.float32))
    loss = poison_(torch.empty(1, device="cuda", dtype=torch.float64))
    x, s = est.cuda(), ref.cuda()
    assert raw(x, s, n_ffts, g, [fc] * len(n_ffts), ws, need, loss, None) == 0
    torch.cuda.synchronize()
    assert same_bits(loss, l1)
    nparts = sum(B * -(-(L + n) // ({128: 29, 256: 13, 512: 13, 1024: 9, 2048: 8}[n] * n // 4)) for n in n_ffts)
    grads = ws[(8 * nparts + 255) // 256 * 64:]
    assert bool((bits(grads) == bits(poison_(torch.empty(1, device="cuda")))).all())
    lw, dw = ops.mrspec_loss(x, s, n_ffts, g, FACTOR, fc, want_grad=False)
    assert dw is None and same_bits(lw, l1)


@pytest.mark.parametrize("sid", ["a", "d"])
def test_bounds_poisoned_workspace_and_gradient(sid):
    from cruse_amd import ops
    from cruse_amd._lib import lib
    est, ref, _, _ = reference(sid, 0)
    B, L, n_ffts, g, fc = SHAPES[sid]
    fcl = [fc] * len(n_ffts) if fc else None
    x, s = est.cuda(), ref.cuda()
    need = ops.mrspec_ws_bytes(B, L, n_ffts)
    assert need > 0 and need % 256 == 0
    extra = 4096
    ws = poison_(torch.empty((need + extra) // 4, device="cuda", dtype=torch.float32))
    dest = poison_(torch.empty(B * L + 1024, device="cuda", dtype=torch.float32))
    loss = poison_(torch.empty(4, device="cuda", dtype=torch.float64))
    assert raw(x, s, n_ffts, g, fcl, ws, need, loss, dest) == 0
    torch.cuda.synchronize()
    pat = bits(poison_(torch.empty(1, device="cuda")))
    assert bool((bits(ws[need // 4:]) == pat).all()), "the workspace was written beyond cruse_mrspec_ws_bytes"
    assert bool((bits(dest[B * L:]) == pat).all()), "dest was written beyond B * L"
    assert not has_poison(dest[:B * L]) and not has_poison(loss[:1]) and has_poison(loss[1:])
    l0, d0 = ops.mrspec_loss(x, s, n_ffts, g, FACTOR, fc)
    assert same_bits(loss[:1], l0) and same_bits(dest[:B * L].view(B, L), d0)
    assert raw(x, s, n_ffts, g, fcl, ws, need - 1, loss, dest) == -1
    assert "ws_bytes" in lib.cruse_last_error().decode()


def test_autograd_applies_the_upstream_scalar():
    from cruse_amd import ops
    from cruse_amd.loss import MultiResSpecLoss, multi_res_spec_loss
    est, ref, loss64, _ = reference("a", 0)
    x = est.clone().cuda().requires_grad_(True)
    s = ref.cuda()
    val = multi_res_spec_loss((128, 256), 0.3, FACTOR, 1000.0)(x, s)
    assert val.dtype == torch.float32 and abs(float(val) - float(loss64)) <= 1e-5 * float(loss64)
    (3.0 * val).backward()
    _, dx = ops.mrspec_loss(est.cuda(), s, (128, 256), 0.3, FACTOR, 1000.0)
    assert torch.equal(x.grad, dx * 3.0)
    x2 = est.clone().cuda().requires_grad_(True)
    MultiResSpecLoss([128, 256], 0.3, FACTOR, 1000.0)(x2, s).backward()
    assert torch.equal(x2.grad, dx)
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        multi_res_spec_loss()(torch.zeros(2, 700).cuda(), torch.zeros(2, 701).cuda())
    with pytest.raises(ValueError, match="too short"):
        multi_res_spec_loss()(torch.zeros(2, 256).cuda(), torch.zeros(2, 256).cuda())
