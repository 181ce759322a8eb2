"""cruse_mask_head_fwd_bwd (csrc/mask_head.hip, ops.mask_head, EngineConfig.fuse_mask_head): the last decoder BatchNorm, the mask conv,
WO-MALE and the decoder-1 data gradient in one launch, against the four calls it replaces

    ops.bn_finalize_act_fwd -> ops.conv_scatter2(act=1) -> ops.mask_loss(want_dlogit) -> ops.conv_gather(bn_bwd=...)

on the same inputs.  Eight outputs are compared as BITS: u_1, mask, dlogit, du_1, mean, rstd, running_mean, running_var.  The loss sum and the
two BatchNorm-backward sums are f64 atomics in both forms (free order): they are compared to an f64 torch-CPU restatement of the whole chain, and
the fused error may be at most twice the unfused error of the same case (plus what the f64 reference itself cannot resolve: 2^-52 times the
sum of the magnitudes of its addends, per addend -- the rounding bound of its own summation).

Shapes: the bench geometry (C1, F1) = (8, 80) and a 16-channel variant (16, 40); (B, T) = (1, 1) one frame, (1, 7) fewer frames than a tile of 8,
(2, 9) a tile plus one frame, (3, 33) several tiles with a ragged last one; input batch sums and backward sums in 1 and in BN_STAT_REPLICAS
replicas; the grid capped at 2 workgroups for the largest case, so that a workgroup walks several tiles.

Poison: the six output tensors are NaN-filled before the call and every element must come out written.  The running statistics are updated from
their previous value ((1 - momentum) * old + momentum * new), so NaN cannot stand in them: they start from a sentinel and every element must have
moved to the bits of the unfused call.  Every input lies inside a larger NaN-filled buffer; a read outside it would surface as a NaN in an output
or in a sum.  The accumulators (loss, backward sums) are pre-loaded with non-zero values and handed over as `zeroed`: the kernel must ADD."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
ALPHA, BETA = 2.0, 1.0
PAD = 64                    # floats of NaN on either side of every input (a multiple of 4: the 16-byte alignment of the rows is kept)
SHAPES = [(8, 80), (16, 40)]
BT = [(1, 1), (1, 7), (2, 9), (3, 33)]


def _inside_nan(t: torch.Tensor) -> torch.Tensor:
    """a copy of t in the middle of a larger NaN-filled buffer"""
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device="cuda", dtype=t.dtype)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _case(C, F1, B, T, nrep, seed):
    g = torch.Generator().manual_seed(seed)
    rows, Fn, Fs = B * T, 2 * F1, 2 * F1 + 1
    r = lambda *s: torch.randn(*s, generator=g)
    v = r(B, T, C, F1) * 1.5 + 0.3
    # the batch sums of v in f64, spread over nrep replicas (the statistic is the sum over the replicas)
    v64 = v.double()
    tot = torch.cat([v64.sum(dim=(0, 1, 3)), (v64 * v64).sum(dim=(0, 1, 3))])
    share = torch.rand(nrep, 1, generator=g).double() + 0.1
    sums = (share / share.sum()) * tot[None, :]
    c = dict(C=C, F1=F1, B=B, T=T, rows=rows, Fn=Fn, Fs=Fs, nrep=nrep,
             v=v, skip=r(B, T, C, F1), sums=sums, gamma=1.0 + 0.2 * r(C), beta=0.3 * r(C), w=0.4 * r(C, 1, 1, 3), bias=0.1 * r(1),
             rm=r(C), rv=torch.rand(C, generator=g) + 0.5, nre=r(rows, Fs), nim=r(rows, Fs), cmag=r(rows, Fs).abs())
    c["dev"] = {k: _inside_nan(c[k].cuda()) for k in ("v", "skip", "sums", "gamma", "beta", "w", "bias", "nre", "nim", "cmag")}
    return c


def _reference(c):
    """the chain in f64 on the CPU -> (loss sum, sum g [C], sum g*xhat [C], and the sums of the magnitudes of their addends)"""
    C, F1, B, T, rows, Fn = c["C"], c["F1"], c["B"], c["T"], c["rows"], c["Fn"]
    d = lambda k: c[k].double()
    cnt = rows * F1
    tot = d("sums").sum(0)
    mean = tot[:C] / cnt
    var = (tot[C:] / cnt - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    bc = lambda t: t.view(1, 1, C, 1)
    xh = (d("v") - bc(mean)) * bc(rstd)
    t = xh * bc(d("gamma")) + bc(d("beta"))
    u = t.clamp_min(0.0) + d("skip")
    w = d("w").view(C, 3)
    um1 = torch.nn.functional.pad(u, (1, 0))[..., :F1]
    even = d("bias") + torch.einsum("c,btcf->btf", w[:, 0], u) + torch.einsum("c,btcf->btf", w[:, 2], um1)
    odd = d("bias") + torch.einsum("c,btcf->btf", w[:, 1], u)
    mask = torch.sigmoid(torch.stack([even, odd], dim=-1).reshape(rows, Fn))
    mask_s = torch.nn.functional.pad(mask, (0, 1))                       # bin Fs - 1: mask 0
    re, im, mr = d("nre"), d("nim"), d("cmag")
    mag_est = torch.sqrt((mask_s * re) ** 2 + (mask_s * im) ** 2)
    mag_unp = torch.sqrt(re * re + im * im)
    wgt = torch.exp(ALPHA / (BETA + mr / mag_unp))
    dd = torch.log10(mag_est + 1.0) - torch.log10(mr + 1.0)
    terms = wgt * dd.abs()
    dm = wgt * torch.sign(dd) / np.log(10.0) / (mag_est + 1.0) * mag_unp / (rows * c["Fs"])
    dlogit = (dm[:, :Fn] * mask * (1.0 - mask)).view(B, T, Fn)
    xp = torch.nn.functional.pad(dlogit, (0, 2))
    du = torch.stack([w[ch, 0] * xp[..., 0:Fn:2] + w[ch, 1] * xp[..., 1:Fn + 1:2] + w[ch, 2] * xp[..., 2:Fn + 2:2] for ch in range(C)], dim=2)
    gr = du * (t > 0)
    return (terms.sum(), gr.sum(dim=(0, 1, 3)), (gr * xh).sum(dim=(0, 1, 3)),
            terms.abs().sum(), gr.abs().sum(dim=(0, 1, 3)), (gr * xh).abs().sum(dim=(0, 1, 3)))


def _unfused(c):
    from cruse_amd import ops
    C, F1, B, T, rows, Fn, Fs = c["C"], c["F1"], c["B"], c["T"], c["rows"], c["Fn"], c["Fs"]
    x = c["dev"]
    rm, rv = c["rm"].cuda(), c["rv"].cuda()
    u, mean, rstd = ops.bn_finalize_act_fwd(x["v"], x["sums"], rows * F1, EPS, MOM, x["gamma"], x["beta"], x["skip"], rows, C, F1, relu=True,
                                            running_mean=rm, running_var=rv)
    mask = ops.conv_scatter2(u, x["w"], x["bias"], B, T, C, F1, 1, KT=1, pad=0, act=1, prec="bf16")
    loss, _, dlogit, _, _ = ops.mask_loss(mask, x["nre"], x["nim"], x["cmag"], rows, Fn, Fs, ALPHA, BETA, want_dlogit=True)
    du, bsums = ops.conv_gather(dlogit.view(B, T, 1, Fn), x["w"], None, B, T, 1, Fn, C, F1, KT=1, S=2, pad=0, prec=ops.PREC_BF16,
                                bn_bwd=(x["v"], mean, rstd, x["gamma"], x["beta"], True))
    torch.cuda.synchronize()
    return dict(u=u, mask=mask.view(rows, Fn), dlogit=dlogit, du=du, mean=mean, rstd=rstd, rm=rm, rv=rv, loss=loss.cpu()[0],
                bsums=bsums.view(-1, 2 * C).sum(0).cpu())


def _fused(c, bwd_replicas, max_blocks=0):
    """the entry point itself: poisoned outputs, pre-loaded accumulators handed over as already cleared"""
    from cruse_amd import ops
    from cruse_amd._lib import check, lib
    C, F1, B, T, rows, Fn, Fs = c["C"], c["F1"], c["B"], c["T"], c["rows"], c["Fn"], c["Fs"]
    x, P = c["dev"], ops._p
    nan = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=torch.float32)
    o = dict(u=nan(B, T, C, F1), mask=nan(rows, Fn), dlogit=nan(rows, Fn), du=nan(B, T, C, F1), mean=nan(C), rstd=nan(C),
             rm=c["rm"].cuda(), rv=c["rv"].cuda())
    loss0, sums0 = 3.25, torch.arange(1, bwd_replicas * 2 * C + 1, dtype=torch.float64).view(bwd_replicas, 2 * C) * 0.125
    loss, bsums = torch.full((1,), loss0, device="cuda", dtype=torch.float64), sums0.cuda()
    check(lib.cruse_mask_head_fwd_bwd(P(x["v"]), P(x["sums"]), c["nrep"], EPS, MOM, P(x["gamma"]), P(x["beta"]), P(x["skip"]), P(x["w"]), P(x["bias"]),
                                      P(x["nre"]), P(x["nim"]), P(x["cmag"]), B, T, C, F1, Fs, ALPHA, BETA, P(o["u"]), P(o["mean"]), P(o["rstd"]),
                                      P(o["rm"]), P(o["rv"]), P(o["mask"]), P(o["dlogit"]), P(o["du"]), P(loss), 1, P(bsums), bwd_replicas, 1,
                                      max_blocks, ops._stream()))
    torch.cuda.synchronize()
    o["loss"] = loss.cpu()[0] - loss0
    o["bsums"] = (bsums.cpu() - sums0).sum(0)
    return o


_UNFUSED = {}       # (C, F1, B, T, nrep) -> (case, unfused outputs, reference): computed once, shared, never modified


def _shared(C, F1, B, T, nrep):
    key = (C, F1, B, T, nrep)
    if key not in _UNFUSED:
        c = _case(C, F1, B, T, nrep, seed=1000 + 97 * C + 13 * B + T + nrep)
        _UNFUSED[key] = (c, _unfused(c), _reference(c))
    return _UNFUSED[key]


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _compare(c, un, fu, ref, tag):
    C = c["C"]
    for k in ("u", "mask", "dlogit", "du", "mean", "rstd", "rm", "rv"):
        assert not torch.isnan(fu[k]).any(), (tag, k, "an element was not written (or a read went outside the inputs)")
        assert _bits(fu[k], un[k]), (tag, k, float((fu[k] - un[k]).abs().max()))
    for k, old in (("rm", c["rm"]), ("rv", c["rv"])):
        assert bool((fu[k].cpu() != old).all()), (tag, k, "a running statistic was not updated")
    ref_loss, ref_g, ref_gx, mag_loss, mag_g, mag_gx = ref
    n = c["rows"] * c["Fs"]
    e_un, e_fu = abs(float(un["loss"]) - float(ref_loss)), abs(float(fu["loss"]) - float(ref_loss))
    floor = n * 2.0 ** -52 * float(mag_loss)
    print(f"{tag} loss: unfused error {e_un:.3e} fused error {e_fu:.3e} (sum {float(ref_loss):.6e}, reference resolution {floor:.1e})")
    assert np.isfinite(e_fu) and e_fu <= 2.0 * e_un + floor, (tag, "loss", e_fu, e_un)
    n = c["rows"] * c["F1"]
    for name, lo, r, mag in (("sum g", 0, ref_g, mag_g), ("sum g*xhat", C, ref_gx, mag_gx)):
        e_un = float((un["bsums"][lo:lo + C] - r).abs().max())
        e_fu = float((fu["bsums"][lo:lo + C] - r).abs().max())
        floor = n * 2.0 ** -52 * float(mag.max())
        print(f"{tag} {name}: unfused error {e_un:.3e} fused error {e_fu:.3e} (largest |sum| {float(r.abs().max()):.3e}, reference resolution {floor:.1e})")
        assert np.isfinite(e_fu) and e_fu <= 2.0 * e_un + floor, (tag, name, e_fu, e_un)


@pytest.mark.parametrize("nrep", [1, 16])
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("C,F1", SHAPES)
def test_fused_head_gives_the_bits_of_the_four_calls(C, F1, B, T, nrep):
    from cruse_amd import ops
    assert ops.BN_STAT_REPLICAS == 16
    c, un, ref = _shared(C, F1, B, T, nrep)
    _compare(c, un, _fused(c, bwd_replicas=nrep), ref, f"C{C} F{F1} B{B} T{T} nrep{nrep}")


@pytest.mark.parametrize("C,F1", SHAPES)
def test_a_workgroup_walks_several_tiles(C, F1):
    """3 clips of 33 frames are 15 tiles; two workgroups take 8 and 7 of them"""
    c, un, ref = _shared(C, F1, 3, 33, 16)
    _compare(c, un, _fused(c, bwd_replicas=16, max_blocks=2), ref, f"C{C} F{F1} two workgroups")


def test_ops_wrapper_outside_a_step():
    """ops.mask_head without an active arena: fresh accumulators, cleared by the entry point"""
    from cruse_amd import ops
    c, un, ref = _shared(8, 80, 2, 9, 16)
    x = c["dev"]
    C, F1 = c["C"], c["F1"]
    mean, rstd = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
    rm, rv = c["rm"].cuda(), c["rv"].cuda()
    bn = ops.BnIn(x["v"], x["sums"], c["nrep"], c["rows"] * F1, EPS, MOM, x["gamma"], x["beta"], mean, rstd, rm, rv, add=x["skip"])
    u, mask, loss, dlogit, du, bsums = ops.mask_head(bn, x["w"], x["bias"], x["nre"], x["nim"], x["cmag"], c["B"], c["T"], C, F1, c["Fs"], ALPHA, BETA)
    torch.cuda.synchronize()
    fu = dict(u=u, mask=mask, dlogit=dlogit, du=du, mean=mean, rstd=rstd, rm=rm, rv=rv, loss=loss.cpu()[0], bsums=bsums.view(-1, 2 * C).sum(0).cpu())
    _compare(c, un, fu, ref, "ops.mask_head")
    assert not ops.mask_head_eligible(32, 20, 41) and not ops.mask_head_eligible(8, 82, 165) and not ops.mask_head_eligible(8, 80, 160)
    with pytest.raises(RuntimeError, match="mask_head"):
        ops.mask_head(bn, x["w"], x["bias"], x["nre"], x["nim"], x["cmag"], c["B"], c["T"], C, F1, c["Fs"] - 1, ALPHA, BETA)


def test_whole_step_on_and_off():
    """TrainEngine at B = 2, T = 17 (bf16 mode, eager launches) with fuse_mask_head on and off from the same seed: the loss within 1e-6 relative;
    every gradient tensor within twice what two `off` runs differ from each other.  Where the `off` runs are bit-equal: conv1_t.weight and
    conv1_t.bias, which no atomic sum feeds (they are formed from dlogit and u_1 alone), must be bit-equal; the rest of the gradient lies behind
    the bn2_t backward sums, f64 atomics whose order is free in BOTH forms: the two per-channel means (sum / count, rounded to f32) can move by
    one f32 ulp, 2^-24 relative, and the gradient is linear in them -- 1e-5 of the tensor's largest magnitude allows for that ulp and for the
    bf16 operand roundings (2^-9) it can flip further down."""
    from cruse_amd import ops
    from cruse_amd.config import EngineConfig
    from cruse_amd.data import synth_batch
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse_net import unet_2
    hop = 160
    noisy, clean = synth_batch(2, 16 * hop, "cuda", 21)
    assert ops.stft_frames(noisy.shape[1], hop) == 17
    runs = []
    for flag in (False, False, True):
        torch.manual_seed(5)
        eng = TrainEngine(unet_2(rnn_groups=1, precision="bf16").cuda(), use_graph=False, lr=0.0, config=EngineConfig(fuse_mask_head=flag))
        ls = eng.step(noisy, clean)
        torch.cuda.synchronize()
        runs.append((eng.loss_value(ls), {n: g.clone() for n, g in eng.flat.G.items()}, eng._last_mask.clone()))
        assert eng.skipped_steps() == 0 and ops.gru_status() == 0
    (l_a, g_a, m_a), (l_b, g_b, _), (l_on, g_on, m_on) = runs
    print(f"loss off {l_a:.9e} / {l_b:.9e} on {l_on:.9e}")
    assert abs(l_on - l_a) <= 1e-6 * abs(l_a)
    assert _bits(m_on, m_a)
    for n in g_a:
        spread = float((g_a[n] - g_b[n]).abs().max())
        diff = float((g_on[n] - g_a[n]).abs().max())
        print(f"{n}: off-off {spread:.3e} on-off {diff:.3e} (max |g| {float(g_a[n].abs().max()):.3e})")
        if spread > 0.0:
            assert diff <= 2.0 * spread, (n, diff, spread)
        elif n.startswith("conv1_t."):
            assert _bits(g_on[n], g_a[n]), (n, diff)
        else:
            assert diff <= 1e-5 * float(g_a[n].abs().max()), (n, diff)
