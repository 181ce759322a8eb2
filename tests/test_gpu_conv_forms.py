"""GPU: every fused form of the frame-major convolutions equals its unfused composition, through the public ops wrappers, for gather
and scatter2 on both routes (MFMA / VALU; ops.conv_plan says which a shape takes).  The ten entry points share one host path
(conv_run, csrc/conv.hip); these are the cells where the former gather / scatter2 copies of it could have drifted apart.

Shapes: B = 2, T = 7 -- not a multiple of the 8-frame time tile of either route, two workgroups -- at the level-3 geometry (Cin, Cout, Fin, Fout) = (16, 32, 40, 20), KT = 2, S = 2, pad = 1 for
gather and its decoder mirror (32, 16, 20, 40) for scatter2 (both tap classes); the VALU route is the same with 3 input channels.

Bounds.  Outputs of the same kernel with another epilogue, and everything the library computes by literally running the separate calls,
must be bit-identical.  Batch sums are f64 accumulations of f32 partial sums taken in another order than the separate pass takes them:
rel_l2 < 1e-6, the bound tests/test_gpu_kernels.py holds replica sums to (test_conv_bnstats_epilogue, which checks the _bnstats sums
of the KT = 1 decoder form and of all encoder levels against torch; test_conv_dgrad_accumulates_the_batchnorm_backward_sums and
test_conv_data_gradient_with_fused_batchnorm_backward_input check _bnbwd / _bnbwd_in on other shapes at T = 21)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T = 2, 7
ROWS = B * T
FORMS = ("gather", "scatter2")
ROUTES = ("mfma", "valu")


@pytest.fixture(scope="module")
def ops():
    from cruse_amd import ops as o
    return o


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def shape(form, route, Cout=None):
    """(Cin, Fin, Cout, Fout) of the cell"""
    Cin, Fin, Co, Fout = (16, 40, 32, 20) if form == "gather" else (32, 20, 16, 40)
    return (3 if route == "valu" else Cin), Fin, Cout or Co, Fout


def weight(form, Cin, Cout):
    return (0.2 * torch.randn(Cout, Cin, 2, 3) if form == "gather" else 0.2 * torch.randn(Cin, Cout, 2, 3)).cuda()


def plan(ops, form, Cin, Fin, Cout, Fout, prec, **kw):
    return ops.conv_plan(form == "scatter2", Cin, Fin, Cout, Fout, 2, 2, 1, 0, B, T, prec, **kw)


def call(ops, form, suffix, head, w, tail, Cin, Fin, Cout, Fout, **kw):
    """ops.conv_<form><suffix>(*head, w, *tail, <geometry>, KT = 2, [S = 2,] pad = 1, **kw)"""
    geom = (B, T, Cin, Fin, Cout, Fout, 2, 2, 1) if form == "gather" else (B, T, Cin, Fin, Cout, 2, 1)
    return getattr(ops, f"conv_{form}{suffix}")(*head, w, *tail, *geom, **kw)


def fold(ops, sums, C):
    return sums.view(-1, 2 * C).sum(0)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("form", FORMS)
def test_bnstats_is_the_conv_followed_by_bn_stats(ops, form, route):
    torch.manual_seed(11)
    Cin, Fin, Cout, Fout = shape(form, route)
    assert plan(ops, form, Cin, Fin, Cout, Fout, "bf16x3", forms=ops.CONV_FORM_SUMS)["route"] == route
    x = (torch.randn(B, T, Cin, Fin) + 0.3).cuda(); w = weight(form, Cin, Cout); b = torch.randn(Cout).cuda()
    y0 = call(ops, form, "", (x,), w, (b,), Cin, Fin, Cout, Fout, prec="bf16x3")
    y, sums = call(ops, form, "_bnstats", (x,), w, (b,), Cin, Fin, Cout, Fout, prec="bf16x3")
    assert torch.equal(y, y0)
    assert sums.numel() == ops.BN_STAT_REPLICAS * 2 * Cout
    assert rel_l2(fold(ops, sums, Cout), ops.bn_stats(y0, ROWS, Cout, Fout)) < 1e-6


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("form", FORMS)
def test_bnbwd_is_the_conv_followed_by_the_backward_reduce(ops, form, route):
    from cruse_amd._lib import check, lib
    torch.manual_seed(12)
    Cin, Fin, Cout, Fout = shape(form, route)
    assert plan(ops, form, Cin, Fin, Cout, Fout, ops.PREC_BF16, forms=ops.CONV_FORM_BNB)["route"] == route
    x = torch.randn(B, T, Cin, Fin).cuda(); w = weight(form, Cin, Cout)
    by = torch.randn(B, T, Cout, Fout).cuda()
    mean = (0.1 * torch.randn(Cout)).cuda(); rstd = (1.0 + 0.2 * torch.rand(Cout)).cuda()
    gamma = (1.0 + 0.3 * torch.randn(Cout)).cuda(); beta = (0.2 * torch.randn(Cout)).cuda()
    y0 = call(ops, form, "", (x,), w, (None,), Cin, Fin, Cout, Fout, prec=ops.PREC_BF16)
    y, sums = call(ops, form, "", (x,), w, (None,), Cin, Fin, Cout, Fout, prec=ops.PREC_BF16, bn_bwd=(by, mean, rstd, gamma, beta, True))
    assert torch.equal(y, y0)
    ref = torch.zeros(2 * Cout, dtype=torch.float64).cuda()
    p = lambda t_: t_.data_ptr()
    check(lib.cruse_bn_act_bwd_reduce(p(y0), p(by), p(mean), p(rstd), p(gamma), p(beta), ROWS, Cout, Fout, 1, p(ref), 1,
                                      torch.cuda.current_stream().cuda_stream))
    assert rel_l2(fold(ops, sums, Cout), ref) < 1e-6


def _bwd_in_inputs(ops, Cin, Fin, Cout, Fout, dout_bf16):
    dout = torch.randn(B, T, Cin, Fin).cuda()
    dout = dout.bfloat16() if dout_bf16 else dout
    y_in = torch.randn(B, T, Cin, Fin).cuda()
    mean = y_in.mean(dim=(0, 1, 3)).contiguous(); rstd = (1.0 / (y_in.var(dim=(0, 1, 3), unbiased=False) + 1e-5).sqrt()).contiguous()
    gamma = (torch.rand(Cin) + 0.5).cuda(); beta = (0.1 * torch.randn(Cin)).cuda()
    xh = (y_in - mean.view(1, 1, -1, 1)) * rstd.view(1, 1, -1, 1)
    g = dout.float() * ((xh * gamma.view(1, 1, -1, 1) + beta.view(1, 1, -1, 1)) > 0)
    sums = torch.zeros(ops.BN_STAT_REPLICAS, 2 * Cin, dtype=torch.float64).cuda()          # replica 0 holds them, as after the reduce pass
    sums[0, :Cin] = g.double().sum(dim=(0, 1, 3)); sums[0, Cin:] = (g.double() * xh.double()).sum(dim=(0, 1, 3))
    by = torch.randn(B, T, Cout, Fout).cuda()
    bnb = (by, (0.1 * torch.randn(Cout)).cuda(), (1.0 + 0.2 * torch.rand(Cout)).cuda(), (torch.rand(Cout) + 0.5).cuda(),
           (0.1 * torch.randn(Cout)).cuda(), True)
    return dout, (y_in, mean, rstd, gamma, beta, sums), bnb


@pytest.mark.parametrize("variant", ["fused", "f32_dout", "cout64"])
@pytest.mark.parametrize("form", FORMS)
def test_bwd_in_is_the_batchnorm_backward_apply_followed_by_the_data_gradient(ops, form, variant):
    """fused: bf16 dout, Cout <= 32 -- the MFMA kernel forms dy while staging; f32_dout: refused without an attempt; cout64: refused after
    the attempt (64-row tiles).  The refused variants ARE the two separate calls: every result bit-identical."""
    torch.manual_seed(13)
    Cin, Fin, Cout, Fout = shape(form, "mfma", Cout=64 if variant == "cout64" else None)
    dout, bn, bnb = _bwd_in_inputs(ops, Cin, Fin, Cout, Fout, variant != "f32_dout")
    pl = plan(ops, form, Cin, Fin, Cout, Fout, ops.PREC_BF16, forms=ops.CONV_FORM_BBI | ops.CONV_FORM_BNB,
              x_dtype=0 if variant == "f32_dout" else 2)
    assert pl["route"] == "mfma" and pl["fused"] == (variant == "fused")
    w = weight(form, Cin, Cout)
    res = []
    for fused in (True, False):
        dg = torch.zeros(Cin).cuda(); db = torch.zeros(Cin).cuda()
        if fused:
            out, osums, dy = call(ops, form, "_bwd_in", (dout, bn + (True, True, dg, db, None)), w, (), Cin, Fin, Cout, Fout,
                                  prec=ops.PREC_BF16, bn_bwd=bnb)
        else:
            dy = ops.bn_act_bwd(dout, *bn[:5], ROWS, Cin, Fin, True, True, dg, db, sums=bn[5], out_bf16=True)
            out, osums = call(ops, form, "", (dy,), w, (None,), Cin, Fin, Cout, Fout, prec=ops.PREC_BF16, bn_bwd=bnb)
        res.append((dy.float(), out, osums.clone(), dg, db))
    for a, b_, name in zip(res[0], res[1], ("dy", "out", "sums", "dgamma", "dbeta")):
        if name == "sums" and variant == "fused":
            assert rel_l2(fold(ops, a, Cout), fold(ops, b_, Cout)) < 1e-6
        else:
            assert torch.equal(a, b_), (variant, name)


@pytest.mark.parametrize("form", FORMS)
def test_bwd_in_on_the_valu_route_is_refused_like_its_second_call(ops, form):
    """no VALU kernel reads a bf16 dy: the fallback's data-gradient call is refused, with the message of the plain call"""
    torch.manual_seed(14)
    Cin, Fin, Cout, Fout = shape(form, "valu")
    dout, bn, _ = _bwd_in_inputs(ops, Cin, Fin, Cout, Fout, True)
    w = weight(form, Cin, Cout)
    dg = torch.zeros(Cin).cuda(); db = torch.zeros(Cin).cuda()
    msgs = []
    for suffix, head, tail in (("_bwd_in", (dout, bn + (True, True, dg, db, None)), ()), ("", (dout,), (None,))):
        with pytest.raises(RuntimeError, match="a bf16 input / output needs the MFMA kernel") as e:
            call(ops, form, suffix, head, w, tail, Cin, Fin, Cout, Fout, prec=ops.PREC_BF16)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_bnin_is_bn_finalize_act_fwd_followed_by_the_conv(ops, form, add):
    """two consumers of one virtual tensor, `publish` on exactly one: both outputs are the conv of the materialised tensor, mean / rstd and
    the running statistics are written once"""
    torch.manual_seed(15)
    Cin, Fin, Cout, Fout = shape(form, "mfma")
    assert plan(ops, form, Cin, Fin, Cout, Fout, "bf16", forms=ops.CONV_FORM_BNI)["route"] == "mfma"
    y_pre = (torch.randn(B, T, Cin, Fin) + 0.2).cuda(); w = weight(form, Cin, Cout); b = torch.randn(Cout).cuda()
    skip = torch.randn(B, T, Cin, Fin).cuda() if add else None
    gamma = (torch.rand(Cin) + 0.5).cuda(); beta = (0.1 * torch.randn(Cin)).cuda()
    sums = torch.zeros(ops.BN_STAT_REPLICAS, 2 * Cin, dtype=torch.float64).cuda()
    sums[0] = ops.bn_stats(y_pre, ROWS, Cin, Fin)
    rm0 = torch.randn(Cin).cuda(); rv0 = (torch.rand(Cin) + 0.5).cuda()
    rm_ref, rv_ref = rm0.clone(), rv0.clone()
    e_bf16 = torch.empty(B, T, Cin, Fin, dtype=torch.bfloat16).cuda()
    e, mean_ref, rstd_ref = ops.bn_finalize_act_fwd(y_pre, sums, ROWS * Fin, 1e-5, 0.1, gamma, beta, skip, ROWS, Cin, Fin, running_mean=rm_ref,
                                                    running_var=rv_ref, out_bf16=e_bf16)
    y_ref, s_ref = call(ops, form, "_bnstats", (e,), w, (b,), Cin, Fin, Cout, Fout, prec="bf16")
    rm, rv = rm0.clone(), rv0.clone()
    mean = torch.full((Cin,), float("nan")).cuda(); rstd = torch.full((Cin,), float("nan")).cuda()
    bn = ops.BnIn(y_pre, sums, ops.BN_STAT_REPLICAS, ROWS * Fin, 1e-5, 0.1, gamma, beta, mean, rstd, rm, rv, add=skip)
    copy = torch.empty_like(e_bf16)
    y1 = call(ops, form, "_bnin", (bn,), w, (b,), Cin, Fin, Cout, Fout, prec="bf16")                              # publish = False
    assert torch.isnan(mean).all() and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    y2, s2 = call(ops, form, "_bnin", (bn,), w, (b,), Cin, Fin, Cout, Fout, prec="bf16", publish=True, copy_bf16=copy, want_sums=True)
    assert torch.equal(y1, y_ref) and torch.equal(y2, y_ref)
    assert torch.equal(mean, mean_ref) and torch.equal(rstd, rstd_ref) and torch.equal(rm, rm_ref) and torch.equal(rv, rv_ref)
    assert torch.equal(copy, e_bf16)
    assert rel_l2(fold(ops, s2, Cout), fold(ops, s_ref, Cout)) < 1e-6


@pytest.mark.parametrize("form", FORMS)
def test_bnin_on_the_valu_route_is_refused(ops, form):
    Cin, Fin, Cout, Fout = shape(form, "valu")
    z = torch.zeros(B, T, Cin, Fin).cuda(); c = torch.ones(Cin).cuda()
    bn = ops.BnIn(z, torch.zeros(ops.BN_STAT_REPLICAS, 2 * Cin, dtype=torch.float64).cuda(), ops.BN_STAT_REPLICAS, ROWS * Fin, 1e-5, 0.1, c, c, c, c)
    with pytest.raises(RuntimeError, match=f"conv_{form}_bnin: the fused input BatchNorm needs the MFMA kernel"):
        call(ops, form, "_bnin", (bn,), weight(form, Cin, Cout), (None,), Cin, Fin, Cout, Fout, prec="bf16")
