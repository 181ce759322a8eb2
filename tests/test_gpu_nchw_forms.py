"""GPU: every kernel form of the general NCHW convolutions (6) and their weight gradients (5), in each storage type in which the form exists,
through the public entry points, against a float64 CPU convolution of the same stored values.  Each case first asks ops.nchw_conv_plan that
its shape really takes the form it is named after.  B = 2, channels that straddle a 16-row tile (24 -> 20 / 40), H x W = 5 x 19 (W no
multiple of 8, HW no multiple of 64), the depthwise 3x3 with dilation (2, 1) and causal pad, stride (1, 2) and up_w = 2 on the general kernel,
N * HS < 8 for the per-weight weight gradient.

Tolerance, from the number formats: |err| <= (n_terms 2^-24 + r) sum|w||x| + s |y|, n_terms the products of one output (f32 accumulation in
any order), r = 2 * 2^-11 on the forms that hand f16 operands to the MFMA, s = 2^-11 for f16 storage and 2^-24 for f32.  Sums that end in f64
atomics are held to (n 2^-53 + s) sum|terms| over the n terms of a channel: the f64 accumulation in any order, plus the storage rounding s of
the tensor whose stored values they sum (all the forms that serve a request store f16, the statistics pass reads what was stored).  The
reference is the float64 sum of the STORED values, so the s term is slack for how the kernels form a term and their f32 partial sums in
front of the f64 atomic: measured on an MI355X, the errors are at most 5.5e-05 absolute, 1.23 2^-24 sum|terms| (sum of y^2 behind the
LDS-transposed pointwise kernel; every other sum below 0.6 2^-24 sum|terms|) -- the unchanged kernels do not meet n 2^-53 sum|terms| alone.
Each sum's error is printed as a multiple of its bound, and of 2^-24 sum|terms|, before it is asserted."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, H, W = 2, 5, 19
DW3 = dict(KH=3, KW=3, dh=2, dw=1, pt=4, pl=1)
F32, F16 = 0, 1
TDT = {F32: torch.float32, F16: torch.float16}
S = {F32: 2.0 ** -24, F16: 2.0 ** -11}
R_MFMA = 2 * 2.0 ** -11
BN_SUMS, RESIDUAL, BNBWD, DB = 1, 2, 4, 1


def geom(Cin, Cout, KH=1, KW=1, sh=1, sw=1, dh=1, dw=1, pt=0, pl=0, groups=1, up_w=1, h=H, b=B):
    return dict(B=b, Cin=Cin, Cout=Cout, H=h, W=W, Ho=(h - 1) // sh + 1, Wo=(W * up_w - 1) // sw + 1, KH=KH, KW=KW, sh=sh, sw=sw, dh=dh, dw=dw, pt=pt,
                pl=pl, groups=groups, up_w=up_w)


# form -> (geometry, storage types, options that steer a type onto the form)
CONV = {"pw_tr_f16": (geom(24, 20), {F16: {}}),
        "pw_mfma_f16": (geom(24, 40), {F16: {}}),
        "pw": (geom(24, 40), {F32: {}, F16: {"pw_valu": 1}}),
        "dw_lds_f16": (geom(12, 12, groups=12, **DW3), {F16: {}}),
        "dw": (geom(12, 12, groups=12, **DW3), {F32: {}, F16: {"dw_nolds": 1}}),
        "general": (geom(8, 12, KH=3, KW=3, sw=2, pt=1, pl=1, up_w=2), {F32: {}, F16: {}})}
WGRAD = {"pw_mfma_f16": (geom(24, 20), {F16: {}}),
         "dw_lds_f16": (geom(12, 12, groups=12, **DW3), {F16: {}}),
         "dw": (geom(12, 12, groups=12, **DW3), {F32: {}, F16: {"dw_nolds": 1}}),
         "rows": (geom(20, 12, KH=3, KW=3, sw=2, pt=1, pl=1, up_w=2), {F32: {}, F16: {}}),
         "weight": (geom(20, 12, KH=3, KW=3, sw=2, pt=1, pl=1, up_w=2, b=1), {F32: {}, F16: {}})}


@pytest.fixture(scope="module")
def ops():
    from cruse_amd import ops as o
    return o


def plan(ops, g, dt, requests=0, wgrad=False, act=0):
    if wgrad:       # S = dy (Cout, Ho x Wo), Bg = x
        return ops.nchw_conv_plan(1, g["B"], g["Cout"], g["Ho"], g["Wo"], g["Cin"], g["H"], g["W"], g["KH"], g["KW"], g["sh"], g["sw"], g["dh"], g["dw"],
                                  g["pt"], g["pl"], g["groups"], g["up_w"], dtype=dt, requests=requests)
    return ops.nchw_conv_plan(0, g["B"], g["Cin"], g["H"], g["W"], g["Cout"], g["Ho"], g["Wo"], g["KH"], g["KW"], g["sh"], g["sw"], g["dh"], g["dw"],
                              g["pt"], g["pl"], g["groups"], g["up_w"], act=act, dtype=dt, requests=requests)


def tensors(g, dt, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g["B"], g["Cin"], g["H"], g["W"], generator=gen).to(TDT[dt])
    w = torch.randn(g["Cout"], g["Cin"] // g["groups"], g["KH"], g["KW"], generator=gen) * 0.3
    bias = torch.randn(g["Cout"], generator=gen)
    dy = torch.randn(g["B"], g["Cout"], g["Ho"], g["Wo"], generator=gen).to(TDT[dt])
    return x, w, bias, dy


def padded(x, g):
    """the zero-padded, W-upsampled input in float64: row ho * sh + kh * dh, column wo * sw + kw * dw is the tap (kh, kw) of output (ho, wo)"""
    xu = x.double().repeat_interleave(g["up_w"], dim=3)
    return F.pad(xu, (g["pl"], g["KW"] * g["dw"] + g["sw"] * g["Wo"], g["pt"], g["KH"] * g["dh"] + g["sh"] * g["Ho"]))


def conv_ref(x, w, bias, g):
    y = F.conv2d(padded(x, g), w.double(), None if bias is None else bias.double(), (g["sh"], g["sw"]), 0, (g["dh"], g["dw"]), g["groups"])
    return y[:, :, :g["Ho"], :g["Wo"]]


def wgrad_ref(dy, x, g):
    xp, d = padded(x, g), dy.double()
    G, cg, og = g["groups"], g["Cin"] // g["groups"], g["Cout"] // g["groups"]
    dw = torch.zeros(g["Cout"], cg, g["KH"], g["KW"], dtype=torch.float64)
    for kh in range(g["KH"]):
        for kw in range(g["KW"]):
            tap = xp[:, :, kh * g["dh"]:kh * g["dh"] + g["sh"] * g["Ho"]:g["sh"], kw * g["dw"]:kw * g["dw"] + g["sw"] * g["Wo"]:g["sw"]]
            dw[:, :, kh, kw] = torch.einsum("ngohw,ngchw->goc", d.view(g["B"], G, og, g["Ho"], g["Wo"]),
                                            tap.reshape(g["B"], G, cg, g["Ho"], g["Wo"])).reshape(g["Cout"], cg)
    return dw


def run_conv(x, w, bias, g, **kw):
    from cruse_amd import nn_generic as NG
    y = NG._conv_raw(x.cuda(), w.cuda(), None if bias is None else bias.cuda(), (g["Ho"], g["Wo"]), g["KH"], g["KW"], (g["sh"], g["sw"]), (g["dh"], g["dw"]),
                     g["pt"], g["pl"], g["groups"], g["up_w"], False, g["Cout"], **kw)
    torch.cuda.synchronize()
    return y.cpu()


def run_wgrad(dy, x, g, with_db):
    from cruse_amd import nn_generic as NG
    dw = torch.zeros(g["Cout"], g["Cin"] // g["groups"], g["KH"], g["KW"], device="cuda")
    db = torch.zeros(g["Cout"], device="cuda") if with_db else None
    NG._wgrad_raw(dy.cuda(), x.cuda(), dw, g["KH"], g["KW"], (g["sh"], g["sw"]), (g["dh"], g["dw"]), g["pt"], g["pl"], g["groups"], g["up_w"], db=db)
    torch.cuda.synchronize()
    return dw.cpu(), None if db is None else db.cpu()


def check_close(got, ref, mag, n_terms, r, s, what):
    bound = (n_terms * 2.0 ** -24 + r) * mag + s * ref.abs()
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: max |err| %.3e, worst err / bound %.3f" % (what, float(err.max()), worst))
    assert worst <= 1.0, what


CONV_CASES = [(f, dt) for f, (_, dts) in CONV.items() for dt in dts]
WGRAD_CASES = [(f, dt) for f, (_, dts) in WGRAD.items() for dt in dts]


@pytest.mark.parametrize("form,dt", CONV_CASES, ids=["%s-%s" % (f, "f16" if d else "f32") for f, d in CONV_CASES])
def test_conv_form(ops, form, dt):
    g, dts = CONV[form]
    x, w, bias, _ = tensors(g, dt, 11)
    with ops.options(**dts[dt]):
        assert plan(ops, g, dt, act=1)["form"] == form
        y = run_conv(x, w, bias, g, act=1)
    ref = conv_ref(x, w, bias, g)
    mag = conv_ref(x.abs(), w.abs(), bias.abs(), g)
    n = g["Cin"] // g["groups"] * g["KH"] * g["KW"] + 1
    check_close(y, ref.clamp_min(0), mag, n, R_MFMA if "mfma" in form or "tr_f16" in form else 0.0, S[dt], "conv " + form)


@pytest.mark.parametrize("form,dt", WGRAD_CASES, ids=["%s-%s" % (f, "f16" if d else "f32") for f, d in WGRAD_CASES])
def test_wgrad_form(ops, form, dt):
    g, dts = WGRAD[form]
    x, _, _, dy = tensors(g, dt, 12)
    with ops.options(**dts[dt]):
        p = plan(ops, g, dt, requests=DB, wgrad=True)
        assert p["form"] == form and (p["served"], p["pass"]) == ((DB, None) if form == "pw_mfma_f16" else (0, "channel_sum"))
        dw, db = run_wgrad(dy, x, g, True)
        dw_plain, _ = run_wgrad(dy, x, g, False)
    n = g["B"] * g["Ho"] * g["Wo"]
    r = R_MFMA if "mfma" in form else 0.0
    check_close(dw, wgrad_ref(dy, x, g), wgrad_ref(dy.abs(), x.abs(), g), n, r, 2.0 ** -24, "wgrad " + form)
    check_close(dw_plain, wgrad_ref(dy, x, g), wgrad_ref(dy.abs(), x.abs(), g), n, r, 2.0 ** -24, "wgrad (no db) " + form)
    # db, in the kernel (the pointwise MFMA form) or by the channel-sum pass: f32 sums of the stored dy
    check_close(db, dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3)), n, r, 2.0 ** -24, "db " + form)


def check_sums(got, terms, what):
    """f64 atomics over the stored f16 values: terms [B, C, H, W] float64, got [C]"""
    n = terms.shape[0] * terms.shape[2] * terms.shape[3]
    mag = terms.abs().sum((0, 2, 3))
    err = (got - terms.sum((0, 2, 3))).abs()
    worst = float((err / ((n * 2.0 ** -53 + S[F16]) * mag).clamp_min(1e-300)).max())
    print("%s: max |err| %.3e, worst err / bound %.5f, worst err / (2^-24 sum|terms|) %.3f" % (what, float(err.max()), worst,
                                                                                             float((err / (2.0 ** -24 * mag).clamp_min(1e-300)).max())))
    assert worst <= 1.0, what


@pytest.mark.parametrize("form", ["pw_tr_f16", "pw_mfma_f16", "dw_lds_f16", "general"])
def test_batch_sums_request(ops, form):
    """served by pw_tr_f16 / dw_lds_f16, a statistics pass after pw_mfma_f16 / general: y is the plain call's bit for bit"""
    g, _ = CONV[form]
    x, w, bias, _ = tensors(g, F16, 13)
    p = plan(ops, g, F16, requests=BN_SUMS)
    assert p["form"] == form and (p["served"], p["pass"]) == ((BN_SUMS, None) if form in ("pw_tr_f16", "dw_lds_f16") else (0, "stats"))
    sums = torch.zeros(8, 2 * g["Cout"], dtype=torch.float64, device="cuda")
    y = run_conv(x, w, bias, g, bn_sums=sums)
    assert torch.equal(y, run_conv(x, w, bias, g))
    got = sums.cpu().sum(0)
    yd = y.double()
    for k, terms in enumerate((yd, yd * yd)):
        check_sums(got[k * g["Cout"]:(k + 1) * g["Cout"]], terms, "batch sums %s [%d]" % (form, k))


@pytest.mark.parametrize("form", ["pw_tr_f16", "pw_mfma_f16", "dw_lds_f16"])
def test_residual_request(ops, form):
    """served by pw_tr_f16, cruse_add_nchw after the others: y = T(T(conv) + residual) either way"""
    g, _ = CONV[form]
    x, w, bias, dy = tensors(g, F16, 14)
    p = plan(ops, g, F16, requests=RESIDUAL)
    assert p["form"] == form and (p["served"], p["pass"]) == ((RESIDUAL, None) if form == "pw_tr_f16" else (0, "add"))
    y = run_conv(x, w, bias, g, residual=dy.cuda())
    assert torch.equal(y, (run_conv(x, w, bias, g).float() + dy.float()).half())


@pytest.mark.parametrize("form", ["pw_tr_f16", "dw_lds_f16", "pw_mfma_f16", "general"])
def test_bn_backward_sums_request(ops, form):
    """cruse_conv2d_nchw_bnbwd: served by pw_tr_f16 / dw_lds_f16 (*delivered = 1), not delivered by the others; y is the plain call's"""
    from cruse_amd._lib import lib, check
    g, _ = CONV[form]
    if g["up_w"] != 1:
        g = dict(g, up_w=1, Wo=(W - 1) // g["sw"] + 1)
    x, w, _, _ = tensors(g, F16, 15)
    C = g["Cout"]
    gen = torch.Generator().manual_seed(16)
    bn_x = torch.randn(g["B"], C, g["Ho"], g["Wo"], generator=gen).half()
    mean, rstd, gamma, beta = (torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5, torch.rand(C, generator=gen) + 0.5,
                               torch.randn(C, generator=gen) * 0.1)
    p = plan(ops, g, F16, requests=BNBWD)
    served = form in ("pw_tr_f16", "dw_lds_f16")
    assert p["form"] == form and p["served"] == (BNBWD if served else 0) and p["pass"] is None
    dev = [t.cuda() for t in (x, w, bn_x, mean, rstd, gamma, beta)]
    y = torch.empty(g["B"], C, g["Ho"], g["Wo"], dtype=torch.float16, device="cuda")
    r = torch.zeros(8, 4, C, dtype=torch.float64, device="cuda")
    delivered = ctypes.c_int(-1)
    ptr = [t.data_ptr() for t in dev]
    check(lib.cruse_conv2d_nchw_bnbwd(ptr[0], ptr[1], y.data_ptr(), g["B"], g["Cin"], g["H"], g["W"], C, g["Ho"], g["Wo"], g["KH"], g["KW"], g["sh"],
                                      g["sw"], g["dh"], g["dw"], g["pt"], g["pl"], g["groups"], 0, ptr[2], ptr[3], ptr[4], ptr[5], ptr[6], None, 0,
                                      r.data_ptr(), 8, ctypes.addressof(delivered), F16, None))
    torch.cuda.synchronize()
    assert delivered.value == (1 if served else 0)
    y = y.cpu()
    assert torch.equal(y, run_conv(x, w, None, g))
    if served:
        xhat = (bn_x.double() - mean.double().view(1, C, 1, 1)) * rstd.double().view(1, C, 1, 1)
        got = r.cpu().sum(0)
        for k, terms in ((0, y.double()), (1, y.double() * xhat), (3, xhat)):
            check_sums(got[k], terms, "BatchNorm-backward sums %s [%d]" % (form, k))
