"""CPU: what the general NCHW convolutions and their weight gradients launch for a call (cruse_conv2d_nchw_plan / ops.nchw_conv_plan) -- kernel
form, template case, grid, block, LDS bytes, the requests served in the kernel and the pass owed beside it -- or the error the entry point
answers with; and the library's option names.  A host-side decision: the library loads without a GPU.

The expected results (tests/golden/nchw_plan_parent.json) were recorded from the library as it was BEFORE the five entry points were put
behind call descriptors, never from the code under test.  A build of the parent commit got a scratch patch, kept out of the repository: in
generic.hip every launch of conv2d_nchw_t / wgrad_nchw_t wrote (form, two template integers, grid x / y / z, block, LDS bytes, run or band or
the epilogue instance) into a caller-supplied array and returned instead of launching; the tails of cruse_conv2d_nchw_ex / _bnbwd and the
channel-sum call of the weight gradient wrote, from the out-flags, which requests the kernel had served and which pass they would have
run, and ran none; "dw_nolds" -- read by the dispatcher, missing from the option table -- was made settable.  That build's own entry points
(the one entry() below picks for a case) were called with 16-byte aligned stand-in pointers over cases(), and their return code, the entry
name in front of cruse_last_error() and the array were written down.  Layout of the file: "results", the distinct outcomes (the eleven
figures, or [code, entry name] of a refusal); "index", one entry into "results" per case of cases(), in that order."""
import ctypes
import itertools
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nchw_plan_parent.json")
F32, F16 = 0, 1
BN_SUMS, RESIDUAL, BNBWD, DB = 1, 2, 4, 1
E_SHAPE, E_DTYPE = -1, -3
DTYPES = (F32, F16)
PW_VALU = ((), (("pw_valu", 1),), (("pw_valu", 2),))
NOLDS = ((), (("dw_nolds", 1),))


def conv(B, Cin, Cout, H, W, KH=1, KW=1, sh=1, sw=1, dh=1, dw=1, pt=0, pl=0, groups=1, up_w=1, transposed=0):
    """the 18 geometry integers of cruse_conv2d_nchw; the output keeps the input's size but for stride and upsampling"""
    Ho, Wo = (H * sh, W * sw) if transposed else ((H - 1) // max(sh, 1) + 1, (W * up_w - 1) // max(sw, 1) + 1)
    return (B, Cin, H, W, Cout, Ho, Wo, KH, KW, sh, sw, dh, dw, pt, pl, groups, up_w, transposed)


def wgrad(N, CA, CB, HS, WS, KH=1, KW=1, sh=1, sw=1, dh=1, dw=1, pt=0, pl=0, groups=1, up_w=1):
    """the 17 geometry integers of cruse_conv2d_nchw_wgrad (S the strided side)"""
    return (N, CA, HS, WS, CB, HS * sh, WS * sw // max(up_w, 1), KH, KW, sh, sw, dh, dw, pt, pl, groups, up_w)


DW3 = dict(KH=3, KW=3, dh=2, dw=1, pt=4, pl=1)             # TFCM_Block's dilated causal 3x3


def _conv_cases():
    """(options, geometry, act, accumulate, dtype, requests)"""
    for opt, dt, tr in itertools.product(PW_VALU, DTYPES, (0, 1)):
        for Cout, Cin in itertools.product((16, 17, 32, 33, 64, 65), (32, 33, 64, 65, 128, 129, 256, 257)):      # pointwise: every tile edge
            for acc in (0, 1):
                yield opt, conv(2, Cin, Cout, 5, 19, transposed=tr), 0, acc, dt, 0
        for (Cin, Cout), HW in itertools.product(((24, 40), (64, 64), (128, 40), (200, 48), (257, 65)), (1, 63, 64 * 4 * 768 + 1)):   # the block caps
            yield opt, conv(1, Cin, Cout, 1, HW, transposed=tr), 0, 0, dt, 0
            yield opt, conv(64, Cin, Cout, 1, HW, transposed=tr), 0, 0, dt, 0
        for nolds, W in itertools.product(NOLDS, (19, 401, 5000)):                              # depthwise: the LDS image fits 60 KB up to W = 3839
            yield opt + nolds, conv(2, 4, 4, 16, W, groups=4, transposed=tr, **DW3), 0, 0, dt, 0
            yield opt + nolds, conv(8, 24, 24, 161, W, groups=24, transposed=tr, **DW3), 1, 0, dt, 0
        yield opt, conv(2, 6, 6, 9, 19, KH=2, KW=5, pt=1, pl=2, groups=6, transposed=tr), 0, 0, dt, 0      # 10 taps: the general kernel
        for C in (65535, 65536):                                                                  # grid.y = B * Cout planes
            yield opt, conv(1, C, C, 4, 19, groups=C, transposed=tr, **DW3), 0, 0, dt, 0
        for g in (1, 2, 8):
            yield opt, conv(2, 8, 8, 9, 19, KH=3, KW=3, sh=1, sw=2, pt=1, pl=1, groups=g, transposed=tr), 0, 0, dt, 0           # strided (also depthwise)
            if not tr:
                yield opt, conv(2, 8, 8, 9, 19, KH=3, KW=3, pt=1, pl=1, groups=g, up_w=2), 2, 0, dt, 0
        # each request on each form: served in the kernel, or a pass owed
        forms = [conv(2, 24, 20, 5, 19, transposed=tr), conv(2, 24, 40, 5, 19, transposed=tr), conv(2, 200, 48, 5, 19, transposed=tr),
                 conv(2, 12, 12, 5, 19, groups=12, transposed=tr, **DW3), conv(2, 12, 12, 5, 5000, groups=12, transposed=tr, **DW3),
                 conv(2, 12, 20, 5, 19, KH=3, KW=3, pt=1, pl=1, transposed=tr)]
        for geom, req in itertools.product(forms, (0, BN_SUMS, RESIDUAL, BNBWD)):
            yield opt, geom, 0, 0, dt, req
        yield opt, forms[0], 1, 0, dt, BN_SUMS
    # refusals: one per CRUSE_REQUIRE of cruse_conv2d_nchw, _ex and _bnbwd that integers can reach
    ok = dict(B=2, Cin=8, Cout=8, H=5, W=19, KH=3, KW=3, pt=1, pl=1)
    for req in (0, BN_SUMS, BNBWD):
        yield (), conv(**dict(ok, B=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, W=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, KH=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, sw=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, dh=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, groups=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, groups=3)), 0, 0, F16, req
        yield (), conv(**ok), 0, 0, 2, req                     # CRUSE_DT_BF16 is no storage type here
        yield (), conv(**dict(ok, groups=0)), 0, 0, 7, req     # a shape error wins over a dtype error
    for req in (0, BN_SUMS):
        yield (), conv(**dict(ok, up_w=0)), 0, 0, F16, req
        yield (), conv(**dict(ok, up_w=2))[:17] + (1,), 0, 0, F16, req       # transposed with upsampling
        yield (), conv(**ok), 3, 0, F16, req
        yield (), conv(**ok), -1, 0, F32, req
    yield (), conv(**ok), 1, 1, F32, 0                         # accumulate with an activation
    yield (), conv(**ok), 0, 0, F16, BN_SUMS | RESIDUAL       # statistics of a sum


def _wgrad_cases():
    """(options, geometry, dtype, requests)"""
    for opt, dt, db in itertools.product(PW_VALU, DTYPES, (0, DB)):
        for CA, CB in itertools.product((8, 16, 17, 32, 33), (8, 15, 16, 17, 31, 32, 33)):       # pointwise; db in the kernel: CB % 16, CB < 32, CA <= 32
            yield opt, wgrad(2, CA, CB, 5, 19), dt, db
        for N, HS, WS in ((1, 1, 1), (8, 161, 401), (16, 161, 401), (3, 64, 1024)):              # run: 1024, 2048, 4096
            yield opt, wgrad(N, 24, 40 if N == 3 else 24, HS, WS), dt, db
        for W in (400, 401):                                                                      # a row pair: 150 KB = (48 + 48) * 400 floats
            yield opt, wgrad(2, 48, 48, 5, W, KH=3, KW=3, pt=1, pl=1), dt, db
        for N, HS in ((1, 7), (1, 8), (7, 1), (2, 4)):                                            # N * HS = 7 / 8
            yield opt, wgrad(N, 12, 20, HS, 19, KH=3, KW=3, pt=1, pl=1), dt, db
        for N, CA, CB, K in ((1, 12, 20, 3), (3, 12, 20, 1), (3, 4, 4, 1), (5, 4, 4, 3), (2, 64, 64, 3), (64, 2, 2, 1)):     # the ny loop: 1, clamped to N, doubled
            yield opt, wgrad(N, CA, CB, 2, 19, KH=K, KW=K, pt=K // 2, pl=K // 2), dt, db
        yield opt, wgrad(2, 8, 8, 5, 19, KH=3, KW=3, pt=1, pl=1, groups=2), dt, db
        yield opt, wgrad(2, 8, 8, 9, 38, KH=3, KW=3, pt=1, pl=1, up_w=2), dt, db
        for nolds in NOLDS:
            for N, C, HS, WS in ((2, 12, 5, 19), (8, 24, 161, 401), (64, 32, 161, 401), (2, 4, 16, 5000), (1, 1, 1, 1), (1, 8, 64, 1024), (1, 65535, 4, 19),
                                 (1, 65536, 4, 19)):                                               # the band loop: 4, 8, 16; the LDS image
                yield opt + nolds, wgrad(N, C, C, HS, WS, groups=C, **DW3), dt, db
            yield opt + nolds, wgrad(2, 12, 12, 5, 19, KH=3, KW=3, sh=2, sw=2, pt=1, pl=1, groups=12), dt, db        # strided depthwise: no LDS form
            yield opt + nolds, wgrad(2, 12, 12, 5, 19, KH=2, KW=5, pt=1, pl=2, groups=12), dt, db                    # 10 taps
    ok = dict(N=2, CA=8, CB=8, HS=5, WS=19, KH=3, KW=3, pt=1, pl=1)
    for db in (0, DB):
        yield (), wgrad(**dict(ok, N=0)), F16, db
        yield (), wgrad(**dict(ok, KW=0)), F16, db
        yield (), wgrad(**dict(ok, groups=3)), F16, db
        yield (), wgrad(**dict(ok, up_w=0)), F16, db
        yield (), wgrad(**ok), 2, db
        yield (), wgrad(**dict(ok, groups=3)), 9, db


def cases():
    """("conv", options, geometry, act, accumulate, dtype, requests) and ("wgrad", options, geometry, 0, 0, dtype, requests), in the order of
    the recorded file"""
    for opt, geom, act, acc, dt, req in _conv_cases():
        yield "conv", opt, geom, act, acc, dt, req
    for opt, geom, dt, req in _wgrad_cases():
        yield "wgrad", opt, geom, 0, 0, dt, req


# refusals only a pointer or an argument outside the plan's reach triggers: (entry point, changed argument) through the real entry points --
# refused before any launch, so they run wherever the library loads
DIRECT = (("cruse_conv2d_nchw", "slope"), ("cruse_conv2d_nchw_ex", "slope"), ("cruse_conv2d_nchw_ex", "bn_nrep"), ("cruse_conv2d_nchw_bnbwd", "bn_x"),
          ("cruse_conv2d_nchw_bnbwd", "bn_act"), ("cruse_conv2d_nchw_bnbwd", "bn_slope"), ("cruse_conv2d_nchw_bnbwd", "r_nrep"),
          ("cruse_conv2d_nchw_bnbwd", "delivered"))


def entry(case):
    """the entry point a case is a call of"""
    kind, _, _, _, _, _, req = case
    if kind == "wgrad":
        return "cruse_conv2d_nchw_wgrad_ex" if req else "cruse_conv2d_nchw_wgrad"
    return "cruse_conv2d_nchw_bnbwd" if req & BNBWD else "cruse_conv2d_nchw_ex" if req else "cruse_conv2d_nchw"


_BUF = ctypes.create_string_buffer(64)
_DEV = []


def standin():
    """a 16-byte aligned stand-in for every tensor: the host only asks whether a pointer is null.  These calls are made where they must be
    refused; should a check regress, the entry point would launch on the stand-in, so where a device is present it is 1 MiB of device memory
    (more than the tensors of any refused case here), and host memory only where nothing can launch"""
    import torch
    if torch.cuda.is_available():
        if not _DEV:
            _DEV.append(torch.zeros(1 << 18, dtype=torch.float32, device="cuda"))
        return _DEV[0].data_ptr()
    return (ctypes.addressof(_BUF) + 15) & ~15


def call_entry(lib, case, direct=None):
    """the call of the real entry point (ctypes library handle with cruse_amd._lib's signatures) for a case; only where it is refused does it
    launch nothing.  direct: the DIRECT argument to spoil"""
    kind, _, g, act, acc, dt, req = case
    P = standin()
    if kind == "wgrad":
        if req:
            return lib.cruse_conv2d_nchw_wgrad_ex(P, P, P, P, *g, dt, None)
        return lib.cruse_conv2d_nchw_wgrad(P, P, P, *g, dt, None)
    slope = P if act == 2 else None
    if req & BNBWD:
        a = dict(bn_x=P, bn_slope=None, bn_act=0, r_nrep=1, delivered=ctypes.addressof(_BUF) + 32)
        a.update({"bn_x": {"bn_x": None}, "bn_act": {"bn_act": 4}, "bn_slope": {"bn_act": 2}, "r_nrep": {"r_nrep": 0},
                  "delivered": {"delivered": None}}.get(direct, {}))
        return lib.cruse_conv2d_nchw_bnbwd(P, P, P, *g[:16], g[17], a["bn_x"], P, P, P, P, a["bn_slope"], a["bn_act"], P, a["r_nrep"], a["delivered"], dt, None)
    if direct == "slope":
        act, slope = 2, None
    if req:
        return lib.cruse_conv2d_nchw_ex(P, P, None, P if req & RESIDUAL else None, P, *g, act, slope, P if req & BN_SUMS else None,
                                        0 if direct == "bn_nrep" else 1, dt, None)
    return lib.cruse_conv2d_nchw(P, P, None, P, *g, act, slope, acc, dt, None)


def refusal(lib, rc):
    """the recorded form of a refusal: [code, entry name in front of the message]"""
    return [rc, lib.cruse_last_error().decode().partition(":")[0]]


def direct_case(name):
    req = {"cruse_conv2d_nchw": 0, "cruse_conv2d_nchw_ex": BN_SUMS, "cruse_conv2d_nchw_bnbwd": BNBWD}[name]
    return ("conv", (), conv(2, 8, 8, 5, 19, KH=3, KW=3, pt=1, pl=1), 0, 0, F16, req)


@pytest.fixture(scope="module")
def ops():
    from cruse_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        d = json.load(f)
    assert len(d["index"]) == sum(1 for _ in cases()) and len(d["direct"]) == len(DIRECT)
    return d


def _plan(ops, case):
    kind, _, g, act, acc, dt, req = case
    geom = g if kind == "conv" else g + (0,)
    try:
        return ops.nchw_conv_plan(kind == "wgrad", *geom, act=act, accumulate=acc, dtype=dt, requests=req)["raw"]
    except RuntimeError as e:
        head, _, msg = str(e).partition(": ")
        return [int(head.rsplit(" ", 1)[1]), msg.partition(":")[0]]


def test_the_recorded_file_reaches_every_form(golden):
    plans = [(c[0], golden["results"][i]) for c, i in zip(cases(), golden["index"]) if len(golden["results"][i]) == 11]
    assert {r[0] for k, r in plans if k == "conv"} == set(range(6))
    assert {r[0] for k, r in plans if k == "wgrad"} == set(range(5))
    # served in the kernel and owed as a pass, for every request
    conv_req = {(c[6], r[9], r[10]) for c, i in zip(cases(), golden["index"]) for r in [golden["results"][i]] if c[0] == "conv" and len(r) == 11}
    assert {(BN_SUMS, BN_SUMS, 0), (BN_SUMS, 0, 2), (RESIDUAL, RESIDUAL, 0), (RESIDUAL, 0, 1), (BNBWD, BNBWD, 0), (BNBWD, 0, 0)} <= conv_req
    wg_req = {(c[6], r[9], r[10]) for c, i in zip(cases(), golden["index"]) for r in [golden["results"][i]] if c[0] == "wgrad" and len(r) == 11}
    assert wg_req == {(0, 0, 0), (DB, DB, 0), (DB, 0, 3)}
    refused = {tuple(golden["results"][i]) for i in golden["index"] if len(golden["results"][i]) == 2} | {tuple(r) for r in golden["direct"]}
    assert {name for _, name in refused} == {"conv2d_nchw", "conv2d_nchw_ex", "conv2d_nchw_bnbwd", "conv2d_nchw_wgrad", "conv2d_nchw_wgrad_ex"}
    assert {code for code, _ in refused} == {E_SHAPE, E_DTYPE}


def test_nchw_plan_is_what_the_parent_launched(ops, golden):
    from cruse_amd._lib import lib
    by_opt = {}
    for case, i in zip(cases(), golden["index"]):
        by_opt.setdefault(case[1], []).append((case, golden["results"][i]))
    for opt, rows in by_opt.items():
        with ops.options(**dict(opt)):
            for case, want in rows:
                got = _plan(ops, case)
                assert got == want, (case, got, want)
                if len(want) == 2:                     # a refusal: the entry point itself answers the same
                    assert refusal(lib, call_entry(lib, case)) == want, (case, want)
        assert all(ops.get_option(k) is None for k, _ in opt)


def test_refusals_the_plan_cannot_express(golden):
    from cruse_amd._lib import lib
    for (name, arg), want in zip(DIRECT, golden["direct"]):
        assert refusal(lib, call_entry(lib, direct_case(name), direct=arg)) == want == [E_SHAPE, name[len("cruse_"):]], (name, arg)


@pytest.mark.parametrize("bad", [dict(groups=0), dict(sh=0), dict(sw=0), dict(dh=0), dict(dw=0), dict(groups=-1), dict(sh=-2)])
@pytest.mark.parametrize("db", [0, DB])
def test_wgrad_refuses_what_it_used_to_divide_by(ops, db, bad):
    """new with the shared validation (the parent evaluated CA % groups with groups = 0): CRUSE_E_SHAPE, from the plan and from the entry point"""
    from cruse_amd._lib import lib
    g = wgrad(2, 8, 8, 5, 19, KH=3, KW=3, pt=1, pl=1)
    names = ("N", "CA", "HS", "WS", "CB", "HB", "WB", "KH", "KW", "sh", "sw", "dh", "dw", "pt", "pl", "groups", "up_w")
    g = tuple(bad.get(n, v) for n, v in zip(names, g))
    case = ("wgrad", (), g, 0, 0, F16, db)
    name = "conv2d_nchw_wgrad_ex" if db else "conv2d_nchw_wgrad"
    assert _plan(ops, case) == [E_SHAPE, name]
    assert refusal(lib, call_entry(lib, case)) == [E_SHAPE, name]


def test_plan_refuses_requests_that_name_no_entry_point(ops):
    g = conv(2, 24, 40, 5, 19)
    for kw in (dict(requests=8), dict(requests=BN_SUMS | BNBWD), dict(requests=BN_SUMS, accumulate=1), dict(requests=BNBWD, act=1)):
        with pytest.raises(RuntimeError, match="conv2d_nchw_plan"):
            ops.nchw_conv_plan(0, *g, dtype=F16, **kw)
    with pytest.raises(RuntimeError, match="conv2d_nchw_plan"):
        ops.nchw_conv_plan(1, *wgrad(2, 8, 8, 5, 19), 0, dtype=F16, requests=2)


def test_every_configured_option_can_be_set_and_read_back(ops):
    from cruse_amd.config import EngineConfig
    names = sorted(set(EngineConfig._LIB_ENV.values()) | {"cm_grid", "cm_dbg", "dw_nolds"})
    assert len(names) == 17                                             # the whole list of include/cruse_hip.h
    for i, name in enumerate(names):
        assert ops.get_option(name) is None
        ops.set_option(name, 3 + i)
        try:
            assert ops.get_option(name) == 3 + i
        finally:
            ops.set_option(name, None)
        assert ops.get_option(name) is None
    for name in ("wgpw_run", "wgpw_blocks", "wgpw_dbg", "lnb_grid", "gb_deep", "wg_tfw", "pw_value", ""):
        with pytest.raises(RuntimeError, match="unknown option"):
            ops.set_option(name, 1)
        with pytest.raises(RuntimeError, match="unknown option"):
            ops.get_option(name)


def test_the_header_lists_exactly_the_options():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "cruse_amd", "csrc", "common.h")) as f:
        src = f.read()
    listed = re.findall(r"X\((\w+)\)", src[src.index("#define CRUSE_OPTIONS(X)"):src.index("#define CRUSE_OPT_ENUM")])
    with open(os.path.join(root, "include", "cruse_hip.h")) as f:
        hdr = f.read()
    comment = hdr[hdr.index("/* Library options"):hdr.index("int cruse_set_option")]
    assert sorted(re.findall(r'"(\w+)"', comment)) == sorted(listed) and len(listed) == 17
