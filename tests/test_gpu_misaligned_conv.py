"""GPU: the convolution and weight-gradient routes chosen from operand alignment, on views that are not 16-byte aligned.

Companion of test_gpu_misaligned.py (same helper, same rules).  The branches read before an operand was moved:
  conv.hip, stage_rows: float4 staging of x needs Fin % 4 == 0 and x % 16 == 0, else the element loop (tested in the kernel);
  conv_mfma.hip, cm_plan: the MFMA kernels need x % 16 == 0, else the call takes the VALU kernel;
  conv_mfma.hip, launch_mt: the swapped-role (vector-store) forms need y and bn_y % 16 == 0, else the 4-byte stores of the plain form;
  wgrad_mfma.hip, cruse_wgrad_mfma_plan: a, bt % 16 == 0, else not this kernel;  wgrad_rd.hip, cruse_wgrad_rd_plan: a, bt % 4 == 0
  (its 16-byte loads are declared 4-byte aligned), else not this kernel;  the VALU weight-gradient kernel loads 4 bytes at a time.
Only x, the f32 output of an MFMA-eligible call (by 8 bytes) and a / bt are moved.  The reference is the plain-C twin (oracle/cruse_ref.c:
float64 accumulation of the same f32 inputs); the bars are those of test_gpu_abi_ref.py: convolutions 2e-5 max-rel exact, rel-L2 1e-4
split-bf16 and 2e-2 bf16; weight gradients 3e-5 max-rel exact / f32, rel-L2 2e-2 bf16."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_lib as R  # noqa: E402
from misalign import bf16_bits, bf16_value, max_rel, place, rel_l2  # noqa: E402
from test_gpu_misaligned import Tally, rnd, st  # noqa: E402
from test_wgrad_route_host import RAGGED_SHAPES  # noqa: E402

pytestmark = pytest.mark.gpu
B, T = 2, 5
CONV_BAR = {-1: (2e-5, max_rel), 1: (1e-4, rel_l2), 2: (2e-2, rel_l2)}
WGRAD_BAR = {-1: (3e-5, max_rel), 0: (3e-5, max_rel), 2: (2e-2, rel_l2)}


@pytest.fixture(scope="module")
def hip():
    from cruse_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def ref():
    return R.load()


def conv(hip, ref, tally, form, geom, prec, offs, accum, g):
    """one gather (form 'g': Cin, Fin, Cout, KT, S, pad, w_layout) or scatter2 ('s': Cs, Fg, Cout, KT, pad) call against its twin"""
    if form == "g":
        Cin, Fin, Cout, KT, S, pad, wl = geom
        Fout = (Fin + 2 * pad - 3) // S + 1
        w = rnd(g, *((Cin, Cout, 1, 3) if wl else (Cout, Cin, KT, 3)), scale=0.3)
        tail = lambda p: (B, T, Cin, Fin, Cout, Fout, KT, S, pad, wl, 0, accum, p, 0, 0)
        name = "cruse_conv_gather"
    else:
        Cin, Fin, Cout, KT, pad = geom
        Fout = 2 * Fin
        w = rnd(g, Cin, Cout, KT, 3, scale=0.3)
        tail = lambda p: (B, T, Cin, Fin, Cout, Fout, KT, pad, 0, accum, p, 0, 0)
        name = "cruse_conv_scatter2"
    x, bias, y0 = rnd(g, B, T, Cin, Fin), rnd(g, Cout), rnd(g, B, T, Cout, Fout)
    want = y0.copy()
    R.call(ref, name, x, w, None if accum else bias, want, *tail(prec), None)
    X, W, Bs, Y = place(x, offs["x"]), place(w), place(bias), place(y0, offs["out"])
    rc = getattr(hip, name)(X.ptr, W.ptr, None if accum else Bs.ptr, Y.ptr, *tail(prec), st())
    torch.cuda.synchronize()
    assert rc == 0, (name, geom, prec, offs, rc, hip.cruse_last_error())
    assert all(p.pads_ok() for p in (X, W, Bs, Y)), (name, geom, prec, offs)
    bar, measure = CONV_BAR[prec]
    tally.judge(f"{name[11:]} {geom} prec {prec} accum {accum}", offs, measure(Y.get(), want), bar)


def test_valu_conv_staging_of_a_misaligned_input(hip, ref):
    """conv.hip stage_rows: Fin % 4 == 0, x 1..3 floats off: the element-wise staging loop; forward and data-gradient forms"""
    g = np.random.default_rng(41)
    tally = Tally("VALU conv staging")
    for Cin, Fin, Cout in ((8, 16, 16), (1, 160, 8)):
        forms = [("g", (Cin, Fin, Cout, 2, 2, 1, 0)),       # the encoder conv
                 ("g", (Cin, Fin, Cout, 1, 1, 1, 1)),       # data gradient of the decoder's transposed conv (transposed weights)
                 ("s", (Cin, Fin, Cout, 1, 0)),             # the decoder's transposed conv
                 ("s", (Cin, Fin, Cout, 2, 1))]             # data gradient of the encoder conv
        for form, geom in forms:
            for k in (0, 1, 2, 3):
                for accum in (0, 1):
                    conv(hip, ref, tally, form, geom, -1, dict(x=k, out=0), accum, g)
    tally.done()


@pytest.mark.parametrize("prec", (1, 2))
def test_mfma_conv_eligibility_and_store_form(hip, ref, prec):
    """conv_mfma.hip: a misaligned x sends the call to the VALU kernel; with x aligned, an output 8 bytes off a 16-byte boundary takes the
    plain (4-byte store) form instead of the swapped-role one.  Level-2 and level-3 shapes of the model."""
    g = np.random.default_rng(50 + prec)
    tally = Tally(f"MFMA conv prec {prec}")
    forms = [("g", (16, 80, 32, 2, 2, 1, 0)), ("g", (32, 40, 64, 2, 2, 1, 0)), ("g", (32, 40, 32, 1, 1, 1, 1)), ("g", (16, 40, 16, 1, 1, 1, 0)),
             ("s", (32, 20, 16, 1, 0)), ("s", (64, 10, 32, 1, 0)), ("s", (32, 40, 16, 2, 1)), ("s", (64, 20, 32, 2, 1))]
    for form, geom in forms:
        for offs in (dict(x=0, out=0), dict(x=1, out=0), dict(x=2, out=0), dict(x=3, out=0), dict(x=0, out=2)):
            for accum in (0, 1):
                conv(hip, ref, tally, form, geom, prec, offs, accum, g)
    tally.done()


@pytest.mark.parametrize("prec", (-1, 0, 2))
def test_weight_gradient_routes_of_misaligned_operands(hip, ref, prec):
    """a and bt 4 and 8 bytes off: never the LDS-staged MFMA kernel (needs 16-byte alignment); the register-direct kernel of the bf16 mode
    keeps them (4-byte alignment suffices), the other modes take the VALU kernel.  The route is read from conv_wgrad_plan, then run."""
    from cruse_amd import ops
    g = np.random.default_rng(60 + prec)
    tally = Tally(f"cruse_conv_wgrad prec {prec}")
    routes = set()
    for (Bq, Tq, Ca, Fa, Cb, KT, S, pad) in RAGGED_SHAPES:
        Fb = S * Fa
        a, bt, dw0 = rnd(g, Bq, Tq, Ca, Fa), rnd(g, Bq, Tq, Cb, Fb), rnd(g, Ca, Cb, KT, 3)
        nws = max(hip.cruse_conv_wgrad_ws_bytes(Ca, Cb, KT), 16)
        aligned_kernel = None
        for ka, kb in ((0, 0), (1, 0), (0, 1), (2, 2), (1, 2)):
            offs = dict(a=ka, bt=kb)
            try:
                plan = ops.conv_wgrad_plan(Bq, Tq, Ca, Fa, Cb, Fb, KT, S, pad, prec=prec, a_misalign=4 * ka, bt_misalign=4 * kb)
            except RuntimeError:
                plan = None                                 # outside the VALU kernel's domain: the call itself must refuse and write nothing
            A, Bt, Dw = place(a, ka), place(bt, kb), place(dw0, sentinel=plan is None)
            ws = place(np.zeros(nws, np.uint8), sentinel=True)
            rc = hip.cruse_conv_wgrad(A.ptr, Bt.ptr, Dw.ptr, Bq, Tq, Ca, Fa, Cb, Fb, KT, S, pad, prec, 0, 0, ws.ptr, st())
            torch.cuda.synchronize()
            assert all(p.pads_ok() for p in (A, Bt, Dw, ws)), (Ca, Fa, Cb, KT, S, pad, offs)
            if plan is None:
                assert rc == -1 and Dw.untouched() and ws.untouched(), (rc, hip.cruse_last_error())
                continue
            assert rc == 0, (rc, hip.cruse_last_error())
            if ka or kb:
                assert plan["kernel"] != "mfma", (plan, offs)
                assert plan["kernel"] == ("rd" if prec == 2 and aligned_kernel == "rd" else "valu"), (plan, aligned_kernel, offs)
            else:
                aligned_kernel = plan["kernel"]
            routes.add((plan["kernel"], bool(ka or kb)))
            want = dw0.copy()
            R.call(ref, "cruse_conv_wgrad", a, bt, want, Bq, Tq, Ca, Fa, Cb, Fb, KT, S, pad, prec, 0, 0, None, None)
            bar, measure = WGRAD_BAR[prec]
            tally.judge(f"{(Bq, Tq, Ca, Fa, Cb, KT, S, pad)} {plan['kernel']}", offs, measure(Dw.get(), want), bar)
    print("routes run (kernel, misaligned):", sorted(routes))
    # misaligned operands ran the VALU kernel (exact and f32 modes) or, in the bf16 mode, the register-direct one, which every shape here takes
    assert {k for k, mis in routes if mis} == ({"rd"} if prec == 2 else {"valu"}), routes
    tally.done()


def test_weight_gradient_of_bf16_operands_two_bytes_off(hip):
    """bf16-stored a / bt one element (2 bytes) off: the register-direct kernel needs 4-byte alignment, the LDS-staged one 16, and the VALU
    kernel reads f32 only -- whatever conv_wgrad_plan answers, the call does the same: the planned kernel against float64, or a refusal
    that has written nothing"""
    from cruse_amd import ops
    g = np.random.default_rng(70)
    tally = Tally("cruse_conv_wgrad bf16 operands")
    for (Bq, Tq, Ca, Fa, Cb, KT, S, pad) in RAGGED_SHAPES[:4]:
        Fb = S * Fa
        a, bt, dw0 = bf16_bits(rnd(g, Bq, Tq, Ca, Fa)), bf16_bits(rnd(g, Bq, Tq, Cb, Fb)), rnd(g, Ca, Cb, KT, 3)
        nws = max(hip.cruse_conv_wgrad_ws_bytes(Ca, Cb, KT), 16)
        for ka, kb in ((0, 0), (1, 0), (0, 1)):
            try:
                plan = ops.conv_wgrad_plan(Bq, Tq, Ca, Fa, Cb, Fb, KT, S, pad, prec=2, a_dtype=2, bt_dtype=2, a_misalign=2 * ka, bt_misalign=2 * kb)
            except RuntimeError:
                plan = None
            assert plan is None or not (ka or kb), "a kernel that takes bf16 operands 2 bytes off: read its loads before this test runs it"
            assert plan is not None or ka or kb, "aligned bf16 operands must have a kernel: else nothing is compared"
            A, Bt, Dw = place(a, ka), place(bt, kb), place(dw0, sentinel=plan is None)
            ws = place(np.zeros(nws, np.uint8), sentinel=True)
            rc = hip.cruse_conv_wgrad(A.ptr, Bt.ptr, Dw.ptr, Bq, Tq, Ca, Fa, Cb, Fb, KT, S, pad, 2, 2, 2, ws.ptr, st())
            torch.cuda.synchronize()
            assert all(p.pads_ok() for p in (A, Bt, Dw, ws))
            if plan is None:
                assert rc != 0 and hip.cruse_last_error() and Dw.untouched() and ws.untouched(), (rc, ka, kb)
                tally.n["offset" if ka or kb else "aligned"] += 1
                continue
            assert rc == 0, (rc, hip.cruse_last_error())
            a64, b64 = bf16_value(a), bf16_value(bt)
            want = dw0.astype(np.float64)
            for kt in range(KT):
                for kf in range(3):
                    fb = np.arange(Fa) * S - pad + kf
                    ok = (fb >= 0) & (fb < Fb)
                    src = np.zeros((Bq, Tq, Cb, Fa))
                    sh = KT - 1 - kt
                    src[:, sh:, :, ok] = b64[:, :Tq - sh][..., fb[ok]]
                    want[:, :, kt, kf] += np.einsum("btaf,btcf->ac", a64, src)
            tally.judge(f"{(Bq, Tq, Ca, Fa, Cb, KT, S, pad)} {plan['kernel']}", dict(a=ka, bt=kb), rel_l2(Dw.get(), want), 2e-2)
    tally.done()
