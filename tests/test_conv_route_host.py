"""CPU: what the frame-major convolutions launch for a call (cruse_conv_plan / ops.conv_plan) -- route, tile, grid and LDS bytes, or the
error the entry point answers with.  A host-side decision: the library loads without a GPU.

The expected results (tests/golden/conv_plan_parent.json) were recorded from the library as it was BEFORE the ten entry points were
gathered onto one call descriptor, never from the code under test.  A build of the parent commit got a scratch patch, kept out of the
repository: the MFMA dispatcher and the two VALU host paths wrote (route, fused, mt, nw, grid, LDS bytes, CO_T) into a caller-supplied
array right before their launch and returned instead of launching, the separate BatchNorm-backward pass of the _bnbwd_in fallback was
skipped, and "cm_grid" -- an option the dispatcher read but the option table did not list -- was made settable.  That build's own entry
points (cruse_conv_gather ... cruse_conv_scatter2_bnbwd_in) were then called with 16-byte aligned stand-in pointers over cases() below, and
their return code, cruse_last_error() and the array were written down.  The file pins that refactor, and every later one, to the same
choices and messages.  Its layout: "results", the distinct outcomes (the seven figures, or [code, message] of a refusal); "per_bt", the
distinct triples of them over the three (B, T) of BT; "index", one entry into "per_bt" per case of cases(), in that order."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_parent.json")
BT = ((1, 1), (2, 7), (64, 401))          # tiles: 1, 2, 3264 -- under and at the grid cap (512 / 1024, or cm_grid)
F32, BF16 = 0, 2                          # CRUSE_DT_*
SUMS, BNB, BNI, BBI = 1, 2, 4, 8          # CRUSE_CONV_FORM_*

# (scatter, Cin, Fin, Cout, Fout, KT, S, pad, w_layout)
CH, FR = (1, 8, 16, 32, 64), (160, 80, 40, 20, 10)
ENCODER = [(0, CH[i], FR[i], CH[i + 1], FR[i + 1], 2, 2, 1, 0) for i in range(4)]                  # level 1: Cin = 1 -> VALU
DECODER = [(1, CH[i + 1], FR[i + 1], CH[i], FR[i], 2, 2, 1, 0) for i in reversed(range(4))]        # level 1: Cout = 1 -> VALU
SKIPS = [(0, CH[i], FR[i], CH[i], FR[i], 1, 1, 1, wl) for i in range(1, 5) for wl in (0, 1)]
VALU_ONLY = [(0, 3, 40, 32, 20, 2, 2, 1, 0), (0, 24, 40, 32, 20, 2, 2, 1, 0), (0, 16, 40, 6, 20, 2, 2, 1, 0), (0, 16, 40, 128, 20, 2, 2, 1, 0),
             (0, 16, 41, 32, 20, 2, 2, 1, 0),                                                      # odd Fin: VALU in the bf16 modes
             (1, 3, 20, 16, 40, 2, 2, 1, 0), (1, 24, 20, 16, 40, 2, 2, 1, 0), (1, 16, 20, 6, 40, 2, 2, 1, 0), (1, 16, 20, 128, 40, 2, 2, 1, 0),
             (1, 16, 21, 16, 42, 2, 2, 1, 0)]
FIVE_WAVE = [(0, 32, 20, 32, 10, 2, 2, 1, 0)]      # 5 N-tiles, mt = 2: the fused BatchNorm-backward input is refused for the waves alone
GEOMS = ENCODER + DECODER + SKIPS + VALU_ONLY + FIVE_WAVE

# (forms, x_dtype -- dout_dtype with BBI --, y_dtype, act, accum): what the parent's entry points can express
VARIANTS = [(0, F32, F32, 0, 0), (0, F32, F32, 1, 0), (0, F32, F32, 0, 1), (0, BF16, F32, 0, 0), (0, BF16, BF16, 0, 1),
            (SUMS, F32, F32, 0, 0),
            (SUMS | BNB, F32, F32, 0, 0), (SUMS | BNB, BF16, F32, 0, 0), (SUMS | BNB, BF16, BF16, 0, 1),
            (BNI, F32, F32, 0, 0), (BNI | SUMS, F32, F32, 0, 0),
            (BBI, BF16, F32, 0, 0), (BBI, BF16, BF16, 0, 1), (BBI, F32, F32, 0, 0),
            (BBI | BNB, BF16, F32, 0, 0), (BBI | BNB, BF16, BF16, 0, 1), (BBI | BNB, F32, F32, 0, 0)]
OPTION_VARIANTS = [VARIANTS[0], VARIANTS[8], VARIANTS[11]]
OPTIONS = (None, ("cm_nw", 4), ("cm_nw", 5), ("cm_grid", 100))
PRECS = (0, 1, 2)                         # CRUSE_PREC_F32, _BF16X3, _BF16

# the refusals the issue names, beyond those the matrix meets on its own (bni on a shape the MFMA kernel refuses, bf16 input on the VALU route)
ERRORS = [((0, 16, 40, 32, 20, 2, 2, 1, 0), 1, (0, F32, F32, 1, 1)),          # accum with act
          ((1, 32, 20, 16, 40, 2, 2, 1, 0), 1, (0, F32, F32, 1, 1)),
          ((0, 16, 40, 16, 40, 2, 1, 1, 1), 1, (0, F32, F32, 0, 0)),          # w_layout = 1 with KT = 2
          ((0, 16, 40, 32, 21, 2, 2, 1, 0), 1, (0, F32, F32, 0, 0)),          # Fout reads past Fin
          ((1, 32, 20, 16, 41, 2, 2, 1, 0), 1, (0, F32, F32, 0, 0)),          # scatter2 with Fout != 2 * Fg
          ((0, 3, 40, 32, 20, 2, 2, 1, 0), 1, (BNI, F32, F32, 0, 0)),         # bni on a shape the MFMA kernel refuses
          ((1, 3, 20, 16, 40, 2, 2, 1, 0), 1, (BNI, F32, F32, 0, 0)),
          ((0, 3, 40, 32, 20, 2, 2, 1, 0), 2, (0, BF16, F32, 0, 0)),          # a bf16 input on the VALU route
          ((1, 3, 20, 16, 40, 2, 2, 1, 0), 2, (0, BF16, F32, 0, 0))]


def cases():
    """(option, geometry, precision, variant) in the order of the recorded file; each stands for the three (B, T) of BT"""
    for opt in OPTIONS:
        for geom in GEOMS:
            for prec in PRECS:
                for var in (VARIANTS if opt is None else OPTION_VARIANTS):
                    if geom[8] and var[0] in (SUMS, BNI, BNI | SUMS):
                        continue                      # (the _bnstats / _bnin entry points have no w_layout)
                    yield opt, geom, prec, var
    for geom, prec, var in ERRORS:
        yield None, geom, prec, var


def key(case):
    return json.dumps(case, separators=(",", ":"))


@pytest.fixture(scope="module")
def ops():
    from cruse_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        d = json.load(f)
    assert len(d["index"]) == sum(1 for _ in cases()) and all(len(t) == len(BT) for t in d["per_bt"])
    return {key(c): [d["results"][j] for j in d["per_bt"][i]] for c, i in zip(cases(), d["index"])}


def _plan(ops, geom, prec, var, B, T):
    """the recorded form of a result: the seven figures, or [code, message] of the refusal"""
    forms, xdt, ydt, act, accum = var
    try:
        d = ops.conv_plan(*geom, B, T, prec, x_dtype=xdt, y_dtype=ydt, act=act, accum=accum, forms=forms)
    except RuntimeError as e:
        head, _, msg = str(e).partition(": ")
        return [int(head.rsplit(" ", 1)[1]), msg]
    return [1 if d["route"] == "mfma" else 0, int(d["fused"]), d["mt"], d["nw"], d["grid"], d["lds_bytes"], d["co_t"]]


def test_the_recorded_file_covers_the_matrix(golden):
    def row(geom, prec, var, opt=None):
        return golden[key((opt, geom, prec, var))]
    # the corners the issue names are in the file with the outcome it names
    assert all(r[0] == 0 for r in row(ENCODER[0], 1, VARIANTS[0]))                         # Cin = 1: VALU
    assert all(r[0] == 1 for r in row(ENCODER[2], 1, VARIANTS[0]))                         # level 3: MFMA
    assert all(r[0] == 0 for g in VALU_ONLY[:4] + VALU_ONLY[5:9] for p in PRECS for r in row(g, p, VARIANTS[0]))
    assert all(r[0] == 1 for r in row(VALU_ONLY[4], 0, VARIANTS[0])) and all(r[0] == 0 for p in (1, 2) for r in row(VALU_ONLY[4], p, VARIANTS[0]))
    assert all(r[:2] == [1, 1] for r in row(ENCODER[2], 2, VARIANTS[11]))                  # bbi: the fused kernel ...
    assert all(r[:4] == [1, 0, 4, 5] for r in row(ENCODER[3], 2, VARIANTS[11]))            # ... not at Cout = 64 (mt = 4) ...
    assert all(r[:4] == [1, 0, 2, 5] for r in row(FIVE_WAVE[0], 2, VARIANTS[11]))          # ... nor on a 5-wave shape
    assert row(ENCODER[1], 1, VARIANTS[0])[2][4] == 1024 and row(ENCODER[1], 1, VARIANTS[0], ("cm_grid", 100))[2][4] == 100
    assert all(len(r) == 2 for g, p, v in ERRORS for r in row(g, p, v))


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "defaults" if o is None else "%s=%d" % o)
def test_conv_plan_is_what_the_parent_launched(ops, golden, opt):
    with (ops.options(**{opt[0]: opt[1]}) if opt else ops.options()):
        for case in cases():
            if case[0] != opt:
                continue
            _, geom, prec, var = case
            got = [_plan(ops, geom, prec, var, B, T) for B, T in BT]
            assert got == golden[key(case)], (case, got, golden[key(case)])
    assert opt is None or ops.get_option(opt[0]) is None
