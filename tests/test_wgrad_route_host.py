"""CPU: what cruse_conv_wgrad launches for a call (cruse_conv_wgrad_plan / ops.conv_wgrad_plan) -- which of the three kernels, its template
integers, grid, block, LDS bytes, slabs and the reduce that follows, or the error the entry point answers with.  A host-side decision: the
library loads without a GPU.

The expected results (tests/golden/wgrad_plan_parent.json) were recorded from the library as it was BEFORE the weight-gradient host path
was gathered onto one call descriptor, never from the code under test.  A build of the parent commit got a scratch patch, kept out of the
repository: each of the three host paths (cruse_wgrad_rd_try, cruse_wgrad_mfma_try, the VALU path inside cruse_conv_wgrad) wrote the
fourteen figures of cruse_conv_wgrad_plan into a caller-supplied array right before its launch and returned instead of launching, the
entry point added the grid of the reduce it was about to launch, and the workspace size it hands the register-direct path (always
cruse_conv_wgrad_ws_bytes in the parent) was made settable.  That build's own cruse_conv_wgrad was then called with stand-in pointers of
the given misalignment over cases() below, and its return code, cruse_last_error() and the array were written down.  The file pins that
refactor, and every later one, to the same choices and messages.  Its layout: "results", the distinct outcomes (the fourteen figures, or
[code, message] of a refusal); "per_bt", the distinct quadruples of them over the four (B, T) of BT; "index", one entry into "per_bt" per
case of cases(), in that order."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan_parent.json")
BT = ((1, 1), (2, 7), (3, 21), (64, 401))
F32, F16, BF16 = 0, 1, 2                  # CRUSE_DT_*
VALU, MFMA, RD = 0, 1, 2                  # out[0]

# (Ca, Fa, Cb, Fb, KT, S, pad)
CH, FR = (1, 8, 16, 32, 64), (160, 80, 40, 20, 10)
ENCODER = [(CH[k], FR[k], CH[k - 1], FR[k - 1], 2, 2, 1) for k in range(1, 5)]
SKIPS = [(CH[k], FR[k], CH[k], FR[k], 1, 1, 1) for k in range(1, 5)]
DECODER = [(CH[k], FR[k], CH[k - 1], FR[k - 1], 1, 2, 0) for k in range(1, 5)]
UPSAMPLE = [g for k in range(1, 5) for g in ((CH[k], FR[k - 1], CH[k - 1], FR[k - 1], 1, 1, 1), (CH[k - 1], FR[k - 1], CH[k], FR[k - 1], 1, 1, 1))]
# the shapes of tests/test_gpu_kernels.py::test_conv_wgrad_register_direct_kernel, as (B, T, Ca, Fa, Cb, KT, S, pad)
RAGGED_SHAPES = [(2, 5, 8, 8, 1, 2, 2, 1), (3, 1, 16, 12, 8, 2, 2, 1), (1, 2, 32, 20, 16, 2, 2, 1), (2, 7, 64, 10, 32, 2, 2, 1), (2, 9, 24, 10, 12, 2, 2, 1),
                 (2, 5, 8, 40, 1, 1, 2, 0), (3, 3, 16, 12, 8, 1, 2, 0), (2, 4, 64, 10, 32, 1, 2, 0), (1, 6, 40, 20, 24, 1, 2, 0),
                 (2, 5, 8, 16, 8, 1, 1, 1), (3, 3, 32, 20, 32, 1, 1, 1), (2, 4, 64, 10, 64, 1, 1, 1), (1, 11, 12, 12, 40, 1, 1, 1),
                 (5, 21, 16, 40, 8, 2, 2, 1)]
RAGGED = [(Ca, Fa, Cb, S * Fa, KT, S, pad) for _, _, Ca, Fa, Cb, KT, S, pad in RAGGED_SHAPES]
EDGES = [(16, 9, 8, 18, 2, 2, 1), (16, 1, 8, 2, 2, 2, 1),            # Fa odd: neither MFMA kernel
         (40, 9, 24, 18, 2, 2, 1),                                   # ... and 60 output tiles do not divide the VALU block
         (16, 6, 8, 12, 2, 2, 1),                                    # Fa = 6: below the register-direct minimum of 8
         (128, 10, 8, 20, 2, 2, 1), (128, 10, 64, 20, 2, 2, 1),      # Ca = 128: VALU; with Cb = 64, 512 output tiles > 256 threads
         (16, 20, 64, 40, 2, 2, 1),                                  # ntw = 6 > 3 (and 8 source windows > 4)
         (16, 20, 8, 42, 2, 2, 1), (16, 20, 8, 20, 1, 2, 0),         # Fb != S * Fa
         (8, 8, 1, 8, 1, 1, 1)]                                      # (B, T) = (1, 1): bt has 8 < 16 elements
GEOMS = list(dict.fromkeys(ENCODER + SKIPS + DECODER + UPSAMPLE + RAGGED + EDGES))
SUBSET = [ENCODER[1], ENCODER[3], SKIPS[1], DECODER[2], UPSAMPLE[2], RAGGED[0], RAGGED[4], RAGGED[8], RAGGED[12], EDGES[3], EDGES[9]]

PRECS = (-1, 0, 1, 2)                     # VALU, CRUSE_PREC_F32, _BF16X3, _BF16
DTYPES = ((F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32))
MISALIGN = ((4, 0), (0, 4), (2, 0))
OPTIONS = (None, ("wg_rd", 0), ("wg_grid", 8), ("wg_grid", 100))
WS_SLABS = (1, 16)                        # ws_bytes as a number of [Ca][Cb][KT][3] slabs (cruse_conv_wgrad_ws_bytes holds 1024); 0 = the default

# refusals: (geometry, prec, dtypes) beyond those the matrix meets on its own
ERRORS = [((0, 20, 8, 40, 2, 2, 1), 2, (F32, F32)), ((16, 20, 0, 40, 2, 2, 1), -1, (F32, F32)),          # empty shape
          ((16, 20, 8, 40, 2, 2, 1), 2, (F16, F32)), ((16, 20, 8, 40, 2, 2, 1), -1, (F32, 3)),          # bad dtype code
          ((16, 20, 8, 40, 3, 2, 1), 2, (F32, F32)), ((16, 20, 8, 60, 2, 3, 1), 0, (F32, F32)), ((16, 20, 8, 40, 2, 2, 2), -1, (F32, F32)),
          ((16, 20, 8, 40, 2, 2, 1), -1, (BF16, BF16)), ((16, 9, 8, 18, 2, 2, 1), 2, (BF16, F32)),      # bf16 operands reaching the VALU path
          ((6, 20, 8, 40, 2, 2, 1), -1, (F32, F32)), ((6, 9, 8, 18, 2, 2, 1), 2, (F32, F32)),           # Ca % 4 != 0
          ((16, 20, 6, 40, 2, 2, 1), -1, (F32, F32)), ((16, 9, 6, 18, 2, 2, 1), 1, (F32, F32)),         # Cb = 6
          ((40, 20, 24, 40, 1, 2, 0), -1, (F32, F32)), ((128, 10, 64, 20, 2, 2, 1), -1, (F32, F32)),    # 60 / 512 output tiles
          ((64, 160, 64, 160, 1, 1, 1), -1, (F32, F32))]                                                # VALU LDS over 160 KB


def cases():
    """(option, geometry, precision, dtypes, misalignment, ws slabs) in the order of the recorded file; each stands for the four (B, T) of BT"""
    for geom in GEOMS:
        for prec in PRECS:
            for dt in DTYPES:
                yield None, geom, prec, dt, (0, 0), 0
    for geom in SUBSET:
        for prec in PRECS:
            for dt in DTYPES[:2]:
                for mis in MISALIGN:
                    yield None, geom, prec, dt, mis, 0
    for opt in OPTIONS[1:]:
        for geom in GEOMS:
            for prec in (0, 2):
                for dt in (DTYPES if opt[0] == "wg_rd" else DTYPES[:2]):
                    yield opt, geom, prec, dt, (0, 0), 0
    for opt in (None, ("wg_grid", 100)):
        for geom in SUBSET:
            for prec in (0, 2):
                for dt in DTYPES[:2]:
                    for slabs in WS_SLABS:
                        yield opt, geom, prec, dt, (0, 0), slabs
    for geom, prec, dt in ERRORS:
        yield None, geom, prec, dt, (0, 0), 0


def key(case):
    return json.dumps(case, separators=(",", ":"))


def ws_bytes_of(geom, slabs):
    """`slabs` [Ca][Cb][KT][3] f32 slabs with the channels rounded up to 16: 1 / 1024 of cruse_conv_wgrad_ws_bytes each"""
    Ca, _, Cb, _, KT, _, _ = geom
    return slabs * ((Ca + 15) // 16 * 16) * ((Cb + 15) // 16 * 16) * KT * 3 * 4


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


def _plan(ops, geom, prec, dt, mis, slabs, B, T):
    """the recorded form of a result: the fourteen figures, or [code, message] of the refusal"""
    Ca, Fa, Cb, Fb, KT, S, pad = geom
    try:
        return ops.conv_wgrad_plan(B, T, Ca, Fa, Cb, Fb, KT, S, pad, prec, a_dtype=dt[0], bt_dtype=dt[1], a_misalign=mis[0], bt_misalign=mis[1],
                                   ws_bytes=ws_bytes_of(geom, slabs))["raw"]
    except RuntimeError as e:
        head, _, msg = str(e).partition(": ")
        return [int(head.rsplit(" ", 1)[1]), msg]


def test_the_recorded_file_covers_the_matrix(ops, golden):
    def row(geom, prec, dt=(F32, F32), opt=None, mis=(0, 0), slabs=0):
        return golden[key((opt, geom, prec, dt, mis, slabs))]
    # every kernel at every prec that can reach it
    reached = {(r[0], c[2]) for c in cases() for r in golden[key(c)] if len(r) == 14}
    assert reached == {(VALU, -1), (VALU, 0), (VALU, 1), (VALU, 2), (MFMA, 0), (MFMA, 1), (MFMA, 2), (RD, 2)}
    # the corners the issue names are in the file with the outcome it names
    bf = (BF16, BF16)
    assert [r[0] for r in row(ENCODER[1], 2, bf)] == [RD] * 4 and [r[0] for r in row(ENCODER[1], 2, bf, ("wg_rd", 0))] == [MFMA] * 4
    assert [r[0] for r in row(EDGES[9], 2, bf)] == [MFMA, RD, RD, RD]                      # (1, 1): bt has fewer than 16 elements
    assert [r[0] for r in row(EDGES[3], 2)] == [MFMA] * 4                                  # Fa = 6
    assert all(r[0] == VALU for g in (EDGES[0], EDGES[1], EDGES[4], EDGES[6]) for p in PRECS for r in row(g, p))
    assert all(r[0] != RD for g in (EDGES[7], EDGES[8]) for r in row(g, 2))                # Fb != S * Fa
    assert all(r[0] != RD for m in ((2, 0),) for r in row(ENCODER[1], 2, bf, mis=m))       # 2-byte aligned: not register-direct ...
    assert all(r[0] == RD for m in ((4, 0), (0, 4)) for r in row(ENCODER[1], 2, bf, mis=m))    # ... 4-byte aligned: not LDS-staged
    # the register-direct grid: the nframes / 4 clamp at (3, 21), gcap 256 / TG and whole rounds of 8 XCDs at (64, 401), wg_grid, the ns clamp
    r = row(ENCODER[1], 2, bf)
    assert (r[2][8], r[2][10], r[2][5]) == (13, 5, 16)          # 63 frames: at most 63 / 4 = 15 slabs -> 5 frames each -> 13 slabs, 2 rounds of XCDs
    assert (r[3][8], r[3][9], r[3][10], r[3][5]) == (255, 1, 101, 256)      # 25664 frames over 256 slabs: 101 frames each -> 255 slabs
    assert row(ENCODER[1], 2, bf, ("wg_grid", 100))[3][8] == 100 and row(ENCODER[1], 2, bf, ("wg_grid", 8))[3][8] == 8
    assert row(ENCODER[1], 2, bf, slabs=16)[3][8] == 16 and row(ENCODER[1], 2, bf, slabs=1)[3][8] == 1       # slabs clamped to the workspace
    # Ca = 40, Cb = 24: a register-direct slab is 2 workgroups x 4 row tiles of 16 x 16 x 3 = 24576 B, a [48][32][3] slab 18432 B: one does not fit
    assert [r[0] for r in row(RAGGED[8], 2, bf, slabs=1)] == [MFMA] * 4 and [r[0] for r in row(RAGGED[8], 2, bf, slabs=16)] == [RD] * 4
    assert row(ENCODER[1], 0)[3][5] == 512 and row(ENCODER[3], 0)[3][5] == 256             # the LDS-staged kernel's gcap
    assert all(len(r) == 2 and r[0] < 0 for g, p, dt in ERRORS for r in row(g, p, dt))
    assert len({r[1] for g, p, dt in ERRORS for r in row(g, p, dt)}) >= 11                 # each refusal the issue names has its own message


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "defaults" if o is None else "%s=%d" % o)
def test_conv_wgrad_plan_is_what_the_parent_launched(ops, golden, opt):
    with (ops.options(**{opt[0]: opt[1]}) if opt else ops.options()):
        for case in cases():
            if case[0] != opt:
                continue
            _, geom, prec, dt, mis, slabs = case
            got = [_plan(ops, geom, prec, dt, mis, slabs, B, T) for B, T in BT]
            assert got == golden[key(case)], (case, got, golden[key(case)])
    assert opt is None or ops.get_option(opt[0]) is None


def test_default_workspace_is_what_ops_passes(ops):
    """ws_bytes = 0 stands for cruse_conv_wgrad_ws_bytes, the size ops.conv_wgrad allocates"""
    from cruse_amd._lib import lib
    for geom in SUBSET:
        Ca, Fa, Cb, Fb, KT, S, pad = geom
        assert lib.cruse_conv_wgrad_ws_bytes(Ca, Cb, KT) == ws_bytes_of(geom, 1024)
        for dt in DTYPES[:2]:
            assert (ops.conv_wgrad_plan(64, 401, *geom, 2, *dt) == ops.conv_wgrad_plan(64, 401, *geom, 2, *dt, ws_bytes=ws_bytes_of(geom, 1024)))
