"""CPU: what the bf16 / f16 gate GEMMs launch for a call (cruse_gemm_bf16_plan / ops.gemm_bf16_plan) -- kernel variant, grid, LDS bytes and tile
geometry, or the error the entry point answers with.  A host-side decision: the library loads without a GPU.

The expected results (tests/golden/gemm_bf16_plan_parent.json) were recorded from the library as it was BEFORE the ten entry points were gathered
onto one call descriptor, never from the code under test.  A build of the parent commit got a scratch patch, kept out of the repository:
gemm_bf16_impl wrote the 16 figures (MODE, NST, F16, ATR of the kernel it was about to launch, grid, LDS bytes, k-slices, k-tiles per slice,
xcdk, tiles_m, tiles_n, nunits, inner, output rows, slab stride, blocks of the slab sum) into a caller-supplied array right before each of its
launch sites, ahead of cruse_ensure_dyn_lds, and returned instead of launching.  That build's own ten entry points (cruse_gemm_bf16_nt ...
cruse_gemm_bf16x3_nt) were then called with 16-byte aligned stand-in pointers over cases() below, and their return code, cruse_last_error() and
the array were written down.  The six refusals marked "impl" in ERRORS ask for something no entry point has an argument for (an f16 call that
accumulates, a slab call with a bias ...): for those the parent's gemm_bf16_impl was called directly, with the arguments the form's entry point
passes and the one scalar changed.  DIRECT holds the refusals only a pointer can trigger; they were recorded through the parent's entry points
and are asked of the real entry points here.  The file pins that refactor, and every later one, to the same choices and messages.  Its layout:
"results", the distinct outcomes (the 16 figures, or [code, message] of a refusal); "index", one entry into "results" per case of cases(), in
that order; "direct", [code, message] per entry of DIRECT."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bf16_plan_parent.json")
F32, F16, BF16 = 0, 1, 2                  # CRUSE_DT_*
A_LO, B_LO, UNALIGNED = 1, 2, 4           # ops.GEMM_PLANE_*
SHAPES = ((1, 1, 64),                     # one ragged tile
          (129, 127, 128),                # two tiles each way, ragged
          (200, 96, 4096),                # kt_chunk = 64 at split-K 1: deep
          (200, 96, 4032),                # ... and 63: not
          (64, 1920, 640), (1920, 640, 25664), (25664, 640, 1920))      # the bench's gi, dW and dX
SPLITK = (1, 0, 3, 6, -3, -8, 1000)       # (1000: clamped to the k-tile count)
LAYOUTS = ("rows", "ktiled")
VARIANTS = {(m, n, False, False) for m in range(5) for n in (2, 3)} | {(0, 2, False, True), (1, 2, False, True), (0, 2, True, False), (3, 2, True, False)}


def case(form, M, N, K, layout="rows", lda=None, a_ks=None, ldb=None, b_ks=None, ldc=None, planes=0, bias=0, acc=0, splitk=1, f16=0, dt=F32, extras=()):
    """(form, M, N, K, lda, a_kstride, ldb, b_kstride, ldc, planes, bias, accumulate, splitk, operands_f16, out_dtype, extras): the arguments of
    ops.gemm_bf16_plan.  layout "rows": row-major operands; "ktiled": lda = 64 and a k-tile stride of 64 * (rows of the operand)"""
    kt = layout == "ktiled"
    d = ((64 if kt else K) if lda is None else lda, (64 * max(M, 2) if kt else 64) if a_ks is None else a_ks,
         (64 if kt else K) if ldb is None else ldb, (64 * max(N, 2) if kt else 64) if b_ks is None else b_ks, N if ldc is None else ldc)
    return (form, M, N, K) + d + (planes, bias, acc, splitk, f16, dt, tuple(extras))


def slab_bytes(rows, N, K, splitk):
    """bytes of the slabs a split-K call stores: the k-slices after the library's clamping, rows x N floats each"""
    nkt = K // 64
    z = min(max(abs(splitk) if splitk < -1 else splitk, 1), nkt)
    z = -(-nkt // -(-nkt // z))
    return z * rows * N * 4


def cat_extras(Ms, a_rows, nprob, scratch):
    return (scratch, nprob) + tuple(Ms) + tuple(a_rows)


# slabs_cat: (Ms, N, K, a_kstride): the three weight-gradient products of a GRU layer at Hg = 128, 160, 640, and products that end inside a tile
CATS = [((3 * h, 2 * h, h), h, 25664, 4 * h * 64) for h in (128, 160, 640)] + [((70, 200, 33), 96, 4096, 64 * 400)]

# one refusal per CRUSE_REQUIRE of the GEMM host path, beyond those the matrix meets on its own (split-K without accumulate, a scratch one byte
# short).  "impl": no entry point has the argument (see the docstring)
ERRORS = [
    case("plain", 128, 128, 100),                                                  # K % 64 != 0
    case("plain", 0, 128, 64),                                                     # empty shape
    case("plain", 128, 128, 64, ldc=127),                                          # ldc < N: strides too small
    case("plain", 128, 128, 128, lda=132),                                         # a stride that is no multiple of 8
    case("plain", 128, 128, 128, lda=64),                                          # lda too small for the row-major layout
    case("plain", 128, 128, 128, "ktiled", lda=56),                                # ... and for the K-tiled one
    case("plain", 1 << 30, 257 * 128, 64),                                         # a grid of 2^31 blocks and more
    case("plain", 128, 128, 256, splitk=2),                                        # split-K > 1 without accumulate
    case("x3", 128, 128, 64, planes=A_LO),                                         # A_lo without B_lo
    case("x3", 128, 128, 64),                                                      # no low plane at all
    case("x3", 128, 128, 64, planes=A_LO | B_LO | UNALIGNED),                      # unaligned low planes
    case("f16x2", 128, 128, 64),                                                   # B_lo is required
    case("f16", 128, 128, 64, acc=1),                                              # impl: f16 with accumulate
    case("f16", 128, 128, 256, acc=1, splitk=2),                                   # impl: f16 with split-K
    case("out16", 128, 128, 64, dt=F32), case("out16", 128, 128, 64, dt=7),        # a bad out_dtype
    case("out16", 128, 128, 64, planes=A_LO, dt=F16),                              # A_lo without B_lo
    case("out16", 128, 128, 64, planes=A_LO | B_LO, f16=1, dt=F16),                # A_lo with f16 operands
    case("out16", 128, 128, 64, planes=B_LO | UNALIGNED, dt=BF16),                 # an unaligned low plane
    case("out16", 128, 128, 64, acc=1, dt=BF16),                                   # impl: a 16-bit result with accumulate
    case("atr", 130, 128, 128, extras=(128 * 64 - 8, 3)),                          # a short a_mb_stride
    case("atr", 130, 128, 128, extras=(128 * 64, 2)),                              # too few 64-row blocks
    case("atr", 130, 128, 128, planes=B_LO, extras=(128 * 64, 3)),                 # impl: ATR with a low plane
    case("groups", 128, 96, 64, lda=192, ldc=3 * 96, extras=(3, 64, 96 * 64, 100, 96)),            # (G - 1) * c_gstep + N > ldc
    case("groups", 128, 96, 64, lda=192, ldc=3 * 96, extras=(0, 64, 96 * 64, 96, 96)),             # G = 0
    case("groups", 128, 96, 64, lda=192, ldc=3 * 96, planes=A_LO, extras=(3, 64, 96 * 64, 96, 96)),  # A_lo without B_lo
    case("groups", 128, 96, 256, lda=768, ldc=3 * 96, acc=1, splitk=2, extras=(3, 256, 96 * 256, 96, 96)),   # impl: groups with split-K
    case("slabs", 129, 127, 128, splitk=2, extras=(1 << 20,)),                     # slab form with N % 4 != 0
    case("slabs", 128, 128, 128, bias=1, splitk=2, extras=(1 << 20,)),             # impl: slab form with a bias
    case("slabs_cat", 0, 96, 4096, "ktiled", a_ks=64 * 400, extras=cat_extras((70, 200, 33), (0, 0, 210), 0, 1 << 24)),     # nprob 0
    case("slabs_cat", 0, 96, 4096, "ktiled", a_ks=64 * 400, extras=cat_extras((70, 200, 33), (0, 0, 210), 4, 1 << 24)),     # nprob 4
    case("slabs_cat", 0, 96, 4096, "ktiled", a_ks=64 * 400, extras=cat_extras((70, 0, 33), (0, 0, 210), 3, 1 << 24)),       # an empty product
    case("slabs_cat", 0, 96, 4096, extras=cat_extras((70, 200, 33), (0, 0, 210), 3, 1 << 24)),                              # row-major A
    case("seg", 15, 96, 128, extras=(0, 17, 7)),                                   # seg_len = 0
    case("seg", 16, 96, 128, extras=(5, 17, 7)),                                   # M % seg_len != 0
    case("seg", 15, 96, 128, extras=(5, 4, 7)),                                    # seg_stride < seg_len
    case("seg", 15, 96, 128, planes=A_LO, extras=(5, 17, 7)),                      # A_lo without B_lo
]

# every CRUSE_REQUIRE of the GEMM host path, by a piece of its message
REFUSALS = ("gemm_bf16_nt_groups: row-major A", "gemm_bf16_nt_atr: plain bf16", "gemm_f16_nt: f32 result stored", "a bf16 result is stored",
            "bad row segments", "empty shape", "must be a multiple of 64", "strides too small", "too small for the operand layout",
            "16-byte aligned rows and k-tiles", "slab form needs N", "do not fit", "slab form has no bias", "grid too large", "split-K adds into C",
            "gemm_f16x2_nt: B_lo is required", "gemm_nt_out16: out_dtype", "gemm_nt_out16: low planes", "gemm_bf16_nt_atr: a_mb_stride",
            "gemm_bf16_nt_groups: G=", "gemm_bf16_nt_groups: low planes", "gemm_bf16_nt_slabs: scratch is NULL", "gemm_bf16_nt_slabs_cat: 1..3 products",
            "gemm_bf16_nt_slabs_cat: product", "gemm_bf16_nt_slabs_cat: K-tiled A", "gemm_bf16_nt_seg: seg_len", "gemm_bf16_nt_seg: low planes",
            "gemm_bf16x3_nt: B_lo missing", "gemm_bf16x3_nt: unaligned low planes")

# refusals only a pointer triggers, through the real entry points: refused before any launch, so they run wherever the library loads
DIRECT = ("slabs: scratch is NULL", "slabs_cat: Bs[1] is NULL", "x3: A_lo is A_hi")


def cases():
    """the calls of the recorded file, in its order: every shape, split-K, plane set, result dtype and operand layout with each form that accepts it"""
    for M, N, K in SHAPES:
        for lay in LAYOUTS:
            for z in SPLITK:
                for acc in (0, 1):
                    yield case("plain", M, N, K, lay, bias=int(z == 1), acc=acc, splitk=z)
                for short in (0, 1):
                    yield case("slabs", M, N, K, lay, splitk=z, extras=(slab_bytes(M, N, K, z) - short,))
            for planes in (B_LO, A_LO | B_LO):
                for acc in (0, 1):
                    yield case("x3", M, N, K, lay, planes=planes, bias=1 - acc, acc=acc)
            yield case("f16", M, N, K, lay, bias=1)
            yield case("f16x2", M, N, K, lay, planes=B_LO)
            for dt in (F16, BF16):
                for f16, planes in ((0, 0), (0, B_LO), (0, A_LO | B_LO), (1, 0), (1, B_LO)):
                    yield case("out16", M, N, K, lay, planes=planes, bias=1, f16=f16, dt=dt)
            for acc in (0, 1):
                for more in (0, 1):                    # n_mb exact and one larger
                    yield case("atr", M, N, K, lay, acc=acc, extras=(4 * K * 64, (M + 63) // 64 + more))
        for G in (1, 3, 4):
            for cg in (N, N + 8):
                for planes in (0, B_LO, A_LO | B_LO):
                    for acc in (0, 1):
                        yield case("groups", M, N, K, lda=G * K, ldc=(G - 1) * cg + N, planes=planes, bias=1 - acc, acc=acc,
                                   extras=(G, K, N * K, cg, N))
    for Ms, N, K, a_ks in CATS:
        for nprob in (1, 2, 3):
            rows = sum(Ms[:nprob])
            for z in SPLITK:
                for short in (0, 1):
                    yield case("slabs_cat", 0, N, K, "ktiled", a_ks=a_ks, splitk=z,
                               extras=cat_extras(Ms, (0, 0, Ms[0]), nprob, slab_bytes(rows, N, K, z) - short))
    for seg, M in (((5, 17, 7), 3 * 5), ((401, 401, 0), 2 * 401), ((130, 401, 200), 2 * 130)):
        for N, K in ((96, 128), (1920, 640)):
            for planes in (0, B_LO, A_LO | B_LO):
                for acc in (0, 1):
                    yield case("seg", M, N, K, lda=K + 64, ldc=N + 4, planes=planes, bias=1 - acc, acc=acc, extras=seg)
    yield from ERRORS


def key(c):
    return json.dumps(c, separators=(",", ":"))


@pytest.fixture(scope="module")
def ops():
    from cruse_amd import ops as o
    return o


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden(recorded):
    assert len(recorded["index"]) == sum(1 for _ in cases())
    return {key(c): recorded["results"][i] for c, i in zip(cases(), recorded["index"])}


def _plan(ops, c):
    """the recorded form of a result: the 16 figures, or [code, message] of the refusal"""
    form, M, N, K, lda, a_ks, ldb, b_ks, ldc, planes, bias, acc, splitk, f16, dt, extras = c
    try:
        return ops.gemm_bf16_plan(form, M, N, K, lda, a_ks, ldb, b_ks, ldc, planes=planes, bias=bias, accumulate=acc, splitk=splitk, operands_f16=f16,
                                  out_dtype=dt, extras=extras)["raw"]
    except RuntimeError as e:
        head, _, msg = str(e).partition(": ")
        return [int(head.rsplit(" ", 1)[1]), msg]


_BUF = ctypes.create_string_buffer(96)
_DEV = []


def standin():
    """a 16-byte aligned stand-in for every tensor: the host only asks whether a pointer is null.  The DIRECT calls are made where they must be
    refused; should a check regress, the entry point would launch on the stand-in, so where a device is present it is 1 MiB of device memory
    (more than the tensors of any DIRECT call), and host memory only where nothing can launch"""
    import torch
    if torch.cuda.is_available():
        if not _DEV:
            _DEV.append(torch.zeros(1 << 18, dtype=torch.float32, device="cuda"))
        return _DEV[0].data_ptr()
    return (ctypes.addressof(_BUF) + 15) & ~15


def call_direct(lib, which):
    """the call of the real entry point for an entry of DIRECT (ctypes handle with cruse_amd._lib's signatures): refused, so nothing launches"""
    P = standin()
    if which == DIRECT[0]:
        return lib.cruse_gemm_bf16_nt_slabs(128, 128, 128, P, 128, 64, P, 128, 64, P, 128, 2, None, 0, None)
    if which == DIRECT[1]:
        ms, ar, bs = (ctypes.c_int * 3)(70, 200, 33), (ctypes.c_longlong * 3)(0, 0, 70), (ctypes.c_void_p * 3)(P, None, P)
        return lib.cruse_gemm_bf16_nt_slabs_cat(3, ctypes.cast(ms, ctypes.c_void_p), 96, 128, P, ctypes.cast(ar, ctypes.c_void_p), 64, 64 * 400,
                                                ctypes.cast(bs, ctypes.c_void_p), 128, 64, P, 96, 2, P, 1 << 18, None)
    return lib.cruse_gemm_bf16x3_nt(128, 128, 64, P, P, 64, 64, P + 32, P + 48, 64, 64, P, 128, None, 0, None)


def test_the_recorded_file_covers_the_matrix(golden, recorded):
    rows = [(c, golden[key(c)]) for c in cases()]
    # all 14 instantiated kernels and every refusal of the host path are in the file, from the parent alone
    assert {(r[0], r[1], bool(r[2]), bool(r[3])) for _, r in rows if len(r) == 16} == VARIANTS
    assert all(len(golden[key(c)]) == 2 for c in ERRORS) and all(len(r) == 2 for r in recorded["direct"]) and len(recorded["direct"]) == len(DIRECT)
    said = {r[1] for _, r in rows if len(r) == 2} | {r[1] for r in recorded["direct"]}
    assert all(any(m in s for s in said) for m in REFUSALS), [m for m in REFUSALS if not any(m in s for s in said)]
    # deep: three stages from 64 k-tiles per slice on, not at 63 -- and never for the f16 forms
    deep = {r[7]: r[1] for c, r in rows if c[0] == "plain" and len(r) == 16}
    assert deep[64] == 3 and deep[63] == 2 and all(n == (3 if k >= 64 else 2) for k, n in deep.items())
    assert all(r[1] == 2 for c, r in rows if len(r) == 16 and (c[0] in ("f16", "f16x2", "atr") or c[13]))
    assert golden[key(case("f16", 1920, 640, 25664, bias=1))][:8] == [0, 2, 1, 0, 80, 65536, 1, 401]
    # a negative split-K pins the slices to XCDs only where more than one is left after clamping
    assert all(r[8] == int(c[12] < -1 and r[6] > 1) for c, r in rows if len(r) == 16)
    assert golden[key(case("plain", 1, 1, 64, acc=1, splitk=-8))][6:9] == [1, 1, 0]
    assert golden[key(case("plain", 1920, 640, 25664, acc=1, splitk=-8))][6:9] == [8, 51, 1]
    # concatenated products that end inside a tile: 1 + 2 + 1 row tiles, 303 output rows
    r = golden[key(case("slabs_cat", 0, 96, 4096, "ktiled", a_ks=64 * 400, splitk=-8,
                        extras=cat_extras((70, 200, 33), (0, 0, 70), 3, slab_bytes(303, 96, 4096, -8))))]
    assert (r[0], r[9], r[13], r[14]) == (4, 4, 303, 303 * 96)
    one_short = golden[key(case("slabs", 200, 96, 4096, splitk=3, extras=(slab_bytes(200, 96, 4096, 3) - 1,)))]
    assert one_short[0] == -1 and "do not fit" in one_short[1]


def test_gemm_plan_is_what_the_parent_launched(ops, golden):
    for c in cases():
        got = _plan(ops, c)
        assert got == golden[key(c)], (c, got, golden[key(c)])


def test_pointer_refusals_are_the_parents(recorded):
    from cruse_amd._lib import lib
    for which, want in zip(DIRECT, recorded["direct"]):
        assert [call_direct(lib, which), lib.cruse_last_error().decode()] == want, which
