"""CPU: what the 14 boundary entry points of the streaming server launch for a call (cruse_stream_boundary_plan / ops.stream_boundary_plan) --
kernel family, template instance (DEC, s16, LIM, PF), grid, block, dynamic LDS bytes and the packet geometry -- or the error the entry point
answers with.  A host-side decision: the library loads without a GPU.

The expected results (tests/golden/stream_boundary_plan_parent.json) were recorded from the library as it was BEFORE the entry points were
gathered onto one call descriptor, never from the code under test.  A build of the parent commit (stream.hip and abi.cpp alone, linked into a
library of their own) got a scratch patch, kept out of the repository: launch_encode, launch_decode, launch_encode_n, launch_decode_n and the two
launch sites of the DeepFilter head wrote the 11 figures (family, DEC, s16, LIM, PF, grid x, block x, dynamic LDS bytes, WS, rowmax, wcap; the
last three 0 for a single hop and for the head) into a caller-supplied array right before cruse_ensure_dyn_lds / the launch, and returned
instead of launching.  That build's own 14 entry points (cruse_stream_encode ... cruse_stream_df_head_n) were then called with 16-byte aligned
stand-in pointers over cases() below, and their return code, cruse_last_error() and the array were written down.  Every refusal of the boundary
host path happens before anything is read through a pointer, so DIRECT, the refusals only a pointer can trigger, were recorded the same way and
are asked of the real entry points here (as is one refusal per family that a scalar triggers).  direct_each(), refusals of each of the 14
entry points that repeat its arguments, came from an unpatched build of the parent in the same way.  The file pins that refactor, and every later
one, to the same choices and messages.  Its layout: "results", the distinct outcomes (the 11 figures, or [code, message] of a refusal);
"index", one entry into "results" per case of cases(), in that order.

A case is (entry, args): the entry point's arguments in its order without the stream, a pointer as 1 (present) or 0 (null).

Which case meets which CRUSE_REQUIRE of the boundary host path (REFUSALS holds a piece of each message):
  make_layout   "channel count"       ch (1, 600, 8, 16, 32);   "must be 1"  ch (2, 4, 8, 16, 32);   "exceeds 2048"  ch (1, 32, 8, 16, 32)
  encode/decode "S = 0 or a null buffer" / "S = -1 or ..."  S in (0, -1) and a null flag per pointer, single hop
                "null buffer"         a null flag per pointer, packets
  packet_args   "need work_frames >= hops + 1"   S in (0, -1), hops = 0, work_frames = hops;   "whose rows fit in LDS"  hops = max_hops + 1 and
                work_frames = max_hops + 2
                "in_hops = " / "out_hops = "     io_hops = hops - 1
  fmt_args      "unknown sample format"          fmt 2 (encode, decode, the head)
  out_args      "a clip counter needs s16"       clip with fmt 0 (decode, the head)
  pf_args       "post-filter kind"    pf_kind 0 and 3 with _pf, 3 with _up;   "null pf_tau"   kind 1 and 2 without pf_tau, _pf and _up
  df head       "only the DeepFilter(1, 5)"  (t_dim, f_dim) (2, 5), (1, 3);   "(need S >= 1)"  S in (0, -1);   "null buffer"  a null flag per pointer
                "do not lie in a work row"   wk_re / wk_im / wk_mask once outside, and a row of 481 floats;   "df_state rows of"  st_stride - 1
                "df_work rows of"     dw_stride 321;   "hops = "  hops 0 and 48, work_frames = hops, out_hops = hops - 1, dw_frames = hops - 1
TWO_FAULTS are calls with two faults each: the refactor reports the one the parent reported."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_boundary_plan_parent.json")
ENTRIES = ("encode", "encode_io", "decode", "decode_io", "decode_pf", "decode_up", "encode_n", "encode_n_io", "decode_n", "decode_n_io",
           "decode_n_pf", "decode_n_up", "df_head", "df_head_n")
CHS = ((1, 4, 8, 16, 32), (1, 3, 5, 6, 8), (1, 8, 16, 32, 64))
BAD_CHS = ((2, 4, 8, 16, 32), (1, 600, 8, 16, 32), (1, 32, 8, 16, 32))
MAX_HOPS = {(1, 4, 8, 16, 32): 44, (1, 3, 5, 6, 8): 47, (1, 8, 16, 32, 64): 14}      # stream_packet_layout, asserted below
DF_MAX_HOPS = 47
LN_EPS = 1e-5
# (out_fmt, lim, clip): every format with and without a limit and a counter
IO = [(fmt, lim, clip) for fmt in (0, 1, 2) for lim in (0, 1) for clip in (0, 1)]
PF = [(kind, tau) for kind in (0, 1, 2, 3) for tau in (0, 1)]
FULL = (1, 1, 1)            # s16, a limit, a counter


def encode(io, ch, S=1, packet=None, fmt=0, ptrs=(1,) * 6):
    """packet: None, or (hops, in_hops, work_frames).  ptrs: ctl, in, tab, w, state, work"""
    name = "encode" + ("_n" if packet else "") + ("_io" if io else "")
    return name, (ptrs[0], S) + tuple(packet or ()) + tuple(ch) + (ptrs[1],) + ((fmt,) if io else ()) + tuple(ptrs[2:])


def decode(form, ch, S=1, packet=None, io=(0, 0, 0), pf=(1, 1), ptrs=(1,) * 6):
    """form: "", "_io", "_pf", "_up".  io: (out_fmt, lim, clip); pf: (pf_kind, pf_tau).  ptrs: ctl, tab, w, state, work, out"""
    tail = () if form == "" else tuple(io) if form == "_io" else tuple(io) + tuple(pf)
    return "decode" + ("_n" if packet else "") + form, (ptrs[0], S) + tuple(packet or ()) + tuple(ch) + (ptrs[1], ptrs[2], LN_EPS) + tuple(ptrs[3:]) + tail


def head(lay, S=1, packet=None, drain=0, io=(0, 0, 0), dims=(1, 5), st_stride=None, dw=None, ptrs=(1,) * 6, **off):
    """lay: (wk_stride, wk_re, wk_im, wk_mask, df stride).  packet: None, or (hops, out_hops, work_frames); dw: dw_stride, or dw_frames.
    ptrs: ctl, work, tab, df_state, df_work, out"""
    ws, re_, im, mask, stride = lay
    rows = (off.get("wk_stride", ws), off.get("wk_re", re_), off.get("wk_im", im), off.get("wk_mask", mask))
    dw = (packet[0] if packet else 322) if dw is None else dw
    return "df_head" + ("_n" if packet else ""), ((ptrs[0], S) + (tuple(packet) if packet else (drain,)) + (ptrs[1],) + rows
                                                   + (ptrs[2], ptrs[3], stride if st_stride is None else st_stride, ptrs[4], dw, ptrs[5]) + tuple(io) + tuple(dims))


def one_null(n, i):
    return tuple(int(j != i) for j in range(n))


def packets(ch):
    """(hops, io_hops, work_frames) of the packet sweep: every hops with the tight and a roomy buffer, then one figure too small"""
    m = MAX_HOPS[ch]
    out = [(h, h, h + 1) for h in (1, 2, m, m + 1)] + [(2, 3, 3), (2, 2, 4), (m, m, m + 2), (2, 1, 3), (2, 2, 2), (0, 0, 1), (1, 0, 2)]
    return out


def head_layouts():
    from cruse_amd import ops
    stride = ops.stream_df_layout()["stride"]
    for ch in CHS:
        lay, play = ops.stream_layout(ch), ops.stream_packet_layout(ch)
        yield (lay["wk_stride"], lay["wk_re"], lay["wk_im"], lay["wk_mask"], stride), (play["wk_stride"], lay["wk_re"], lay["wk_im"], lay["wk_mask"], stride)


TWO_FAULTS = [
    encode(1, BAD_CHS[0], S=0, fmt=2, ptrs=one_null(6, 1)),                        # the channels come first
    encode(1, CHS[0], S=0, fmt=2),                                                 # S before the format
    encode(1, CHS[0], packet=(2, 1, 2), fmt=2, ptrs=one_null(6, 3)),               # a null buffer before the packet's figures
    encode(1, CHS[0], packet=(2, 1, 2), fmt=2),                                    # work_frames before in_hops before the format
    encode(1, CHS[0], packet=(2, 1, 3), fmt=2),
    decode("_pf", BAD_CHS[0], S=0, io=(2, 1, 1), pf=(3, 0)),                       # the post-filter's kind comes first of all
    decode("_pf", BAD_CHS[0], S=0, io=(2, 1, 1), pf=(1, 0)),                       # ... and its tau
    decode("_up", BAD_CHS[1], S=0, io=(0, 1, 1), pf=(0, 0)),                       # then the channels
    decode("_io", CHS[1], S=-1, io=(2, 0, 1)),                                     # S before the format
    decode("_io", CHS[1], io=(2, 0, 1)),                                           # the format before the counter
    decode("_up", CHS[1], packet=(2, 1, 2), io=(0, 0, 1), pf=(2, 1), ptrs=one_null(6, 5)),
    decode("_up", CHS[1], packet=(2, 1, 2), io=(0, 0, 1), pf=(2, 1)),
    decode("_up", CHS[1], packet=(2, 1, 3), io=(0, 0, 1), pf=(2, 1)),              # out_hops before the counter
    decode("_pf", CHS[2], packet=(23, 22, 24), io=(2, 0, 0)),                      # the LDS budget before out_hops
]

# refusals through the real entry points: refused before any launch, so they run wherever the library loads.  Those only a pointer triggers (a
# null flag for each pointer of one entry point per family and hop form) and one scalar refusal per family
DIRECT = ([encode(1, CHS[0], fmt=1, ptrs=one_null(6, i)) for i in range(6)] + [encode(0, CHS[0], packet=(2, 2, 3), ptrs=one_null(6, i)) for i in range(6)]
          + [decode("_io", CHS[1], io=FULL, ptrs=one_null(6, i)) for i in range(6)]
          + [decode("_up", CHS[1], packet=(2, 2, 3), io=FULL, ptrs=one_null(6, i)) for i in range(6)]
          + [decode("_pf", CHS[1], io=FULL, pf=(1, 0)), decode("_up", CHS[1], packet=(2, 2, 3), pf=(2, 0)), decode("", CHS[2], S=0),
             encode(1, CHS[2], fmt=2), decode("_io", CHS[2], packet=(2, 2, 3), io=(0, 0, 1)), decode("_pf", CHS[2], pf=(0, 1))])
CH_AT = ((2, 4, 8, 16, 32),) + tuple(CHS[0][:k] + (600,) + CHS[0][k + 1:] for k in (1, 2, 3, 4))       # a refused channel count at each index


def direct_each():
    """More of DIRECT: for each of the 14 entry points a null flag per pointer and refusals whose message repeats the arguments, every int
    with a value of its own, so that an argument that reached the wrong field of the call descriptor would show"""
    for pk in (None, (5, 6, 7)):
        forms = [lambda **kw: encode(0, packet=pk, **kw), lambda **kw: encode(1, packet=pk, fmt=1, **kw)]
        forms += [lambda f=f, **kw: decode(f, packet=pk, io=FULL if f else (0, 0, 0), pf=(2, 1), **kw) for f in ("", "_io", "_pf", "_up")]
        for form in forms:
            yield from (form(ch=CHS[1], S=3, ptrs=one_null(6, i)) for i in range(6))
            yield from (form(ch=ch, S=3) for ch in CH_AT)
            yield form(ch=CHS[1], S=-7)
        yield encode(1, CHS[1], 3, pk, fmt=2)
        for f in ("_io", "_pf", "_up"):
            yield decode(f, CHS[1], 3, pk, io=(2, 1, 1), pf=(1, 1))                # the format, not the kind
            yield decode(f, CHS[1], 3, pk, io=(0, 0, 1), pf=(1, 1))                # the counter, not the limit
        for f in ("_pf", "_up"):
            yield decode(f, CHS[1], 3, pk, io=(1, 1, 0), pf=(3, 1))                # the kind, not the format
            yield decode(f, CHS[1], 3, pk, io=(1, 1, 0), pf=(1, 0))                # tau, not the limit
    for pk in ((5, 4, 7), (5, 6, 4)):                                              # out_hops / in_hops, then work_frames
        yield from (encode(io, CHS[1], 3, pk, fmt=1) for io in (0, 1))
        yield from (decode(f, CHS[1], 3, pk, io=FULL if f else (0, 0, 0), pf=(2, 1)) for f in ("", "_io", "_pf", "_up"))
    lay, play = next(head_layouts())
    for pk, L in ((None, lay), ((5, 6, 7), play)):
        yield from (head(L, 3, pk, io=FULL, ptrs=one_null(6, i)) for i in range(6))
        yield from (head(L, 3, pk, io=io) for io in ((0, 0, 1), (0, 1, 1), (2, 1, 1)))
        yield from (head(L, 3, pk, io=FULL, dims=dims) for dims in ((2, 5), (1, 3), (5, 1)))
        yield head(L, -7, pk, io=FULL)
        for off in (dict(wk_re=L[0] - 160), dict(wk_im=-1), dict(wk_mask=L[0] - 159), dict(wk_stride=481, wk_re=0, wk_im=161, wk_mask=321)):
            yield head(L, 3, pk, io=FULL, **off)
        yield head(L, 3, pk, io=FULL, st_stride=L[4] - 1)
    yield head(lay, 3, drain=1, io=FULL, dw=321)
    for pk, dw in (((48, 49, 50), 51), ((5, 4, 7), 6), ((5, 6, 4), 7), ((5, 6, 7), 3)):
        yield head(play, 3, pk, io=FULL, dw=dw)

REFUSALS = ("stream: channel count ch[1] = 600", "stream: ch[0] must be 1", "exceeds 2048", "S = 0 or a null buffer", "S = -1 or a null buffer",
            "stream_encode_n: null buffer", "stream_decode_n_up: null buffer", "(need work_frames >= hops + 1)", "whose rows fit in LDS", "in_hops = 1 < hops = 2",
            "out_hops = 1 < hops = 2", "unknown sample format 2", "a clip counter needs s16 output", "cruse_stream_decode_pf: post-filter kind 0",
            "cruse_stream_decode_n_up: post-filter kind 3", "cruse_stream_decode_up: null pf_tau", "cruse_stream_decode_n_pf: null pf_tau",
            "only the DeepFilter(1, 5) instance is built", "stream_df_head: S = 0 (need S >= 1)", "stream_df_head_n: null buffer",
            "do not lie in a work row", "df_state rows of", "stream_df_head: df_work rows of 321 floats", "stream_df_head_n: hops = 48 (1..47)")


def cases():
    """the calls of the recorded file, in its order"""
    for ch in CHS:
        for S in (1, 3):
            yield encode(0, ch, S)
            yield decode("", ch, S)
            for fmt in (0, 1, 2):
                yield encode(1, ch, S, fmt=fmt)
            for io in IO:
                yield decode("_io", ch, S, io=io)
                for pf in PF:
                    yield decode("_pf", ch, S, io=io, pf=pf)
                    yield decode("_up", ch, S, io=io, pf=pf)
            for pk in packets(ch):
                yield encode(0, ch, S, pk)
                yield encode(1, ch, S, pk, fmt=1)
                yield decode("", ch, S, pk)
                yield decode("_io", ch, S, pk, io=FULL)
                yield decode("_pf", ch, S, pk, io=FULL, pf=(1, 1))
                yield decode("_up", ch, S, pk, io=(0, 0, 0), pf=(0, 0))
            for fmt in (0, 1, 2):
                yield encode(1, ch, S, (2, 2, 3), fmt=fmt)
            for io in IO:
                yield decode("_io", ch, S, (2, 2, 3), io=io)
                for pf in PF:
                    yield decode("_pf", ch, S, (2, 2, 3), io=io, pf=pf)
                    yield decode("_up", ch, S, (2, 2, 3), io=io, pf=pf)
    for ch in BAD_CHS:
        for pk in (None, (2, 2, 3)):
            yield encode(0, ch, 1, pk)
            yield encode(1, ch, 1, pk, fmt=1)
            for form in ("", "_io", "_pf", "_up"):
                yield decode(form, ch, 1, pk)
    for S in (0, -1):
        for pk in (None, (2, 2, 3)):
            for io in (0, 1):
                yield encode(io, CHS[0], S, pk)
            for form in ("", "_io", "_pf", "_up"):
                yield decode(form, CHS[0], S, pk)
    for pk in (None, (2, 2, 3)):
        for i in range(6):
            for io in (0, 1):
                yield encode(io, CHS[1], 3, pk, ptrs=one_null(6, i))
            for form in ("", "_io", "_pf", "_up"):
                yield decode(form, CHS[1], 3, pk, io=FULL, ptrs=one_null(6, i))
    for lay, play in head_layouts():
        for S in (1, 3):
            for io in IO:
                for drain in (0, 1):
                    yield head(lay, S, drain=drain, io=io)
                yield head(play, S, (2, 2, 3), io=io)
            for h in (1, 2, DF_MAX_HOPS):
                yield head(play, S, (h, h, h + 1))
                yield head(play, S, (h, h + 1, h + 2), dw=h + 1)
    lay, play = next(head_layouts())
    for pk, L in ((None, lay), ((2, 2, 3), play)):
        for S in (0, -1):
            yield head(L, S, pk)
        for dims in ((2, 5), (1, 3)):
            yield head(L, 1, pk, dims=dims)
        for i in range(6):
            yield head(L, 1, pk, io=FULL, ptrs=one_null(6, i))
        for off in (dict(wk_re=L[0] - 160), dict(wk_im=-1), dict(wk_mask=L[0] - 159), dict(wk_stride=481, wk_re=0, wk_im=161, wk_mask=321)):
            yield head(L, 1, pk, **off)
        yield head(L, 1, pk, st_stride=L[4] - 1)
    yield head(lay, dw=321)
    yield head(lay, dw=321, io=(2, 0, 1))                                          # the format before the df_work rows
    yield head(lay, S=0, dims=(2, 5), ptrs=one_null(6, 0))                         # the instance before S before a null buffer
    yield head(lay, S=0, ptrs=one_null(6, 0))
    for pk, dw in (((0, 0, 1), 1), ((DF_MAX_HOPS + 1, 48, 49), 48), ((2, 2, 2), 2), ((2, 1, 3), 2), ((2, 2, 3), 1)):
        yield head(play, 1, pk, dw=dw)
    yield from TWO_FAULTS
    yield from DIRECT
    yield from direct_each()


def key(c):
    return json.dumps(c, separators=(",", ":"))


_BUF = ctypes.create_string_buffer(96)
_DEV = []


def standin():
    """a 16-byte aligned stand-in for every tensor: the host only asks whether a pointer is null.  The DIRECT calls are made where they must be
    refused; should a check regress, the entry point would launch on the stand-in, so where a device is present it is 4 MiB of device memory
    (more than the tensors of any DIRECT call), and host memory only where nothing can launch"""
    import torch
    if torch.cuda.is_available():
        if not _DEV:
            _DEV.append(torch.zeros(1 << 20, dtype=torch.float32, device="cuda"))
        return _DEV[0].data_ptr()
    return (ctypes.addressof(_BUF) + 15) & ~15


def call_direct(lib, signatures, c):
    """[return code, message] of the real entry point for case c (ctypes handle with cruse_amd._lib's signatures; the null stream)"""
    entry, args = c
    sig = signatures[f"cruse_stream_{entry}"][0]
    P = standin()
    rc = getattr(lib, f"cruse_stream_{entry}")(*[(P if v else None) if t == "p" else v for t, v in zip(sig, args)], None)
    return [rc, lib.cruse_last_error().decode()]


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
    """the recorded form of a result: the 11 figures, or [code, message] of the refusal"""
    try:
        return ops.stream_boundary_plan(c[0], *c[1])["raw"]
    except RuntimeError as e:
        head_, _, msg = str(e).partition(": ")
        return [int(head_.rsplit(" ", 1)[1]), msg]


def test_the_recorded_file_covers_the_matrix(ops, golden):
    assert all(ops.stream_packet_layout(ch)["max_hops"] == m for ch, m in MAX_HOPS.items()) and ops.STREAM_BOUNDARY_ENTRIES == ENTRIES
    rows = [(c, golden[key(c)]) for c in cases()]
    assert {c[0] for c, _ in rows} == set(ENTRIES)
    # every kernel instance the library builds is launched by some case: family x DEC x s16 x LIM x PF
    got = {tuple(r[:5]) for _, r in rows if len(r) == 11}
    want = ({(f, 0, s16, 0, 0) for f in (0, 1) for s16 in (0, 1)} | {(f, d, s16, lim, pf) for f in (2, 3) for d in (0, 1) for s16 in (0, 1) for lim in (0, 1) for pf in (0, 1)}
            | {(f, 0, s16, lim, 0) for f in (4, 5) for s16 in (0, 1) for lim in (0, 1)})
    assert got == want, (got ^ want)
    # the plain entry points launch the f32 instance without LIM and PF; _up with nothing set launches what the plain one would with DEC 1
    for ch in CHS:
        plain, up = golden[key(decode("", ch, 3))], golden[key(decode("_up", ch, 3, pf=(0, 0)))]
        assert plain[:5] == [2, 0, 0, 0, 0] and up[:5] == [2, 1, 0, 0, 0] and plain[5:] == up[5:] and plain[5:7] == [3, 1024] and plain[8:] == [0, 0, 0]
        assert golden[key(decode("_io", ch, 3, io=(0, 0, 0)))] == plain
    # every refusal of the host path is in the file, from the parent alone; a refused case holds [code, message]
    said = {r[1] for _, r in rows if len(r) == 2}
    assert all(any(m in s for s in said) for m in REFUSALS), [m for m in REFUSALS if not any(m in s for s in said)]
    assert all(len(golden[key(c)]) == 2 for c in TWO_FAULTS + DIRECT + list(direct_each()))
    assert {c[0] for c in direct_each()} == set(ENTRIES)
    # a packet at max_hops fits the LDS budget of 128 KiB, one frame more does not
    for ch, m in MAX_HOPS.items():
        assert golden[key(decode("", ch, 1, (m, m, m + 1)))][7] <= 128 * 1024 and "whose rows fit" in golden[key(decode("", ch, 1, (m, m, m + 2)))][1]
        assert golden[key(encode(0, ch, 1, (m, m, m + 1)))][7] <= 128 * 1024


def test_boundary_plan_is_what_the_parent_launched(ops, golden):
    for c in cases():
        got = _plan(ops, c)
        assert got == golden[key(c)], (c, got, golden[key(c)])


def test_direct_refusals_are_the_parents(golden):
    from cruse_amd._lib import SIGNATURES, lib
    for c in DIRECT + list(direct_each()):
        assert call_direct(lib, SIGNATURES, c) == golden[key(c)], c


def test_plan_arguments_are_checked(ops):
    with pytest.raises(ValueError, match="takes 13 arguments"):
        ops.stream_boundary_plan("decode", 1, 1)
    assert ops.lib.cruse_stream_boundary_plan(14, None, 0, None) != 0 and b"stream_boundary_plan: entry 14" in ops.lib.cruse_last_error()


def test_entry_point_declared_and_bound():
    from cruse_amd._abi_check import parse_header
    from cruse_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    lib_py = open(os.path.join(ROOT, "cruse_amd", "_lib.py")).read()
    sym = "cruse_stream_boundary_plan"
    assert re.search(rf"\bint {sym}\(", header), f"{sym} is not declared in include/cruse_hip.h"
    assert re.search(rf"\"{sym}\":\s*\(\"[a-zA-Z]+\",\s*\"i\"\)", lib_py), f"{sym} is not in cruse_amd/_lib.py:SIGNATURES"
    assert SIGNATURES[sym] == parse_header()[sym] == ("ipip", "i")
    names = re.search(r"enum \{ (CRUSE_STREAM_ENTRY_ENCODE,.*?) \};", header, re.S).group(1).replace("\n", " ").split(",")
    assert [n.strip() for n in names] == [f"CRUSE_STREAM_ENTRY_{e.upper()}" for e in ENTRIES] + ["CRUSE_STREAM_ENTRY_N"]
    assert "#define CRUSE_ABI_VERSION 15" in header                   # an additive symbol: the version stays
