"""MI355X: StreamingInferencer(io_rate = 8000 / 32000 / 48000) on the rate-conversion kernels (cruse_stream_resample_in / _out / _in_n /
_out_n, csrc/stream_rs.hip).

Reference: R(u) = Out(E(In(u))), the float64 restatement of tests/stream_rs_ref.py (pinned on the CPU by tests/test_stream_rs_host.py) around
the float64 per-frame restatement of tests/stream_ref.py.  Bars: 2e-5 rel-L2 per clip (the project's whole-clip bar), bit equality
wherever the same floats are expected.  Shapes: the two-channel model (g = 1) and the default one (g = 4), 3 slots, a different clip of
12 blocks of 0.1 * randn at io_rate per slot, max_hops = 4 with and without a leading push (a packet then computes 5 frames), a slot
inactive in some calls, an enhance() length that is no multiple of the block.
"""
import functools

import numpy as np
import pytest
import torch

from tests import stream_io_ref as IO
from tests import stream_ref_f16 as R
from tests import stream_rs_ref as RS
from tests.stream_ref import as_double
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
S, NB, K = IO.S, IO.NB, IO.K
NAMES = list(IO.MODELS)
RATES = RS.RATES
BAR = 2e-5

# the three ways through a clip; every slot consumes its 12 blocks, each is inactive in at least one call
PUSHES = [("p", [i != 4 + 3 * s for s in range(S)]) for i in range(NB + 1)]
PACKETS = [("k", c) for c in ([4, 4, 4], [4, 0, 4], [4, 4, 4], [0, 4, 0])]                           # starts the clip inside a packet
PUSH_PACKETS = [("p", [True] * S)] + [("k", c) for c in ([4, 4, 4], [4, 4, 0], [3, 3, 4], [0, 0, 3])]  # first packet: 5 frames
WAYS = {"pushes": PUSHES, "packets": PACKETS, "push+packets": PUSH_PACKETS}


def drive(inf, clips, calls, flush=True):
    """clips [n, nb * B] (host, float32 or int16) through `calls` -- ("p", active per slot): one push; ("k", counts per slot): one
    push_packet -- then flush of every slot that holds a clip.  -> [per-slot 1-D host tensors]"""
    B = inf.io_block
    n, nb = clips.shape[0], clips.shape[1] // B
    blocks = clips.view(n, nb, B).cuda()
    cur, outs = [0] * n, [[] for _ in range(n)]
    for kind, arg in calls:
        if kind == "p":
            blk = torch.stack([blocks[s, min(cur[s], nb - 1)] for s in range(n)])
            out, valid = inf.push(blk, arg)
            assert tuple(out.shape) == (n, B)
            out = out.cpu()
            for s in range(n):
                if arg[s]:
                    cur[s] += 1
                    if valid[s]:
                        outs[s].append(out[s])
        else:
            pkt = torch.zeros(n, max(arg), B, dtype=blocks.dtype, device="cuda")
            for s in range(n):
                pkt[s, :arg[s]] = blocks[s, cur[s]:cur[s] + arg[s]]
            out, n_out = inf.push_packet(pkt, arg)
            assert tuple(out.shape) == (n, max(arg), B)
            out = out.cpu()
            for s in range(n):
                outs[s] += [out[s, k] for k in range(int(n_out[s]))]
                cur[s] += arg[s]
    if flush:
        held = [s for s in range(n) if cur[s] >= 2]
        last = inf.flush(held).cpu()
        assert tuple(last.shape) == (len(held), B)
        for j, s in enumerate(held):
            outs[s].append(last[j])
    return [torch.cat(o) if o else torch.zeros(0) for o in outs]


def clips_at(io_rate: int, first_seed: int = 700) -> torch.Tensor:
    """[S, NB * B]: a different 0.1 * randn clip per slot"""
    B = io_rate // 100
    return torch.stack([0.1 * torch.randn(NB * B, generator=torch.Generator().manual_seed(first_seed + io_rate // 1000 + s)) for s in range(S)])


@functools.lru_cache(maxsize=None)
def model(name):
    """(float64 oracle module, product module on the device); the two-channel model under the seed stream_ref_f16.alive_model picks"""
    o = IO.oracle(name)
    return as_double(o), R.gpu_model(o, IO.MODELS[name])


@functools.lru_cache(maxsize=None)
def setup(name, io_rate):
    """(product module, clips [S, NB * B], [R of each clip]) -- computed once, shared, never modified"""
    o64, m = model(name)
    clips = clips_at(io_rate)
    return m, clips, [RS.R(o64, clips[s], io_rate) for s in range(S)]


def server(m, n_slots=S, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    return StreamingInferencer(m, n_slots, max_hops=K, **kw)


# ---- 1. output against the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io_rate", RATES)
@pytest.mark.parametrize("name", NAMES)
def test_output_against_the_reference(name, io_rate):
    m, clips, want = setup(name, io_rate)
    o64, _ = model(name)
    B = io_rate // 100
    inf = server(m, io_rate=io_rate)
    assert inf.io_block == B and inf.io_delay == RS.io_delay(io_rate) and inf.io_rate == io_rate
    assert inf.blocks.shape == (S, 160) and inf.out.shape == (S, 160) and inf.io_blocks.shape == (S, B) and inf.io_out.shape == (S, B)
    for way, calls in WAYS.items():
        got = drive(inf, clips, calls)                                     # one server: every way starts on flushed slots
        compared = []
        for s in range(S):
            err = rel_l2(got[s], want[s])
            print(f"{name} {io_rate} {way} slot {s}: vs R {err:.2e}")
            assert got[s].shape == (NB * B,) and got[s].dtype == torch.float32
            assert err <= BAR, (name, io_rate, way, s, err)
            compared.append(s)
        assert len(compared) == S
        assert float(inf.rs_state.abs().sum()) == 0.0                      # flush zeroed the histories with the slot
    # stage() keeps showing the 16 kHz rows
    drive(inf, clips, PUSH_PACKETS[:2], flush=False)
    assert inf.stage(0)["block"].shape == (160,) and inf.stage(0)["re"].shape == (161,)
    inf.reset()
    # a second clip on the flushed slots matches its own R
    clips2 = clips_at(io_rate, first_seed=900)
    got = drive(inf, clips2, PACKETS)
    for s in range(S):
        err = rel_l2(got[s], RS.R(o64, clips2[s], io_rate))
        print(f"{name} {io_rate} second clip slot {s}: vs R {err:.2e}")
        assert err <= BAR, (name, io_rate, s, err)
    # enhance(): L is no multiple of B -- the result is R of the zero-padded clip, cut to L
    L = NB * B - B // 2 - 3
    got = inf.enhance(clips[:, :L]).cpu()
    assert got.shape == (S, L)
    compared = []
    for s in range(S):
        padded = torch.cat([clips[s, :L], torch.zeros(NB * B - L)])
        err = rel_l2(got[s], RS.R(o64, padded, io_rate)[:L])
        print(f"{name} {io_rate} enhance L = {L} slot {s}: vs R {err:.2e}")
        assert err <= BAR, (name, io_rate, s, err)
        compared.append(s)
    assert len(compared) == S


# ---- 2. composition is bit-exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("io_rate", RATES)
def test_composition_is_bit_exact(io_rate, precision):
    """resample_in -> a plain 16 kHz server -> resample_out, launched by hand on whole pushes, gives the io_rate server's bits"""
    from cruse_amd import ops
    from cruse_amd.inferencer import resample
    m, clips, _ = setup("hg20_g1", io_rate)
    B = io_rate // 100
    rs, plain = server(m, io_rate=io_rate, precision=precision), server(m, precision=precision)
    taps = ops.stream_resample_taps(io_rate, "cuda")
    assert torch.equal(taps, rs.rs_taps) and taps.dtype == torch.float32
    hist = torch.zeros(S, sum(resample.history(io_rate)), device="cuda")
    mode = torch.full((S,), ops.STREAM_FRAME, dtype=torch.int32, device="cuda")
    blocks = clips.view(S, NB, B).cuda()
    for b in range(NB):
        x16 = torch.empty(S, 160, device="cuda")
        ops.stream_resample_in(mode, io_rate, blocks[:, b].contiguous(), taps, hist, x16)
        out16, valid = plain.push(x16)
        got, valid_rs = rs.push(blocks[:, b])
        assert torch.equal(rs.blocks, x16) and valid.tolist() == valid_rs.tolist()
        if b >= 1:
            y = torch.empty(S, B, device="cuda")
            ops.stream_resample_out(mode, io_rate, out16, taps, hist, y)
            assert torch.equal(y, got), (io_rate, precision, b)
    out16 = plain.flush(list(range(S)))
    y = torch.empty(S, B, device="cuda")
    ops.stream_resample_out(mode, io_rate, out16, taps, hist, y)
    assert torch.equal(y, rs.flush(list(range(S))))


@pytest.mark.parametrize("io_rate", RATES)
def test_graph_equals_eager_and_slots_are_independent(io_rate):
    m, clips, _ = setup("hg20_g1", io_rate)
    graph = drive(server(m, io_rate=io_rate), clips, PUSH_PACKETS)
    eager = drive(server(m, io_rate=io_rate, use_graph=False), clips, PUSH_PACKETS)
    for s in range(S):
        assert torch.equal(graph[s], eager[s]), (io_rate, s)
    # slot 1 alone on a one-slot server, through the calls in which it was active
    mine = [(k, [arg[1]]) for k, arg in PUSH_PACKETS if arg[1]]
    one = drive(server(m, n_slots=1, io_rate=io_rate), clips[1:2], mine)
    assert torch.equal(one[0], graph[1])


# ---- 3. the attenuation limit ----------------------------------------------------------------------------------------------------------------
def test_limit_of_zero_db_is_the_two_converters():
    """0 dB: the 16 kHz chain passes its input through, so the output is Out(In(u)) of the restatement"""
    io_rate = 48000
    m, clips, _ = setup("hg20_g1", io_rate)
    inf = server(m, io_rate=io_rate, atten_lim=True)
    inf.set_atten_lim(0.0)
    for way in ("pushes", "push+packets"):
        got = drive(inf, clips, WAYS[way])
        for s in range(S):
            err = rel_l2(got[s], RS.resample_out(RS.resample_in(clips[s], io_rate), io_rate))
            print(f"0 dB at {io_rate} {way} slot {s}: vs Out(In(u)) {err:.2e}")
            assert err <= BAR, (way, s, err)


# ---- 4. PCM -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io_rate", [8000, 48000])
def test_pcm_in_and_out(io_rate):
    m, _, _ = setup("hg20_g1", io_rate)
    B = io_rate // 100
    v = torch.stack([IO.pcm_noise(NB * B, 400 + s) for s in range(S)])     # int16, about -12 dBFS
    x = v.float() / 32768.0
    for way in ("pushes", "push+packets"):
        y = drive(server(m, io_rate=io_rate), x, WAYS[way])                # the float instance fed v / 32768
        pcm = server(m, io_rate=io_rate, pcm_in=True, pcm_out=True)
        assert pcm.io_blocks.dtype == pcm.io_out.dtype == torch.int16 and pcm.blocks.dtype == pcm.out.dtype == torch.float32
        q = drive(pcm, v, WAYS[way])
        for s in range(S):
            want, _ = IO.quantise(y[s].numpy())
            assert q[s].dtype == torch.int16 and q[s].shape == (NB * B,)
            assert np.array_equal(q[s].numpy(), want), (io_rate, way, s)
        assert pcm.clipped().tolist() == [0] * S


@pytest.mark.parametrize("io_rate", [8000, 48000])
def test_clip_counter(io_rate):
    """a loud clip through the 0 dB passthrough: clipped() is the count of the float instance's samples outside the int16 range"""
    m, _, _ = setup("hg20_g1", io_rate)
    B = io_rate // 100
    x = 2.0 * torch.randn(S, NB * B, generator=torch.Generator().manual_seed(9))
    calls = [(k, [a if s != 1 else (False if k == "p" else 0) for s, a in enumerate(arg)]) for k, arg in PUSH_PACKETS]   # slot 1 never active
    flt, pcm = server(m, io_rate=io_rate, atten_lim=True), server(m, io_rate=io_rate, atten_lim=True, pcm_out=True)
    for inf in (flt, pcm):
        inf.set_atten_lim(0.0)
    y, q = drive(flt, x, calls), drive(pcm, x, calls)
    n = pcm.clipped()
    assert q[1].numel() == 0 and n[1] == 0
    for s in (0, 2):
        want, clamped = IO.quantise(y[s].numpy())
        print(f"{io_rate} slot {s}: clipped() {n[s]}, samples of the float instance outside int16 {int(clamped.sum())} of {NB * B}")
        assert np.array_equal(q[s].numpy(), want) and n[s] == int(clamped.sum()) and n[s] > 100


# ---- 5. bounds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io_rate", RATES)
def test_tensors_stay_inside_their_rows(io_rate):
    """the io tensors, rs_state and the counters as views into larger buffers with B sentinel elements on each side"""
    m, _, _ = setup("hg20_g1", io_rate)
    B = io_rate // 100
    v = torch.stack([IO.pcm_noise(NB * B, 500 + s, dbfs=-3.0) for s in range(S)])
    kw = dict(io_rate=io_rate, pcm_in=True, pcm_out=True)
    free_inf = server(m, **kw)
    free = drive(free_inf, v, PUSH_PACKETS)
    inf = server(m, **kw)
    guards = {}

    def guarded(name, sentinel):
        t = getattr(inf, name)
        buf = torch.full((t.numel() + 2 * B,), sentinel, dtype=t.dtype, device="cuda")
        view = buf[B:B + t.numel()].view(t.shape)
        view.copy_(t)
        setattr(inf, name, view)
        guards[name] = (buf, sentinel, t.numel())

    for name in ("io_blocks", "io_out", "io_pblocks", "io_pout"):
        guarded(name, 12345)
    for name in ("blocks", "out", "pblocks", "pout"):
        guarded(name, 7.5)
    guarded("rs_state", 0.5)
    guarded("clip", 777)
    got = drive(inf, v, PUSH_PACKETS)                                      # a push, packets at max_hops (5 frames), short packets, flush
    torch.cuda.synchronize()
    for name, (buf, sentinel, n) in guards.items():
        assert bool((buf[:B] == sentinel).all()) and bool((buf[B + n:] == sentinel).all()), f"{name}: a sentinel was overwritten"
    for s in range(S):
        assert torch.equal(got[s], free[s])
    assert inf.clipped().tolist() == free_inf.clipped().tolist()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from cruse_amd import _lib, ops
    from cruse_amd.inferencer import StreamingInferencer
    _, m = model("hg20_g1")
    for bad in (44100, 16001, None):
        with pytest.raises(ValueError, match="8000, 16000, 32000, 48000"):
            StreamingInferencer(m, S, io_rate=bad)
    inf = server(m, io_rate=48000)
    with pytest.raises(ValueError, match="480"):
        inf.push(torch.zeros(S, 160, device="cuda"))
    with pytest.raises(ValueError, match="480"):
        inf.push_packet(torch.zeros(S, 2, 160, device="cuda"))
    with pytest.raises(ValueError, match="960"):
        inf.enhance(torch.zeros(S, 640))
    assert list(inf.nblk) == [0] * S and not inf._graphs
    # the C entry points
    lib = _lib.lib
    z = lambda n, dt=torch.float32: torch.zeros(n, device="cuda", dtype=dt)
    ctl = z(2 * S, torch.int32)
    ctl[:S] = ops.STREAM_FRAME                                             # would convert if it were launched
    ctl[S:] = 1
    taps, hist, lo, io, cnt = ops.stream_resample_taps(48000, "cuda"), z(S * 128), z(S * K * 160), z(S * K * 480), z(S, torch.int32)
    lo += 1.0
    io += 1.0
    p = lambda t: t.data_ptr()
    for rate in (16000, 44100, 0):
        assert lib.cruse_stream_resample_in(p(ctl), S, rate, p(io), 0, p(taps), p(hist), 128, p(lo), None) != 0
        assert b"stream_resample_in: unknown io_rate" in lib.cruse_last_error()
        assert lib.cruse_stream_resample_out_n(p(ctl), S, K, K, rate, p(lo), p(taps), p(hist), 128, p(io), 0, None, None) != 0
        assert b"stream_resample_out_n: unknown io_rate" in lib.cruse_last_error()
    for fmt in (2, -1):
        assert lib.cruse_stream_resample_in_n(p(ctl), S, K, K, 48000, p(io), fmt, p(taps), p(hist), 128, p(lo), None) != 0
        assert b"stream_resample_in_n: unknown sample format" in lib.cruse_last_error()
        assert lib.cruse_stream_resample_out(p(ctl), S, 48000, p(lo), p(taps), p(hist), 128, p(io), fmt, None, None) != 0
        assert b"stream_resample_out: unknown sample format" in lib.cruse_last_error()
    assert lib.cruse_stream_resample_out(p(ctl), S, 48000, p(lo), p(taps), p(hist), 128, p(io), 0, p(cnt), None) != 0
    assert b"clip counter needs s16 output" in lib.cruse_last_error()
    assert lib.cruse_stream_resample_out_n(p(ctl), S, K, K, 48000, p(lo), p(taps), p(hist), 128, p(io), 0, p(cnt), None) != 0
    assert lib.cruse_stream_resample_in_n(p(ctl), S, K, K - 1, 48000, p(io), 0, p(taps), p(hist), 128, p(lo), None) != 0
    assert b"in_hops = 3 < hops = 4" in lib.cruse_last_error()
    assert lib.cruse_stream_resample_out_n(p(ctl), S, K, K - 1, 48000, p(lo), p(taps), p(hist), 128, p(io), 0, None, None) != 0
    assert b"out_hops = 3 < hops = 4" in lib.cruse_last_error()
    assert lib.cruse_stream_resample_in(p(ctl), S, 48000, p(io), 0, p(taps), p(hist), 127, p(lo), None) != 0
    assert b"rs_stride" in lib.cruse_last_error()
    assert lib.cruse_stream_resample_in(p(ctl), S, 48000, p(io), 0, None, p(hist), 128, p(lo), None) != 0
    assert b"null buffer" in lib.cruse_last_error()
    with pytest.raises(RuntimeError, match="480"):
        ops.stream_resample_in(ctl[:S], 48000, z(S * 160).view(S, 160), taps, hist.view(S, 128), lo[:S * 160].view(S, 160))
    torch.cuda.synchronize()
    assert float(hist.abs().sum()) == 0.0 and int(cnt.sum()) == 0          # nothing was launched
    assert bool((lo == 1.0).all()) and bool((io == 1.0).all())


# ---- 7. the default is unchanged ------------------------------------------------------------------------------------------------------------
def test_sixteen_kilohertz_is_the_server_without_the_argument():
    _, m = model("hg20_g1")
    clips = IO.clips()
    plain, same = server(m), server(m, io_rate=16000)
    assert same.rs_state is None and same.rs_taps is None and not hasattr(same, "io_blocks") and not hasattr(same, "io_pout")
    assert same.io_block == 160 and same.io_delay == 0
    for way, calls in WAYS.items():
        a, b = drive(plain, clips, calls), drive(same, clips, calls)
        for s in range(S):
            assert a[s].shape == (NB * 160,) and torch.equal(a[s], b[s]), (way, s)
