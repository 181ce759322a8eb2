"""MI355X: the streaming I/O modes -- StreamingInferencer(atten_lim=True / pcm_in=True / pcm_out=True) on the I/O forms of the four
boundary kernels (cruse_stream_encode_io / _decode_io / _encode_n_io / _decode_n_io).

Reference: R(x, lim) = lim * x + (1 - lim) * E64(x), E64 the float64 per-frame restatement (tests/stream_io_ref.py, pinned on the CPU by
tests/test_stream_io_host.py).  Bars: 2e-5 rel-L2 per clip (the project's per-clip bar), 1 LSB for PCM samples, bit equality wherever
the same floats are expected.  Shapes: the two-channel model (g = 1) and the default one (g = 4), 3 slots, clips of 12 blocks, a
different clip per slot, max_hops = 4 with and without a leading push (a packet then computes 5 frames), a slot inactive in some calls.
"""
import functools

import numpy as np
import pytest
import torch

from tests import stream_io_ref as IO
from tests import stream_ref_f16 as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
S, NB, K, L = IO.S, IO.NB, IO.K, IO.L
NAMES = list(IO.MODELS)
BAR = 2e-5

# the three ways through a clip; every slot consumes its 12 blocks, each is inactive in at least one call
PUSHES = [("p", [i != 4 + 3 * s for s in range(S)]) for i in range(NB + 1)]
PACKETS = [("k", c) for c in ([4, 4, 4], [4, 0, 4], [4, 4, 4], [0, 4, 0])]                           # starts the clip inside a packet
PUSH_PACKETS = [("p", [True] * S)] + [("k", c) for c in ([4, 4, 4], [4, 4, 0], [3, 3, 4], [0, 0, 3])]  # first packet: 5 frames
WAYS = {"pushes": PUSHES, "packets": PACKETS, "push+packets": PUSH_PACKETS}


def drive(inf, clips, calls, flush=True, after=None):
    """clips [n, L] (host, float32 or int16) through `calls` -- ("p", active per slot): one push; ("k", counts per slot): one push_packet --
    then flush of every slot that holds a clip.  after(i): called after call i.  -> [per-slot 1-D host tensors]"""
    n, nb = clips.shape[0], clips.shape[1] // 160
    blocks = clips.view(n, nb, 160).cuda()
    cur, outs = [0] * n, [[] for _ in range(n)]
    for i, (kind, arg) in enumerate(calls):
        if kind == "p":
            blk = torch.stack([blocks[s, min(cur[s], nb - 1)] for s in range(n)])
            out, valid = inf.push(blk, arg)
            out = out.cpu()
            for s in range(n):
                if arg[s]:
                    cur[s] += 1
                    if valid[s]:
                        outs[s].append(out[s])
        else:
            pkt = torch.zeros(n, max(arg), 160, dtype=blocks.dtype, device="cuda")
            for s in range(n):
                pkt[s, :arg[s]] = blocks[s, cur[s]:cur[s] + arg[s]]
            out, n_out = inf.push_packet(pkt, arg)
            out = out.cpu()
            for s in range(n):
                outs[s] += [out[s, k] for k in range(int(n_out[s]))]
                cur[s] += arg[s]
        if after is not None:
            after(i)
    if flush:
        held = [s for s in range(n) if cur[s] >= 2]
        last = inf.flush(held).cpu()
        for j, s in enumerate(held):
            outs[s].append(last[j])
    return [torch.cat(o) if o else torch.zeros(0) for o in outs]


@functools.lru_cache(maxsize=None)
def setup(name):
    """(oracle module, product module on the device, clips [S, L], [E64 of each clip]) -- computed once, shared, never modified"""
    o = IO.oracle(name)
    clips = IO.clips()
    return o, R.gpu_model(o, IO.MODELS[name]), clips, [IO.e64(o, clips[s]) for s in range(S)]


def server(m, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    return StreamingInferencer(m, S, max_hops=K, **kw)


# ---- 1. limit off = today ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_limits_of_zero_are_todays_output(name):
    _, m, clips, _ = setup(name)
    plain, lim = server(m), server(m, atten_lim=True)
    assert plain.lim is None and plain.clip is None and plain.out.dtype == plain.blocks.dtype == torch.float32   # nothing new allocated
    assert lim.lim.dtype == torch.float32 and float(lim.lim.abs().sum()) == 0.0
    for way, calls in WAYS.items():
        a, b = drive(plain, clips, calls), drive(lim, clips, calls)
        for s in range(S):
            assert a[s].shape == (L,) and torch.equal(a[s], b[s]), (name, way, s)
    lim.set_atten_lim(None)
    lim.set_atten_lim(float("inf"), [1])
    assert float(lim.lim.abs().sum()) == 0.0


# ---- 2. limits against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_limits_against_the_reference(name):
    _, m, clips, e64 = setup(name)
    want = [IO.mix(clips[s], e64[s], IO.gain(IO.LIMS_DB[s])) for s in range(S)]
    plain, lim = server(m), server(m, atten_lim=True)
    lim.set_atten_lim(list(IO.LIMS_DB))
    assert lim.lim.cpu().tolist() == [np.float32(IO.gain(d)) for d in IO.LIMS_DB]
    mo = lim.lay["wk_mask"]
    for way, calls in WAYS.items():
        a, b = drive(plain, clips, calls), drive(lim, clips, calls)
        for s in range(S):
            err = rel_l2(b[s], want[s])
            print(f"{name} {way} slot {s} limit {IO.LIMS_DB[s]} dB: vs R {err:.2e}")
            assert b[s].shape == (L,) and err <= BAR, (name, way, s, err)
        # stage()["mask"], the wk_mask rows, keep the raw model mask: bit-equal to the default instance's after the same calls
        for s in range(S):
            assert torch.equal(plain.stage(s)["mask"], lim.stage(s)["mask"])
        assert torch.equal(plain.work[:, mo:mo + 160], lim.work[:, mo:mo + 160])
        assert torch.equal(plain.pwork[:, :, mo:mo + 160], lim.pwork[:, :, mo:mo + 160])
        assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])   # and the limits did act
        print(f"{name} {way}: the 0 dB slot vs its input (delayed passthrough): rel-L2 {rel_l2(b[2], clips[2]):.2e}, "
              f"max abs {float((b[2] - clips[2]).abs().max()):.2e}")
    got = lim.enhance(clips)                                              # enhance() keeps the slots' limits: they survive reset / flush
    for s in range(S):
        err = rel_l2(got[s], want[s])
        print(f"{name} enhance slot {s} limit {IO.LIMS_DB[s]} dB: vs R {err:.2e}")
        assert err <= BAR, (name, s, err)
    assert lim.lim.cpu().tolist() == [np.float32(IO.gain(d)) for d in IO.LIMS_DB]


# ---- 3. a limit changed mid-clip under a captured graph ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_limit_changed_mid_clip_keeps_the_graphs(name):
    """The limit changes after block 5.  Output block b overlap-adds frame b (second half) and frame b + 1 (first half), so blocks 0..4 come
    from frames computed with the old limit alone, blocks 6..11 from frames with the new one alone, and block 5 mixes both: it belongs to
    neither reference and is not compared."""
    _, m, clips, e64 = setup(name)
    old_db, new_db = [12.0, None, 0.0], [None, 3.0, 20.0]
    ways = {"pushes": ([("p", [True] * S)] * 6, [("p", [True] * S)] * 6),
            "packets": ([("k", [4] * S), ("k", [2] * S)], [("k", [4] * S), ("k", [2] * S)])}
    for way, (first, second) in ways.items():
        inf = server(m, atten_lim=True)
        inf.set_atten_lim(old_db)
        graphs = {}

        def after(i):
            if i == len(first) - 1:                                       # blocks 0..5 are in
                graphs["before"] = sorted(map(str, inf._graphs))
                inf.set_atten_lim(new_db)
            if i == len(first) + len(second) - 1:                         # the same calls again, before the flush (a chain of its own)
                graphs["after"] = sorted(map(str, inf._graphs))

        got = drive(inf, clips, first + second, after=after)
        assert len(graphs["before"]) == 2 and graphs["after"] == graphs["before"], (way, graphs)
        for s in range(S):
            r_old = IO.mix(clips[s], e64[s], IO.gain(old_db[s]))
            r_new = IO.mix(clips[s], e64[s], IO.gain(new_db[s]))
            e_old, e_new = rel_l2(got[s][:5 * 160], r_old[:5 * 160]), rel_l2(got[s][6 * 160:], r_new[6 * 160:])
            cross = rel_l2(got[s][6 * 160:], r_old[6 * 160:])
            print(f"{name} {way} slot {s}: blocks 0..4 vs R(old) {e_old:.2e}, blocks 6..11 vs R(new) {e_new:.2e} (vs R(old) {cross:.2e})")
            assert got[s].shape == (L,) and e_old <= BAR and e_new <= BAR, (name, way, s, e_old, e_new)
            assert cross > 1e-2                                           # the change is visible


# ---- 4. PCM -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", NAMES)
def test_pcm_in_and_out(name, precision):
    o, m, _, _ = setup(name)
    v = torch.stack([IO.pcm_noise(L, 400 + s) for s in range(S)])          # int16, about -12 dBFS
    x = v.float() / 32768.0
    ref64 = [IO.quantise(IO.e64(o, x[s]).float().numpy())[0] for s in range(S)] if precision == "f32" else None
    for way in ("pushes", "push+packets"):
        calls = WAYS[way]
        y = drive(server(m, precision=precision), x, calls)                # the float instance of the same precision
        q = drive(server(m, precision=precision, pcm_in=True, pcm_out=True), v, calls)
        for s in range(S):
            want, _ = IO.quantise(y[s].numpy())
            assert q[s].dtype == torch.int16 and q[s].shape == (L,)
            d = np.abs(q[s].numpy().astype(np.int64) - want.astype(np.int64))
            print(f"{name} {precision} {way} slot {s}: {int((d == 0).sum())} of {L} samples equal clamp(rint(32768 * y_float)), worst {int(d.max())} LSB")
            assert d.max() <= 1, (name, precision, way, s, int(d.max()))
            if precision == "f32":                                        # and the quantised float64 reference
                d64 = np.abs(q[s].numpy().astype(np.int64) - ref64[s].astype(np.int64))
                print(f"{name} {way} slot {s}: vs the quantised float64 reference: {int((d64 == 0).sum())} of {L} equal, worst {int(d64.max())} LSB")
                assert d64.max() <= 1, (name, way, s, int(d64.max()))


def test_formats_are_independent_and_graph_equals_eager():
    """float in / PCM out and PCM in / float out are legal; graph replay and eager launches give the same bits in every mode"""
    _, m, _, _ = setup("hg20_g1")
    v = torch.stack([IO.pcm_noise(L, 400 + s) for s in range(S)])
    x = v.float() / 32768.0
    y = drive(server(m), x, PUSH_PACKETS)
    f_in = drive(server(m, pcm_in=True), v, PUSH_PACKETS)                  # PCM in, float out: the float instance's bits
    p_out = drive(server(m, pcm_out=True), x, PUSH_PACKETS)                # float in, PCM out
    both = drive(server(m, pcm_in=True, pcm_out=True, atten_lim=True), v, PUSH_PACKETS)
    eager = drive(server(m, pcm_in=True, pcm_out=True, atten_lim=True, use_graph=False), v, PUSH_PACKETS)
    for s in range(S):
        assert f_in[s].dtype == torch.float32 and torch.equal(f_in[s], y[s])
        assert p_out[s].dtype == torch.int16 and torch.equal(p_out[s], both[s]) and torch.equal(both[s], eager[s])


# ---- 5. the clip counter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("way", ["pushes", "push+packets"])
def test_clip_counter(way):
    _, m, _, _ = setup("hg20_g1")
    g = torch.Generator().manual_seed(9)
    levels = torch.tensor([0.0, 0.5, -0.5, 4.0, -4.0, 0.0, 0.5, -0.5])     # a quarter of the samples are +-4
    x = levels[torch.randint(0, 8, (S, L), generator=g)]
    inf = server(m, atten_lim=True, pcm_out=True)
    inf.set_atten_lim(0.0)                                                 # passthrough: the output is the input, 20 ms late
    assert inf.clipped().tolist() == [0] * S and inf.clipped().dtype == np.int64
    # slot 1 is never active: its counter stays 0 and its rows are not written
    calls = [(k, [a if s != 1 else (False if k == "p" else 0) for s, a in enumerate(arg)]) for k, arg in WAYS[way]]
    seen = {}

    def after(i):                                                          # mid-clip: only what reached an output block is counted
        if i == 2:
            seen["n"] = inf.clipped().copy()

    q = drive(inf, x, calls, after=after)
    n = inf.clipped()
    big = x.abs() == 4.0
    print(f"{way}: clipped() {n.tolist()}, +-4 samples per clip {big.sum(1).tolist()}, after three calls {seen['n'].tolist()}")
    assert q[1].numel() == 0 and n[1] == 0
    out_blocks = {"pushes": {0: 2, 2: 2}, "push+packets": {0: 8, 2: 4}}[way]   # output blocks of slots 0 / 2 after the first three calls
    for s in (0, 2):
        assert q[s].dtype == torch.int16 and q[s].shape == (L,)
        assert n[s] == int(big[s].sum())
        assert seen["n"][s] == int(big[s, :160 * out_blocks[s]].sum()), (s, seen["n"][s])
        assert bool((q[s][x[s] == 4.0] == 32767).all()) and bool((q[s][x[s] == -4.0] == -32768).all())
        rest = ~big[s]
        assert int((q[s][rest].long() - (x[s][rest] * 32768).long()).abs().max()) <= 1
    assert inf.clipped([2, 0]).tolist() == [n[2], n[0]]
    assert inf.clipped([0], reset=True).tolist() == [n[0]]
    assert inf.clipped().tolist() == [0, 0, n[2]]
    assert inf.clipped(reset=True).tolist() == [0, 0, n[2]] and inf.clipped().tolist() == [0, 0, 0]


# ---- 6. bounds -----------------------------------------------------------------------------------------------------------------------------
def test_int16_buffers_and_counters_stay_inside_their_rows():
    """the int16 input / output tensors, the limits and the counters as views into larger buffers, 160 sentinel elements on each side"""
    _, m, _, _ = setup("hg20_g1")
    v = torch.stack([IO.pcm_noise(L, 500 + s) for s in range(S)])
    free_inf = server(m, atten_lim=True, pcm_in=True, pcm_out=True)
    free = drive(free_inf, v, PUSH_PACKETS)
    inf = server(m, atten_lim=True, pcm_in=True, pcm_out=True)
    G, guards = 160, {}

    def guarded(name, sentinel):
        t = getattr(inf, name)
        buf = torch.full((t.numel() + 2 * G,), sentinel, dtype=t.dtype, device="cuda")
        view = buf[G:G + t.numel()].view(t.shape)
        view.copy_(t)
        setattr(inf, name, view)
        guards[name] = (buf, sentinel, t.numel())

    for name in ("blocks", "out", "pblocks", "pout"):
        guarded(name, 12345)
    guarded("clip", 777)
    guarded("lim", 0.5)
    got = drive(inf, v, PUSH_PACKETS)                                      # a push, packets at max_hops (5 frames), short packets, flush
    torch.cuda.synchronize()
    for name, (buf, sentinel, n) in guards.items():
        assert bool((buf[:G] == sentinel).all()) and bool((buf[G + n:] == sentinel).all()), f"{name}: a sentinel was overwritten"
    for s in range(S):
        assert torch.equal(got[s], free[s])
    assert inf.clipped().tolist() == free_inf.clipped().tolist()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from cruse_amd import _lib, ops
    _, m, _, _ = setup("hg20_g1")
    pcm = server(m, pcm_in=True, pcm_out=True)
    for call, arg in ((pcm.push, torch.zeros(S, 160, device="cuda")), (pcm.push_packet, torch.zeros(S, 2, 160, device="cuda")),
                      (pcm.enhance, torch.zeros(S, 640)), (pcm.push, torch.zeros(S, 160, device="cuda", dtype=torch.int32))):
        with pytest.raises(ValueError, match=str(arg.dtype).replace(".", r"\.")):
            call(arg)
    assert list(pcm.nblk) == [0] * S and not pcm._graphs
    plain = server(m)
    with pytest.raises(ValueError, match="atten_lim=True"):
        plain.set_atten_lim(6.0)
    with pytest.raises(ValueError, match="pcm_out=True"):
        plain.clipped()
    lim = server(m, atten_lim=True)
    lim.set_atten_lim([3.0, 6.0, 9.0])
    before = lim.lim.clone()
    for bad in (-3.0, float("nan"), [6.0, -1.0, 6.0]):
        with pytest.raises(ValueError, match="non-negative"):
            lim.set_atten_lim(bad)
    with pytest.raises(ValueError, match="values for"):
        lim.set_atten_lim([6.0, 6.0], [0, 1, 2])
    with pytest.raises(ValueError, match="out of range"):
        lim.set_atten_lim(6.0, [S])
    assert torch.equal(lim.lim, before)
    # the C entry points: an unknown format, and a counter with float output
    lib, lay, play = _lib.lib, ops.stream_layout(m.ch), ops.stream_packet_layout(m.ch)
    z = lambda n, dt=torch.float32: torch.zeros(n, device="cuda", dtype=dt)
    ctl, tab, w = z(2 * S, torch.int32), ops.stream_tables("cuda"), z(lay["wtotal"])
    ctl[:S] = ops.STREAM_FRAME                                             # would compute if it were launched
    ctl[S:] = 1
    state, work, pwork = z(S * lay["st_stride"]), z(S * lay["wk_stride"]), z(S * (K + 1) * play["wk_stride"])
    io, cnt, gains = z(S * K * 160), z(S, torch.int32), z(S)
    p = lambda t: t.data_ptr()
    ch = [int(c) for c in m.ch]
    for fmt in (2, -1):
        assert lib.cruse_stream_encode_io(p(ctl), S, *ch, p(io), fmt, p(tab), p(w), p(state), p(work), None) != 0
        assert b"stream_encode_io: unknown sample format" in lib.cruse_last_error()
        assert lib.cruse_stream_decode_io(p(ctl), S, *ch, p(tab), p(w), 1e-5, p(state), p(work), p(io), fmt, p(gains), None, None) != 0
        assert b"stream_decode_io: unknown sample format" in lib.cruse_last_error()
        assert lib.cruse_stream_encode_n_io(p(ctl), S, K, K, K + 1, *ch, p(io), fmt, p(tab), p(w), p(state), p(pwork), None) != 0
        assert b"stream_encode_n_io: unknown sample format" in lib.cruse_last_error()
        assert lib.cruse_stream_decode_n_io(p(ctl), S, K, K, K + 1, *ch, p(tab), p(w), 1e-5, p(state), p(pwork), p(io), fmt, None, None, None) != 0
        assert b"stream_decode_n_io: unknown sample format" in lib.cruse_last_error()
    assert lib.cruse_stream_decode_io(p(ctl), S, *ch, p(tab), p(w), 1e-5, p(state), p(work), p(io), 0, None, p(cnt), None) != 0
    assert b"clip counter needs s16 output" in lib.cruse_last_error()
    assert lib.cruse_stream_decode_n_io(p(ctl), S, K, K, K + 1, *ch, p(tab), p(w), 1e-5, p(state), p(pwork), p(io), 0, None, p(cnt), None) != 0
    with pytest.raises(RuntimeError, match="int16"):
        ops.stream_encode(ctl[:S], m.ch, z(S * 160, torch.float16).view(S, 160), tab, w, state.view(S, -1), work.view(S, -1))
    torch.cuda.synchronize()
    for t in (state, work, pwork, io):
        assert float(t.abs().sum()) == 0.0                                 # nothing was launched
    assert int(cnt.sum()) == 0


# ---- 8. the offline Inferencer ----------------------------------------------------------------------------------------------------------------
# the offline path's GRU kernels need hidden_size / rnn_groups to be a multiple of 32, which the two-channel model (20) is not: the
# smallest model of the streaming tests that both paths accept stands in for it here
OFFLINE = {"small_g2": R.CONFIGS["small_g2"], "g4": R.CONFIGS["g4"]}


@pytest.mark.parametrize("name", list(OFFLINE))
def test_offline_inferencer_with_a_limit(name):
    from cruse_amd.inferencer import Inferencer
    if name in IO.MODELS:
        _, m, clips, e64 = setup(name)
    else:
        o, clips = R.oracle_model(OFFLINE[name]), IO.clips()
        m, e64 = R.gpu_model(o, OFFLINE[name]), [IO.e64(o, clips[s]) for s in range(S)]
    off = Inferencer(m, atten_lim_db=6).mag_mask_to_wave(clips.cuda()).cpu()
    assert torch.equal(Inferencer(m, atten_lim_db=None).mag_mask_to_wave(clips.cuda()), Inferencer(m).mag_mask_to_wave(clips.cuda()))
    inf = server(m, atten_lim=True)
    inf.set_atten_lim(6)
    got = inf.enhance(clips).cpu()
    for s in range(S):
        e_pair, e_ref = rel_l2(got[s], off[s]), rel_l2(off[s], IO.mix(clips[s], e64[s], IO.gain(6.0)))
        print(f"{name} clip {s}, 6 dB: enhance() vs Inferencer {e_pair:.2e}; Inferencer vs R {e_ref:.2e}")
        assert e_pair <= BAR and e_ref <= BAR, (name, s, e_pair, e_ref)
