"""MI355X: StreamingInferencer(head="df") -- the DeepFilter(1, 5) head at the end of every streaming chain (cruse_stream_df_head /
_df_head_n, csrc/stream.hip).

References: ops.df_head_apply on the stacked rows the chain itself leaves (bit for bit), the oracle's offline df waveform and
Inferencer(head="df") (2e-5 rel-L2, the bar tests/test_gpu_streaming.py holds the mask head to), and the float64 frame-by-frame
restatement tests/stream_df_ref.py (pinned to the offline waveform at 1e-9 by tests/test_stream_df_host.py).  Measured on MI355X
(the prints below): whole clips against the oracle 4.6e-7 .. 7.6e-7, against Inferencer(head="df") 4.5e-7 .. 7.4e-7; the df and the
mask stream of one model 1.45 .. 1.63 apart; limit 0 dB against the input 3.7e-7, 12 dB against the Inferencer 4.1e-7; f16 mode 1.70e-5
from float64 where the emulation is 1.70e-5; 64 slots 232 us per push."""
import functools
import time

import pytest
import torch

from oracle import cruse_oracle as O
from tests import stream_ref_f16 as R
from tests.stream_df_ref import df_stream, offline_df
from tests.test_gpu_stream_packets import even_sizes, run_packets
from tests.test_gpu_streaming import _chain, _serve, models, stream_all
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

CONFIGS = {"small_g2": dict(ch=(1, 4, 8, 16, 32), rnn_groups=2), "g4": dict(rnn_groups=4)}
LENGTHS = (320, 480, 1600)
S = 3


@functools.lru_cache(maxsize=None)
def pair(name):
    return models(CONFIGS[name])


@functools.lru_cache(maxsize=None)
def clips(L):
    return torch.cat([O.synth_pair(1, L, seed=300 + i)[0] for i in range(S)])


@functools.lru_cache(maxsize=None)
def refs(name, L):
    """(the oracle's offline df waveforms [S, L], its mask waveforms, Inferencer(head="df") on the GPU), computed once"""
    from cruse_amd.inferencer import Inferencer
    o, m = pair(name)
    x = clips(L)
    df = torch.stack([offline_df(o, x[i]) for i in range(S)])
    mk = torch.stack([offline_df(o, x[i], head="mask") for i in range(S)])
    return df, mk, Inferencer(m, head="df").mag_mask_to_wave(x.cuda()).cpu()


def inf_of(name, n=S, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    return StreamingInferencer(pair(name)[1], n, head="df", **kw)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the bit contract ------------------------------------------------------------------------------------------------------------
def _rows_of_stage(inf, frames=None):
    """(mask, re, im) of the frames slot 0's last call computed"""
    torch.cuda.synchronize()
    idx = [-1] if frames is None else range(frames)
    st = [inf.stage(0, f) if frames is not None else inf.stage(0) for f in idx]
    return [tuple(s[k].clone() for k in ("mask", "re", "im")) for s in st]


@pytest.mark.parametrize("sizes, max_hops", [(["p"] * 10, 1), (["p"] * 10, 4), ([1] * 10, 4), ([3, 3, 3, 1], 4), ([4, 4, 2], 4),
                                             (["p", 3, "p", 4, 1], 4)], ids=str)
def test_rows_have_the_bits_of_df_head_apply(sizes, max_hops):
    """max_hops = 1: pushes run the single-hop chain and cruse_stream_df_head; max_hops = 4: a push is a packet of one block and every call
    runs cruse_stream_df_head_n; flush runs the single-hop END chain and the drain step in both"""
    from cruse_amd import ops
    inf = inf_of("small_g2", 1, use_graph=False, max_hops=max_hops)
    x = clips(1600)[:1].view(1, 10, 160).cuda()
    rows, E, b = [], [], 0
    for c in sizes:
        if c == "p":
            inf.push(x[:, b])
            nfr = int(inf._last_frames[0])
            if nfr > 0:                                     # the push ran as a packet of one block
                rows += _rows_of_stage(inf, nfr)
            else:
                if b == 1:                                  # frames 0 and 1 in two chains: the work row shows frame 1, frame 0 is re-made below
                    rows.append(None)
                if b >= 1:
                    rows += _rows_of_stage(inf)
            b += 1
        else:
            inf.push_packet(x[:, b:b + c])
            rows += _rows_of_stage(inf, int(inf._last_frames[0]))
            b += c
        E.append(inf.stage_df(0).clone())
    if rows[0] is None:                                     # frame 0 alone: the same two chains on a fresh instance, stopped after the first
        other = inf_of("small_g2", 1, use_graph=False)
        other.blocks.copy_(x[:, 0])
        _chain(other, 1, [ops.STREAM_STORE])
        other.blocks.copy_(x[:, 1])
        st = _chain(other, 0, [ops.STREAM_FRAME0])[0]
        rows[0] = tuple(st[k].cuda() for k in ("mask", "re", "im"))
    inf.flush([0])
    torch.cuda.synchronize()
    rows += [tuple(inf.stage(0)[k].clone() for k in ("mask", "re", "im"))]
    E.append(inf.stage_df(0).clone())
    got = torch.cat(E)                                      # [T, 322]
    T = 11
    assert len(rows) == T and got.shape == (T, 322)
    mask = torch.stack([r[0] for r in rows]).view(1, T, 160)
    nre = torch.stack([r[1] for r in rows]).view(1, T, 161)
    nim = torch.stack([r[2] for r in rows]).view(1, T, 161)
    ere, eim = ops.df_head_apply(mask, nre, nim)
    want = torch.cat([ere[0], eim[0]], dim=1)
    differ = int((bits(got) != bits(want)).sum())
    print(f"{sizes} max_hops {max_hops}: {differ} of {want.numel()} words differ from ops.df_head_apply")
    assert differ == 0


# ---- 2. whole clips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_whole_clips_equal_offline(name, L):
    from cruse_amd.inferencer import StreamingInferencer
    x = clips(L)
    want, want_mask, want_gpu = refs(name, L)
    nb = L // 160
    inf = inf_of(name, max_hops=4)
    runs = {"push (single-hop chain)": stream_all(inf_of(name), x), "push": stream_all(inf, x)}
    for K in (1, 2, 3, 4):
        runs[f"packets of {K}"] = run_packets(inf, x, even_sizes(nb, K))
    for K in (None, 3):
        runs[f"enhance hops={K}"] = inf.enhance(x.cuda(), hops=K).cpu()
    plain = stream_all(StreamingInferencer(pair(name)[1], S), x)
    for tag, got in runs.items():
        assert got.shape == x.shape, tag
        for i in range(S):
            e_o, e_g, far = rel_l2(got[i], want[i]), rel_l2(got[i], want_gpu[i]), rel_l2(got[i], plain[i])
            print(f"{name} L {L} {tag} clip {i}: vs oracle df {e_o:.2e}, vs Inferencer(head=df) {e_g:.2e}, vs the mask stream {far:.2f}")
            assert e_o <= 2e-5 and e_g <= 2e-5, (tag, i, e_o, e_g)
            assert far > 1.0, (tag, i, far)                 # not the other head
    for tag, got in runs.items():                           # pushes, packets of any size and enhance on one instance: one set of bits
        assert tag == "push (single-hop chain)" or torch.equal(bits(got), bits(runs["push"])), tag
    assert rel_l2(plain, want_mask) <= 2e-5                 # head="mask" beside it still gives the mask waveform


def test_shortest_clip_no_push_is_valid_and_flush_returns_the_clip():
    inf = inf_of("small_g2")
    x = clips(320)
    for b in range(2):
        out, valid = inf.push(x[:, 160 * b:160 * (b + 1)].cuda())
        assert not valid.any()
    last = inf.flush([0, 1, 2]).cpu()
    assert last.shape == (S, 320)
    assert max(rel_l2(last[i], refs("small_g2", 320)[0][i]) for i in range(S)) <= 2e-5
    assert (inf.nblk == 0).all() and not inf.df_state.any()


SPLITS = [[1] * 10, [2] * 5, [1, 2, 3, 4], [4, 4, 2], [3, 4, 3]]


def test_packets_of_any_split_equal_one_another():
    """What the head adds to a chain is the same code for a push and for a packet (df_frames in csrc/stream.hip), so on equal rows it
    gives equal bits (test_rows_have_the_bits_of_df_head_apply), and every split of a clip into packets gives one waveform."""
    x = clips(1600)
    inf = inf_of("g4", max_hops=4)
    first = run_packets(inf, x, SPLITS[0])
    for sizes in SPLITS[1:]:
        assert torch.equal(bits(run_packets(inf, x, sizes)), bits(first)), sizes


def test_packets_of_any_split_equal_single_pushes():
    """On an instance built for packets (max_hops > 1) a push runs as a packet of one block, so pushes, packets of any split and any mix
    of the two give one set of bits.  The single-hop chain, which an instance with max_hops = 1 runs, is a different set of kernels in
    front of the head and rounds differently (as it does for head="mask", DESIGN 12a: the packet path sums W_ih x and W_hh h apart, and
    decode_n takes the LN2 statistics per wave where decode takes them per workgroup): at frame 2 of these clips re / im / e1 / e4 agree in
    every word, gru1 differs in 198 of 640 words, gru2 in 576, the mask in 99 of 160 (g4), and the waveforms of the two chains differ in
    4474 of 4800 words at 4.9e-7 rel-L2 (head="mask" on the same kernels: 4006 words, 2.2e-7).  That distance is printed and held to the
    2e-5 of the whole-clip tests."""
    x = clips(1600)
    inf = inf_of("g4", max_hops=4)
    want = stream_all(inf, x)
    diffs = {}
    for sizes in SPLITS + [[4, 1, "p", 2, 2], ["p", "p", 4, 3, 1]]:
        got = run_packets(inf, x, sizes)
        diffs[str(sizes)] = int((bits(got) != bits(want)).sum())
        print(f"packets {sizes}: {diffs[str(sizes)]} of {want.numel()} words differ from single pushes, rel-L2 {rel_l2(got, want):.2e}")
    assert not any(diffs.values()), diffs
    single = stream_all(inf_of("g4"), x)
    print(f"single-hop chain (max_hops = 1): {int((bits(single) != bits(want)).sum())} of {want.numel()} words differ from the packet chain, "
          f"rel-L2 {rel_l2(single, want):.2e}")
    assert rel_l2(single, want) <= 2e-5


def test_graph_replay_equals_eager_launches():
    x = clips(1600)
    g, e = inf_of("small_g2", max_hops=4), inf_of("small_g2", max_hops=4, use_graph=False)
    for run in (stream_all, lambda i, c: run_packets(i, c, [3, "p", 4, 2]), lambda i, c: i.enhance(c.cuda()).cpu()):
        a = run(g, x)
        assert torch.equal(bits(a), bits(run(e, x)))
        assert torch.equal(bits(a), bits(run(g, x)))        # the captured graphs, replayed
    g1, e1 = inf_of("small_g2"), inf_of("small_g2", use_graph=False)        # the single-hop chain, its flush and drain
    a = stream_all(g1, x)
    assert torch.equal(bits(a), bits(stream_all(e1, x))) and torch.equal(bits(a), bits(stream_all(g1, x)))


# ---- 3. slots -----------------------------------------------------------------------------------------------------------------------
def test_serving_staggered_inactive_reused_slots():
    o, _ = pair("small_g2")
    clip = lambda n, seed: O.synth_pair(1, 160 * n, seed=seed)[0].view(-1)
    A = {0: [(0, clip(12, 1), [])], 1: [(3, clip(9, 2), [])], 2: [(4, clip(8, 3), [6, 7, 9])],
         3: [(1, clip(5, 4), []), (8, clip(6, 5), [])], 4: [(2, clip(2, 6), []), (5, clip(10, 7), [8])]}
    inf = inf_of("small_g2", 5)
    res = _serve(inf, A, 18)
    for s, items in A.items():
        for k, (_, c, _) in enumerate(items):
            err = rel_l2(res[(s, k)], offline_df(o, c))
            print(f"slot {s} clip {k}: {err:.2e}")
            assert res[(s, k)].shape == c.shape and err <= 2e-5
    # a slot reused after flush gives the bits of a fresh instance; the other slots' schedules do not show
    B = {3: [(0, A[3][1][1], [])], 0: [(1, clip(11, 11), [5, 6])], 2: [(0, clip(4, 12), [])]}
    res_b = _serve(inf_of("small_g2", 5), B, 16)
    assert torch.equal(bits(res_b[(3, 0)]), bits(res[(3, 1)]))
    assert not inf.df_state.any()                           # every slot was flushed: reset with the rest of the slot
    # an inactive slot's state row is untouched by a push of the others, a reset slot's is zero
    x = clips(1600)[:, :640].cuda()
    for b in range(3):
        inf.push(torch.cat([x[:, 160 * b:160 * (b + 1)], x[:2, 160 * b:160 * (b + 1)]]))
    before = inf.df_state.clone()
    assert before[1].any()
    inf.push(torch.zeros(5, 160, device="cuda"), [True, False, True, False, False])
    assert torch.equal(bits(inf.df_state[[1, 3, 4]]), bits(before[[1, 3, 4]])) and not torch.equal(inf.df_state[0], before[0])
    inf.reset([1])
    assert not inf.df_state[1].any() and torch.equal(bits(inf.df_state[3]), bits(before[3]))


# ---- 4. attenuation limit, PCM out, f16 -----------------------------------------------------------------------------------------------
def test_attenuation_limit():
    from cruse_amd.inferencer import Inferencer
    x = clips(1600)
    nolim = stream_all(inf_of("g4"), x)
    inf = inf_of("g4", atten_lim=True)
    inf.set_atten_lim(0)
    thru = stream_all(inf, x)
    print(f"limit 0 dB vs the input: {rel_l2(thru, x):.2e}")
    assert rel_l2(thru, x) <= 1e-5
    # ... delayed by 480 samples: the push of block b (its last sample is 160 b + 159) returns block b - 2 (first sample 160 b - 320)
    blocks = x.view(S, 10, 160).cuda()
    for b in range(10):
        out, valid = inf.push(blocks[:, b])
        assert bool(valid.all()) == (b >= 2)
        if b >= 2:
            assert rel_l2(out.cpu(), blocks[:, b - 2].cpu()) <= 1e-5
    inf.reset()
    inf.set_atten_lim(None)
    assert torch.equal(bits(stream_all(inf, x)), bits(nolim))
    inf.set_atten_lim(12.0)
    want = Inferencer(pair("g4")[1], head="df", atten_lim_db=12.0).mag_mask_to_wave(x.cuda()).cpu()
    err = rel_l2(stream_all(inf, x), want)
    print(f"limit 12 dB vs Inferencer(head=df, atten_lim_db=12): {err:.2e}")
    assert err <= 2e-5
    pk = inf_of("g4", atten_lim=True, max_hops=4)
    # limits at their default: the bits of an instance without them
    assert torch.equal(bits(run_packets(pk, x, [4, 4, 2])), bits(run_packets(inf_of("g4", max_hops=4), x, [4, 4, 2])))
    pk.set_atten_lim(12.0)
    assert rel_l2(run_packets(pk, x, [4, 3, 3]), want) <= 2e-5


def _pcm(y):
    return torch.clamp(torch.round(y * 32768.0), -32768, 32767).to(torch.int16)


@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_pcm_out_and_the_clip_counter(scale):
    """scale 40: the clip overflows.  clipped() counts exactly the clamped samples of the returned blocks; E[0]'s block, in front of the
    clip, is not among them (its samples clamp too at this scale)."""
    x = clips(1600) * scale
    y = stream_all(inf_of("small_g2"), x)                   # the float stream
    want = _pcm(y)
    r = torch.round(y * 32768.0)
    n_clamped = ((r > 32767) | (r < -32768)).sum(dim=1)
    inf = inf_of("small_g2", pcm_out=True)
    got = stream_all(inf, x)
    assert got.dtype == torch.int16 and torch.equal(got, want)
    counts = inf.clipped(reset=True)
    print(f"scale {scale}: clamped samples per slot {counts.tolist()}, expected {n_clamped.tolist()}")
    assert counts.tolist() == n_clamped.tolist() and (scale == 1.0 or min(counts) > 0)
    yp = run_packets(inf_of("small_g2", max_hops=4), x, [3, 4, 3])      # the packet chain's float stream (its own rounding)
    rp = torch.round(yp * 32768.0)
    pk = inf_of("small_g2", pcm_out=True, max_hops=4)
    assert torch.equal(run_packets(pk, x, [3, 4, 3]), _pcm(yp))
    assert pk.clipped().tolist() == ((rp > 32767) | (rp < -32768)).sum(dim=1).tolist()


def test_f16_mode_against_the_float64_restatement():
    cfg = R.CONFIGS["small_g2"]
    o = R.oracle_model(cfg)
    m = R.gpu_model(o, cfg)
    x = R.clip(10, R.ACC_SEED)
    _, frames64, _, frames16, _ = R.references(o, x)
    ref = df_stream(frames64)[0]
    emu = df_stream([{k: f[k].double() for k in ("mask", "re", "im")} for f in frames16])[0]
    e_emu = R.rel(emu, ref)
    from cruse_amd.inferencer import StreamingInferencer
    for tag, run, K in (("push", stream_all, 1), ("packets", lambda i, c: run_packets(i, c, [4, 3, 3]), 4)):
        got = run(StreamingInferencer(m, 1, head="df", precision="f16", max_hops=K), x.view(1, -1))[0]
        err = R.rel(got, ref)
        print(f"f16 {tag}: whole clip vs float64 {err:.2e}; emulation vs float64 {e_emu:.2e}; ratio {err / e_emu:.2f}")
        assert err <= 2 * e_emu and err > 4e-7
    f32 = stream_all(StreamingInferencer(m, 1, head="df"), x.view(1, -1))[0]
    assert R.rel(f32, ref) <= 2e-5


# ---- 5. poison ----------------------------------------------------------------------------------------------------------------------
def test_poisoned_outputs_are_written_where_a_block_is_returned_and_nowhere_else():
    nan = float("nan")
    x = clips(1600).cuda()
    x = torch.cat([x, x[:1]])

    def poison():
        for name in ("out", "out_drain", "pout", "df_work", "df_pwork"):
            if hasattr(inf, name):
                getattr(inf, name).fill_(nan)

    # the single-hop chain (max_hops = 1): slot 3 stays inactive (SKIP); block 0 is STORE, block 1 is FRAME0 + FRAME (E[0]: a row, no block)
    inf = inf_of("small_g2", 4, use_graph=False)
    for b in range(4):
        poison()
        out, valid = inf.push(x[:, 160 * b:160 * (b + 1)], [True, True, True, False])
        torch.cuda.synchronize()
        assert torch.isnan(inf.out[3]).all() and torch.isnan(inf.df_work[3]).all()
        assert torch.isnan(inf.out_drain).all() and torch.isnan(inf.df_work[:, 1]).all()
        if b == 0:
            assert not valid.any() and torch.isnan(inf.out).all() and torch.isnan(inf.df_work).all()
        elif b == 1:
            assert not valid.any() and torch.isnan(inf.out).all() and not torch.isnan(inf.df_work[:3, 0]).any()
        else:
            assert valid.tolist() == [True, True, True, False]
            assert not torch.isnan(inf.out[:3]).any() and not torch.isnan(inf.df_work[:3, 0]).any()
    # packets (max_hops = 4): slots 0..2 hold four blocks; then slot 0 takes 4 more, slot 1 two, slot 2 none, slot 3 (fresh) three: frames
    # 0..2, one block
    inf = inf_of("small_g2", 4, max_hops=4, use_graph=False)
    inf.push_packet(x[:, :640].reshape(4, 4, 160), [4, 4, 4, 0])
    poison()
    pkt = x[:, 640:1280].reshape(4, 4, 160)
    out, n_out = inf.push_packet(pkt, [4, 2, 0, 3])
    torch.cuda.synchronize()
    assert n_out.tolist() == [4, 2, 0, 1]
    for s, (n, rows) in enumerate([(4, 4), (2, 2), (0, 0), (1, 2)]):
        assert not torch.isnan(inf.pout[s, :n]).any() and torch.isnan(inf.pout[s, n:]).all(), s
        assert not torch.isnan(inf.df_pwork[s, :rows]).any() and torch.isnan(inf.df_pwork[s, rows:]).all(), s
        assert n == 0 or inf.stage_df(s).shape == (rows, 322)                   # (an inactive slot keeps showing its last call)
    assert torch.isnan(inf.out).all() and torch.isnan(inf.out_drain).all() and torch.isnan(inf.df_work).all()
    # flush of slots 0 and 3: both blocks and both rows written, the other slots' untouched
    poison()
    last = inf.flush([0, 3])
    torch.cuda.synchronize()
    assert last.shape == (2, 320) and not torch.isnan(last).any()
    assert not torch.isnan(inf.df_work[[0, 3]]).any() and torch.isnan(inf.df_work[[1, 2]]).all()
    assert torch.isnan(inf.out[[1, 2]]).all() and torch.isnan(inf.out_drain[[1, 2]]).all()
    assert not torch.isnan(inf.df_state).any()


# ---- 6. rejections --------------------------------------------------------------------------------------------------------------------
def test_rejections_come_before_any_launch():
    import ctypes
    from cruse_amd import ops
    from cruse_amd._lib import lib
    from cruse_amd.inferencer import StreamingInferencer
    _, m = pair("small_g2")
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="head"):
        StreamingInferencer(m, 2, head="dfn")
    with pytest.raises(ValueError, match="df_dims"):
        StreamingInferencer(m, 2, head="df", df_dims=(2, 5))
    with pytest.raises(ValueError, match="df_dims"):
        StreamingInferencer(m, 2, df_dims=(1, 3))
    with pytest.raises(ValueError, match="io_rate"):
        StreamingInferencer(m, 2, head="df", io_rate=48000)
    assert torch.cuda.memory_allocated() == mem             # nothing was allocated
    with pytest.raises(ValueError, match="head=\"mask\""):
        StreamingInferencer(m, 2).stage_df(0)
    inf = inf_of("small_g2", 2, max_hops=4)
    inf.push(torch.zeros(2, 160, device="cuda"))
    with pytest.raises(ValueError, match="at least 2"):
        inf.flush([0])
    # the entry points: every refusal is a return code with a message, the poisoned outputs stay as they were
    lay, play, D = inf.lay, inf.play, ops.stream_df_layout()
    nan = float("nan")
    out, dfw, pout, dfpw = (torch.full(s, nan, device="cuda") for s in ((2, 160), (2, 322), (2, 4, 160), (2, 4, 322)))
    state = torch.full((2, D["stride"]), nan, device="cuda")
    mode = torch.full((2,), ops.STREAM_FRAME, device="cuda", dtype=torch.int32)
    pk = torch.tensor([[2, 2], [4, 4]], device="cuda", dtype=torch.int32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    WS, PS = lay["wk_stride"], play["wk_stride"]

    def single(**kw):
        a = dict(mode=p(mode), S=2, drain=0, work=p(inf.work), ws=WS, re=lay["wk_re"], im=lay["wk_im"], mask=lay["wk_mask"], tab=p(inf.tab),
                 st=p(state), ss=D["stride"], dfw=p(dfw), dws=322, out=p(out), fmt=0, lim=None, clip=None, td=1, fd=5)
        a.update(kw)
        return lib.cruse_stream_df_head(*a.values(), None)

    def packet(**kw):
        a = dict(pk=p(pk), S=2, hops=4, oh=4, nfw=5, work=p(inf.pwork), ws=PS, re=lay["wk_re"], im=lay["wk_im"], mask=lay["wk_mask"],
                 tab=p(inf.tab), st=p(state), ss=D["stride"], dfw=p(dfpw), dwf=4, out=p(pout), fmt=0, lim=None, clip=None, td=1, fd=5)
        a.update(kw)
        return lib.cruse_stream_df_head_n(*a.values(), None)

    cnt = torch.zeros(2, device="cuda", dtype=torch.int32)
    for fn, who, stride in ((single, b"stream_df_head:", WS), (packet, b"stream_df_head_n:", PS)):
        bad = [dict(td=2), dict(fd=4), dict(td=2, fd=5), dict(S=0), dict(work=None), dict(tab=None), dict(st=None), dict(dfw=None),
               dict(out=None), dict(re=-1), dict(re=stride - 160), dict(im=stride), dict(mask=stride - 159), dict(ws=481),
               dict(ss=D["stride"] - 1), dict(fmt=2), dict(clip=p(cnt))]
        for kw in bad:
            assert fn(**kw) != 0, (who, kw)
            assert who in lib.cruse_last_error(), (who, kw, lib.cruse_last_error())
        assert fn(td=2, fd=5) != 0 and b"only the DeepFilter(1, 5) instance is built" in lib.cruse_last_error()
    assert single(mode=None) != 0 and single(dws=321) != 0 and packet(pk=None) != 0
    for kw in (dict(hops=0), dict(hops=48, nfw=49, oh=48, dwf=48), dict(nfw=4), dict(oh=3), dict(dwf=3)):
        assert packet(**kw) != 0 and b"stream_df_head_n: hops" in lib.cruse_last_error(), kw
    torch.cuda.synchronize()
    for t in (out, dfw, pout, dfpw, state):
        assert torch.isnan(t).all()
    state.zero_()
    assert single() == 0 and packet() == 0                  # and the arguments the refusals were derived from are accepted
    with pytest.raises(RuntimeError, match="only the DeepFilter"):
        ops.stream_df_head(mode, inf.work, lay, inf.tab, state, dfw, out, df_dims=(2, 5))
    with pytest.raises(RuntimeError, match="only the DeepFilter"):
        ops.stream_df_head_n(pk, 4, inf.pwork, lay, inf.tab, state, dfpw, pout, df_dims=(2, 5))


# ---- 7. real time -------------------------------------------------------------------------------------------------------------------
def test_real_time_bound_64_slots():
    inf = inf_of("g4", 64)
    blocks = 0.1 * torch.randn(64, 160, device="cuda")
    for _ in range(20):
        inf.push(blocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(400):
        inf.push(blocks)
    torch.cuda.synchronize()
    mean = (time.perf_counter() - t0) / 400
    print(f"64 slots, head=df: mean push wall {mean * 1e6:.1f} us (RTF {mean / 0.01:.4f})")
    assert mean < 0.010
