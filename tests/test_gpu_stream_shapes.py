"""MI355X: the streaming kernels (cruse_stream_*) at the GRU widths, slot tilings and channel counts the other streaming modules
do not reach, against the per-frame restatement in FLOAT64 (tests/stream_ref.py, pinned at these shapes by tests/test_stream_host.py).

tests/stream_shapes.py is the matrix: every register tiling KQ = 3 / 5 / 10 / 16 of the three GRU kernels at a width that leaves a
64-lane slice partly masked and at its upper edge, Hg < 64, odd channel counts, the widest rows the layout accepts, packets at
exactly the LDS bound.  The tiling tests serve 8 / 9 / 17 slots and enough slots that the GRU grids stride over their tiles, every
slot with its own clip on a ragged schedule, and compare EVERY slot.  Bars are the project's: 1e-5 rel-L2 per stage, 2e-5 per clip."""
import pytest
import torch

from oracle import cruse_oracle as O
from tests.stream_ref import as_double, stream_clip
from tests.stream_shapes import SHAPES, geometry, gru_grids, kq_of
from tests.test_gpu_stream_packets import _serve_packets, run_packets
from tests.test_gpu_streaming import _chain, _check, _serve, models, offline, stage_errors, stream_all
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

NB = 12                                                                    # blocks of the per-model clip: frames 0..12
F64 = torch.float64


def test_matrix_covers_every_gru_instantiation():
    """a later change of the dispatch thresholds (or of the matrix) cannot silently drop an instantiation"""
    assert {kq_of(geometry(c)[3]) for c in SHAPES.values()} == {3, 5, 10, 16}


def _packet_bound(ch):
    from cruse_amd import ops
    return ops.stream_packet_layout(ch)["max_hops"]


def _single_hop_frames(m, x):
    """the clip through the single-hop chain, eager: [(stages, output block, frame index)] of frames 0..NB"""
    from cruse_amd import ops
    from cruse_amd.inferencer import StreamingInferencer
    inf = StreamingInferencer(m, 1, use_graph=False)
    blocks = x.view(NB, 160).cuda()
    res = []
    inf.blocks.copy_(blocks[0:1])
    _chain(inf, 1, [ops.STREAM_STORE])
    inf.blocks.copy_(blocks[1:2])
    st, out, _ = _chain(inf, 0, [ops.STREAM_FRAME0])
    res.append((st, out, 0))
    st, out, _ = _chain(inf, 1, [ops.STREAM_FRAME])
    res.append((st, out, 1))
    for b in range(2, NB):
        inf.blocks.copy_(blocks[b:b + 1])
        st, out, _ = _chain(inf, 1, [ops.STREAM_FRAME])
        res.append((st, out, b))
    st, out, _ = _chain(inf, 1, [ops.STREAM_END])
    res.append((st, out, NB))
    return res


def _packet_frames(m, x, max_hops, sizes):
    """the clip through push_packet calls of the given sizes ("p": a single push), eager: [(stages, output block, frame index)] of
    every frame computed inside a packet, then of the end frame; and the largest number of frames one packet computed.  "p" may
    only come first."""
    from cruse_amd import ops
    from cruse_amd.inferencer import StreamingInferencer
    inf = StreamingInferencer(m, 1, use_graph=False, max_hops=max_hops)
    blocks = x.view(1, NB, 160).cuda()
    res, b, t, most = [], 0, 0, 0
    for c in sizes:
        if c == "p":                                                        # block 0 of the clip: stored, no frame
            assert b == 0
            _, valid = inf.push(blocks[:, 0])
            assert not bool(valid[0])
            b = 1
            continue
        _, n_out = inf.push_packet(blocks[:, b:b + c])
        torch.cuda.synchronize()
        b += c
        nfr = int(inf._last_frames[0])
        most = max(most, nfr)
        for f in range(nfr):
            st = {k: v.cpu().clone() for k, v in inf.stage(0, f).items()}
            assert ("block" in st) == (t >= 1)
            res.append((st, st.get("block"), t))
            t += 1
    assert b == NB and t == NB, (b, t)
    inf._last_frames[:] = 0                                                 # stage(0): the single-hop work row again
    st, out, _ = _chain(inf, 1, [ops.STREAM_END])                           # the end frame on the state the packets left
    res.append((st, out, NB))
    return res, most


def _alternating(first, second):
    """[first, second, first, ...] summing to NB, the last entry trimmed"""
    sizes, left = [], NB
    while left:
        for c in (first, second):
            c = min(c, left)
            if c:
                sizes.append(c)
                left -= c
    return sizes


def _report_and_check(name, what, got, frames):
    """print the worst stage error of the walk (before anything is asserted), then hold every frame to _check's 1e-5"""
    worst = (0.0, None, None)
    for st, out, t in got:
        for k, e in stage_errors(st, out, frames[t], t).items():
            if e > worst[0]:
                worst = (e, k, t)
    print(f"{name} {what}: {len(got)} frames, worst stage error {worst[0]:.2e} ({worst[1]}, frame {worst[2]})")
    for st, out, t in got:
        _check(st, out, frames[t], t)
    return worst[0]


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_stage_and_whole_clip(name):
    from cruse_amd.inferencer import StreamingInferencer
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    o, m = models(cfg)
    assert (m.hidden_size, m.rnn_groups) == (H, g)
    x = O.synth_pair(1, 160 * NB, seed=7)[0].view(-1)
    ref, frames = stream_clip(as_double(o), x, dtype=F64)
    off = offline(o, x)
    bound = _packet_bound(ch)
    print(f"{name}: ch {ch} g {g} H {H} Hg {Hg} KQ {kq_of(Hg)} packet bound {bound}")

    # every stage of every frame 0 .. NB (frame 0, frame 1, mid frames, the end frame), single-hop chain
    got = _single_hop_frames(m, x)
    assert [t for _, _, t in got] == list(range(NB + 1))
    _report_and_check(name, "single-hop chain", got, frames)

    # the same inside packets, where the channel counts admit them
    if bound >= 2:
        K = min(bound, 4)
        got, most = _packet_frames(m, x, K, [K] * (NB // K) + ([NB % K] if NB % K else []))
        assert sorted(t for _, _, t in got) == list(range(NB + 1)) and most == K
        _report_and_check(name, f"packets of {K}", got, frames)
        # a packet that arrives when the slot holds one block computes K + 1 frames: every work row of the slot is in use
        got, most = _packet_frames(m, x, K, ["p"] + _fit(_alternating(K, 1), NB - 1))
        assert most == K + 1
        _report_and_check(name, f"a push, then packets of {K} and 1", got, frames)
    else:
        with pytest.raises(ValueError, match="max_hops must be in"):
            StreamingInferencer(m, 1, max_hops=2)
        print(f"{name}: packets are refused (bound {bound}): asserted")

    # whole clip: pushes (graph replay), then packets, against the f64 restatement and the oracle's offline waveform
    runs = [("pushes", stream_all(StreamingInferencer(m, 1), x.view(1, -1))[0])]
    if bound >= 2:
        K = min(bound, 4)
        runs.append((f"packets of {K}", run_packets(StreamingInferencer(m, 1, max_hops=K), x.view(1, -1), _alternating(K, K))[0]))
    for what, y in runs:
        e_r, e_o = rel_l2(y, ref), rel_l2(y, off)
        print(f"{name} whole clip, {what}: vs f64 restatement {e_r:.2e}, vs offline {e_o:.2e}")
    for what, y in runs:
        assert y.shape == x.shape
        assert rel_l2(y, ref) <= 2e-5 and rel_l2(y, off) <= 2e-5, (name, what)


def _fit(sizes, total):
    """the leading part of `sizes` that sums to `total`, the last entry trimmed"""
    out, left = [], total
    for c in sizes:
        c = min(c, left)
        if c:
            out.append(c)
            left -= c
    assert left == 0
    return out


def test_packets_at_exactly_the_lds_bound():
    """max_hops == stream_packet_layout(ch)["max_hops"], read from the library: the LDS budget is full.  Counts [bound, 1, bound, ...];
    and behind a single push [bound, 1, ...] again, where the first packet computes bound + 1 frames = work_frames."""
    from cruse_amd.inferencer import StreamingInferencer
    name = "hg400_bound"
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    bound = _packet_bound(ch)
    assert 2 <= bound <= 4, bound                                           # small, so that `bound` blocks per call are a short clip
    o, m = models(cfg)
    x = O.synth_pair(1, 160 * NB, seed=8)[0].view(-1)
    ref, frames = stream_clip(as_double(o), x, dtype=F64)
    print(f"{name}: ch {ch} Hg {Hg} KQ {kq_of(Hg)} packets at max_hops = bound = {bound}")
    got, most = _packet_frames(m, x, bound, _alternating(bound, 1))
    assert most == bound
    _report_and_check(name, f"counts [{bound}, 1, ...]", got, frames)
    got, most = _packet_frames(m, x, bound, ["p"] + _fit(_alternating(bound, 1), NB - 1))
    assert most == bound + 1                                                # work_frames = bound + 1 really occurs
    _report_and_check(name, f"a push, then counts [{bound}, 1, ...]", got, frames)
    y = run_packets(StreamingInferencer(m, 1, max_hops=bound), x.view(1, -1), _alternating(bound, 1))[0]    # graph replay
    e_r, e_o = rel_l2(y, ref), rel_l2(y, offline(o, x))
    print(f"{name} whole clip at the bound: vs f64 restatement {e_r:.2e}, vs offline {e_o:.2e}")
    assert e_r <= 2e-5 and e_o <= 2e-5
    with pytest.raises(ValueError, match=rf"\[1, {bound}\]"):
        StreamingInferencer(m, 1, max_hops=bound + 1)


# ---- slot tilings -----------------------------------------------------------------------------------------------------------
# The GRU kernels walk tiles of 8 slots (the packet projection: 8 (slot, frame) rows, hops + 1 rows per slot, so its tiles straddle
# slots unless hops + 1 divides 8) on grid_x = min(ntiles, ceil(2048 / (H/4))) workgroup columns with a stride loop t += gridDim.x.
#   hg1020: H/4 = 255 units, ceil(2048 / 255) = 9 columns; S = 75 is 10 tiles (9 full + 3 slots): the loop iterates, last tile partial
#   hg660:  H/4 = 165 units, ceil(2048 / 165) = 13 columns; S = 107 is 14 tiles (13 full + 3 slots); hg1020 admits no packets
TILINGS = [("hg100_odd", 8, 2, False), ("hg100_odd", 9, 4, False), ("hg100_odd", 17, 4, False), ("hg1020", 75, 0, True),
           ("hg660", 107, 4, True)]


def _clip(nb, seed):
    return O.synth_pair(1, 160 * nb, seed=seed)[0].view(-1)


def _references(o, clips):
    od = as_double(o)
    return {s: stream_clip(od, c, dtype=F64)[0] for s, c in clips.items()}


def _compare_all(tag, S, res, clips, refs):
    compared, worst = set(), (0.0, None)
    for s in range(S):
        y = res[(s, 0)]
        assert y.shape == clips[s].shape, (tag, s)
        e = rel_l2(y, refs[s])
        if e > worst[0]:
            worst = (e, s)
        compared.add(s)
    print(f"{tag}: {len(compared)} slots compared, worst whole-clip error {worst[0]:.2e} (slot {worst[1]})")
    bad = [(s, rel_l2(res[(s, 0)], refs[s])) for s in range(S) if rel_l2(res[(s, 0)], refs[s]) > 2e-5]
    assert not bad, (tag, bad[:8])
    assert len(compared) == S                                               # no slot is left uncompared
    return compared


@pytest.mark.parametrize("name,S,K,strides", TILINGS, ids=[f"{n}-S{s}-K{k}" for n, s, k, _ in TILINGS])
def test_slot_tilings_every_slot_compared(name, S, K, strides):
    from cruse_amd.inferencer import StreamingInferencer
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    o, m = models(cfg)
    grids = gru_grids(S, H, K)
    print(f"{name} S {S} K {K}: H {H} Hg {Hg} KQ {kq_of(Hg)}; (ntiles, grid_x) " + ", ".join(f"{k} {v}" for k, v in grids.items()))
    if strides:
        assert all(nt > gx for nt, gx in grids.values()) and S % 8, grids   # the stride loop iterates; the last tile is partial
    else:
        assert all(nt == gx for nt, gx in grids.values())
    if K and S >= 9:
        assert 8 % (K + 1) and (S * (K + 1)) % 8                            # projection tiles straddle slots, the last one partial
    # 8..12 blocks per clip; 4..7 where the stride loop needs 75 / 107 slots (the float64 restatement of every slot is the module's time)
    clips = {s: _clip(4 + s % 4 if strides else 8 + s % 5, 1000 + s) for s in range(S)}
    refs = _references(o, clips)
    probe = S // 2 + 1                                                       # a slot in the middle of a tile, for the bit-identity below

    # single-hop chain: staggered starts, inactive pushes
    plan = {s: [(s % 4, clips[s], [s % 4 + 2 + s % 3] if s % 2 else [])] for s in range(S)}
    res = _serve(StreamingInferencer(m, S), plan, 20)
    _compare_all(f"{name} S {S} pushes", S, res, clips, refs)
    alone = _serve(StreamingInferencer(m, 1), {0: plan[probe]}, 20)
    assert torch.equal(alone[(0, 0)], res[(probe, 0)]), "a slot's output depends on its neighbours (pushes)"

    # packets: staggered starts, a random count in [0, K] per slot and call
    if K:
        assert K <= _packet_bound(ch)
        plan = {s: [(s % 4, clips[s])] for s in range(S)}
        res = _serve_packets(StreamingInferencer(m, S, max_hops=K), plan, 60, K, seed=5)
        _compare_all(f"{name} S {S} packets of up to {K}", S, res, clips, refs)
        # _serve_packets seeds a clip's counts with seed + 100 * slot: the same packetisation in slot 0 of a one-slot server
        alone = _serve_packets(StreamingInferencer(m, 1, max_hops=K), {0: plan[probe]}, 60, K, seed=5 + 100 * probe)
        assert torch.equal(alone[(0, 0)], res[(probe, 0)]), "a slot's output depends on its neighbours (packets)"


# ---- rejections ---------------------------------------------------------------------------------------------------------------
def test_group_width_above_1024_is_refused_at_construction():
    """unet_2(ch=(1,16,32,64,128), rnn_groups=1): Hg = 1280 passes cruse_stream_layout (rows of 1280 floats) and was refused only by
    cruse_stream_gru on the first push, inside graph capture and after the slot's block counter had advanced."""
    from cruse_amd.inferencer import StreamingInferencer
    from cruse_amd.model.cruse_net import unet_2
    wide = unet_2(ch=(1, 16, 32, 64, 128), rnn_groups=1, precision="f32").cuda().eval()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=r"hidden 1280, groups 1.*1024|1024.*hidden 1280, groups 1"):
        StreamingInferencer(wide, 2)
    with pytest.raises(ValueError, match="1024"):
        StreamingInferencer(wide, 2, use_graph=False, max_hops=2)
    assert torch.cuda.memory_allocated() == before                          # refused before any buffer exists
    # a valid inferencer built afterwards in the same process works
    o, m = models(SHAPES["hg100_odd"])
    x = _clip(10, 3)
    y = stream_all(StreamingInferencer(m, 1), x.view(1, -1))[0]
    err = rel_l2(y, stream_clip(as_double(o), x, dtype=F64)[0])
    print(f"a valid inferencer after the refusal: {err:.2e}")
    assert err <= 2e-5


def test_rows_and_channels_beyond_the_layout_are_refused_at_construction():
    from cruse_amd.inferencer import StreamingInferencer
    from cruse_amd.model.cruse_net import unet_2
    rows = unet_2(ch=(1, 26, 8, 16, 32), rnn_groups=2, precision="f32").cuda().eval()          # 26 * 80 = 2080 floats
    with pytest.raises(RuntimeError, match="row of 2080 floats exceeds 2048"):
        StreamingInferencer(rows, 1)
    chans = unet_2(ch=(1, 4, 8, 16, 516), rnn_groups=6, precision="f32").cuda().eval()         # Hg = 860: only ch[4] > 512 is wrong
    with pytest.raises(RuntimeError, match=r"ch\[4\] = 516 out of range"):
        StreamingInferencer(chans, 1)
    _, m = models(SHAPES["hg20_g1"])
    StreamingInferencer(m, 1).push(torch.zeros(1, 160, device="cuda"))      # and the process goes on
