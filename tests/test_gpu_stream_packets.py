"""MI355X: streaming inference in packets (StreamingInferencer.push_packet / enhance, cruse_stream_*_n kernels).

Packets of 2..8 hops against the oracle's offline waveform and the GPU Inferencer, independence of the packetisation, every stage
of every frame inside a packet against the per-frame CPU restatement (tests/stream_ref.py), ragged multi-slot serving, the state
shared with push, graph replay vs eager launches, enhance() on long clips in bounded memory, the rejections, and the real-time
bounds."""
import time

import numpy as np
import pytest
import torch

from oracle import cruse_oracle as O
from tests.stream_ref import stream_clip
from tests.test_gpu_streaming import CONFIGS, IDS, _check, models, offline, stream_all
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


def run_packets(inf, clips, sizes):
    """clips [n, L] (one per slot, L a multiple of 160) through calls of the given sizes: an int c is a push_packet of c blocks
    for every slot, the string "p" a single push; then flush.  -> [n, L] on the host"""
    n, L = clips.shape
    nb = L // 160
    blocks = clips.view(n, nb, 160).cuda()
    outs = [[] for _ in range(n)]
    b = 0
    for c in sizes:
        if c == "p":
            out, valid = inf.push(blocks[:, b])
            n_out = valid.to(torch.int64)
            out = out.unsqueeze(1)
            b += 1
        else:
            out, n_out = inf.push_packet(blocks[:, b:b + c])
            b += c
        out = out.cpu()
        for s in range(n):
            outs[s] += [out[s, k] for k in range(int(n_out[s]))]
    assert b == nb
    last = inf.flush(list(range(n))).cpu()
    return torch.stack([torch.cat(outs[s] + [last[s]]) for s in range(n)])


def even_sizes(nb, K):
    return [K] * (nb // K) + ([nb % K] if nb % K else [])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_packets_equal_offline(cfg):
    from cruse_amd.inferencer import Inferencer, StreamingInferencer
    o, m = models(cfg)
    clips = torch.cat([O.synth_pair(1, 32000, seed=100 + i)[0] for i in range(3)])
    ref_gpu = Inferencer(m).mag_mask_to_wave(clips.cuda()).cpu()
    ref_o = [offline(o, clips[i]) for i in range(3)]
    inf = StreamingInferencer(m, 3, max_hops=8)
    for K in (2, 3, 4, 8):
        if K == 3:      # 200 blocks: 66 packets of 3 and a short one of 2 that goes through counts
            n, L = clips.shape
            blocks = clips.view(n, 200, 160).cuda()
            outs = [[] for _ in range(n)]
            for b0 in range(0, 200, 3):
                c = min(3, 200 - b0)
                pkt = torch.zeros(n, 3, 160, device="cuda")
                pkt[:, :c] = blocks[:, b0:b0 + c]
                out, n_out = inf.push_packet(pkt, [c] * n)
                for s in range(n):
                    outs[s] += [out[s, k].cpu() for k in range(int(n_out[s]))]
            last = inf.flush([0, 1, 2]).cpu()
            got = torch.stack([torch.cat(outs[s] + [last[s]]) for s in range(n)])
        else:
            got = run_packets(inf, clips, even_sizes(200, K))
        for i in range(3):
            e_o, e_g = rel_l2(got[i], ref_o[i]), rel_l2(got[i], ref_gpu[i])
            print(f"{cfg} K={K} clip {i}: packets vs oracle {e_o:.2e}, vs GPU Inferencer {e_g:.2e}")
            assert got[i].shape == clips[i].shape
            assert e_o <= 2e-5 and e_g <= 2e-5


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_packetisation_does_not_matter(cfg):
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(cfg)
    clip = O.synth_pair(1, 160 * 90, seed=21)[0]
    inf = StreamingInferencer(m, 1, max_hops=8)
    a = stream_all(inf, clip)                                              # K = 1 pushes
    b = run_packets(inf, clip, even_sizes(90, 4))
    mix = [1, "p", 8, 3, "p", "p", 5, 2, 7, 1, 6, "p", 4, 8, 8, "p", 3, 5, 7, 2, 6, "p", 4, 4]
    assert sum(1 if c == "p" else c for c in mix) == 90
    c = run_packets(inf, clip, mix)
    for name, x, y in (("pushes vs K=4", a, b), ("pushes vs mixture", a, c), ("K=4 vs mixture", b, c)):
        err = rel_l2(x[0], y[0])
        print(f"{cfg} {name}: {err:.2e}")
        assert err <= 2e-5


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_every_stage_inside_a_packet(cfg):
    from cruse_amd.inferencer import StreamingInferencer
    o, m = models(cfg)
    x = O.synth_pair(1, 160 * 60, seed=7)[0].view(-1)
    _, frames = stream_clip(o, x)
    inf = StreamingInferencer(m, 1, use_graph=False, max_hops=4)
    blocks = x.view(1, 60, 160).cuda()

    def check_packet(first, n):
        torch.cuda.synchronize()
        for f in range(n):
            st = {k: v.cpu().clone() for k, v in inf.stage(0, f).items()}
            t = first + f
            assert ("block" in st) == (t >= 1)
            _check(st, st.get("block"), frames[t], t)

    out, n_out = inf.push_packet(blocks[:, 0:4])                           # starts the clip: frames 0..3
    assert int(n_out[0]) == 3
    check_packet(0, 4)
    for b0 in range(4, 36, 4):
        inf.push_packet(blocks[:, b0:b0 + 4])
    out, n_out = inf.push_packet(blocks[:, 36:40])                         # mid-clip: frames 36..39
    assert int(n_out[0]) == 4
    check_packet(36, 4)
    last = {k: v.cpu().clone() for k, v in inf.stage(0).items()}           # default: the packet's last frame
    assert torch.equal(last["gru2"], inf.stage(0, 3)["gru2"].cpu())
    # a packet that arrives when the slot holds one block: c + 1 frames
    inf.reset()
    inf.push(blocks[:, 0])
    out, n_out = inf.push_packet(blocks[:, 1:4])
    assert int(n_out[0]) == 3
    check_packet(0, 4)


def _serve_packets(inf, plan, n_calls, K, seed):
    """plan: slot -> list of (start call, clip); every call each running clip consumes a seeded random count in [0, K] of its own
    (a pure function of (seed, slot, clip index, call index of the clip), so a clip's packetisation does not depend on the other
    slots); -> {(slot, k): output}"""
    S = inf.S
    res, cur = {}, {}
    queue = {s: list(v) for s, v in plan.items()}
    for p in range(n_calls):
        pkt = torch.zeros(S, K, 160)
        counts = [0] * S
        for s in range(S):
            if s not in cur and queue.get(s) and queue[s][0][0] <= p:
                _, clip = queue[s].pop(0)
                k = sum(1 for key in res if key[0] == s)
                cur[s] = dict(clip=clip.view(-1, 160), b=0, out=[], k=k, rng=np.random.RandomState(seed + 100 * s + k))
            if s in cur:
                c = cur[s]
                want = int(c["rng"].randint(0, K + 1))
                cnt = min(want, c["clip"].shape[0] - c["b"])
                pkt[s, :cnt] = c["clip"][c["b"]:c["b"] + cnt]
                counts[s] = cnt
        out, n_out = inf.push_packet(pkt.cuda(), counts)
        out = out.cpu()
        for s in list(cur):
            c = cur[s]
            c["out"] += [out[s, k] for k in range(int(n_out[s]))]
            c["b"] += counts[s]
            if c["b"] == c["clip"].shape[0]:
                last = inf.flush([s]).cpu()
                res[(s, c["k"])] = torch.cat(c["out"] + [last[0]])
                del cur[s]
    assert not cur and not any(queue.values())
    return res


def test_ragged_serving_and_neighbour_independence():
    from cruse_amd.inferencer import StreamingInferencer
    o, m = models(dict(rnn_groups=4))
    clip = lambda n, seed: O.synth_pair(1, 160 * n, seed=seed)[0].view(-1)
    A = {0: [(0, clip(40, 1))], 1: [(3, clip(30, 2))], 2: [(5, clip(25, 3))], 3: [(1, clip(20, 4)), (14, clip(18, 5))],
         4: [(2, clip(2, 6)), (6, clip(33, 7))]}
    res = _serve_packets(StreamingInferencer(m, 5, max_hops=4), A, 60, 4, seed=5)
    for s, items in A.items():
        for k, (_, c) in enumerate(items):
            err = rel_l2(res[(s, k)], offline(o, c))
            print(f"slot {s} clip {k}: {err:.2e}")
            assert res[(s, k)].shape == c.shape and err <= 2e-5
    # slot 2's clip with its own packetisation, the other slots carrying different clips and counts: bit-identical
    B = {2: A[2], 0: [(1, clip(43, 11))], 4: [(0, clip(12, 12)), (9, clip(30, 13))], 1: [(7, clip(20, 14))]}
    res_b = _serve_packets(StreamingInferencer(m, 5, max_hops=4), B, 60, 4, seed=5)
    assert torch.equal(res_b[(2, 0)], res[(2, 0)])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_state_is_shared_with_push(cfg):
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(cfg)
    x = O.synth_pair(1, 160 * 30, seed=33)[0].view(1, 30, 160).cuda()
    a, b = StreamingInferencer(m, 1, max_hops=8), StreamingInferencer(m, 1, max_hops=8)
    for b0, c in ((0, 4), (4, 8), (12, 3)):
        a.push_packet(x[:, b0:b0 + c])
    for t in range(15):
        b.push(x[:, t])
    torch.cuda.synchronize()
    lay, H = a.lay, a.H
    rows = {"hist": (lay["st_hist"], 161), "tail": (lay["st_tail"], 160), "h1": (lay["st_h1"], H), "h2": (lay["st_h2"], H)}
    for k in range(4):
        rows[f"prev{k}"] = (lay[f"st_prev{k}"], a.ch[k] * (160 >> k))
    for name, (off, n) in rows.items():
        err = rel_l2(a.state[0, off:off + n].cpu(), b.state[0, off:off + n].cpu())
        print(f"{cfg} state row {name}: {err:.2e}")
        assert err <= 1e-5, (name, err)
    assert list(a.nblk) == list(b.nblk) == [15]
    oa, ob = [], []
    for t in range(15, 30):
        oa.append(a.push(x[:, t])[0][0].cpu())
        ob.append(b.push(x[:, t])[0][0].cpu())
    oa.append(a.flush([0])[0].cpu())
    ob.append(b.flush([0])[0].cpu())
    err = rel_l2(torch.cat(oa), torch.cat(ob))
    print(f"{cfg} continued with pushes: {err:.2e}")
    assert err <= 2e-5


def test_packet_graph_replay_equals_eager_launches():
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(ch=(1, 4, 8, 16, 32), rnn_groups=2))
    clips = torch.cat([O.synth_pair(1, 160 * 30, seed=40 + i)[0] for i in range(4)])
    sizes = [4, 4, 1, "p", 8, 3, 4, 4, 1]
    a = run_packets(StreamingInferencer(m, 4, use_graph=True, max_hops=8), clips, sizes)
    b = run_packets(StreamingInferencer(m, 4, use_graph=False, max_hops=8), clips, sizes)
    assert torch.equal(a, b)


def test_refresh_keeps_packet_graphs():
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(ch=(1, 4, 8, 16, 32), rnn_groups=2))
    clips = O.synth_pair(1, 160 * 24, seed=50)[0]
    inf = StreamingInferencer(m, 1, max_hops=4)
    before = run_packets(inf, clips, [4] * 6)
    with torch.no_grad():
        m.conv1_t.bias.add_(0.5)
    inf.refresh()
    after = run_packets(inf, clips, [4] * 6)                               # the captured graphs replay with the new weights
    fresh = run_packets(StreamingInferencer(m, 1, max_hops=4), clips, [4] * 6)
    with torch.no_grad():
        m.conv1_t.bias.sub_(0.5)
    assert torch.equal(after, fresh) and not torch.equal(after, before)


def test_enhance_long_clips_in_bounded_memory():
    from cruse_amd.inferencer import Inferencer, StreamingInferencer
    _, m = models(dict(rnn_groups=4))
    inf = StreamingInferencer(m, 2, max_hops=8)
    off = Inferencer(m)

    def peak(waves):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = inf.enhance(waves)
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    short = torch.cat([O.synth_pair(1, 48000, seed=60 + i)[0] for i in range(2)]).cuda()
    long = torch.cat([O.synth_pair(1, 480000, seed=62 + i)[0] for i in range(2)]).cuda()
    peak(short)                                                            # warm-up: graphs captured, allocator primed
    _, p_short = peak(short)
    got, p_long = peak(long)
    ref = off.mag_mask_to_wave(long)
    for i in range(2):
        err = rel_l2(got[i].cpu(), ref[i].cpu())
        print(f"enhance 30 s clip {i}: {err:.2e}")
        assert got[i].shape == long[i].shape and err <= 2e-5
    extra = 2 * 2 * (480000 - 48000) * 4                                   # the extra input and output waveform bytes
    print(f"enhance peak device memory: 3 s {p_short} B, 30 s {p_long} B, difference {p_long - p_short} B (allowed {extra} B)")
    assert p_long - p_short <= extra
    # a length that is not a multiple of 160: the offline result of the zero-padded clip, trimmed
    L = 160 * 50 + 37
    odd = torch.cat([O.synth_pair(1, L, seed=70 + i)[0] for i in range(2)])
    padded = torch.zeros(2, 160 * 51)
    padded[:, :L] = odd
    got = inf.enhance(odd, hops=3)                                         # a host tensor
    ref = off.mag_mask_to_wave(padded.cuda())[:, :L]
    assert got.shape == (2, L)
    for i in range(2):
        err = rel_l2(got[i].cpu(), ref[i].cpu())
        print(f"enhance L = {L} clip {i}: {err:.2e}")
        assert err <= 2e-5
    assert list(inf.nblk) == [0, 0] and float(inf.state.abs().max()) == 0.0


def test_packet_rejections():
    from cruse_amd import ops
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(ch=(1, 4, 8, 16, 32), rnn_groups=2))
    _, big = models(dict(rnn_groups=4))
    with pytest.raises(ValueError, match="max_hops"):
        StreamingInferencer(m, 2, max_hops=0)
    bound = ops.stream_packet_layout(big.ch)["max_hops"]
    assert bound >= 8
    with pytest.raises(ValueError, match=rf"\[1, {bound}\]"):
        StreamingInferencer(big, 2, max_hops=bound + 1)
    inf = StreamingInferencer(m, 2, max_hops=4)
    z = lambda *shape: torch.zeros(*shape, device="cuda")
    with pytest.raises(ValueError, match="exceeds max_hops"):
        inf.push_packet(z(2, 5, 160))
    with pytest.raises(ValueError, match="counts must lie"):
        inf.push_packet(z(2, 3, 160), [4, 1])
    with pytest.raises(ValueError, match="counts must lie"):
        inf.push_packet(z(2, 3, 160), [-1, 1])
    with pytest.raises(ValueError, match="counts must have"):
        inf.push_packet(z(2, 3, 160), [1, 1, 1])
    for shape in ((2, 3, 161), (3, 2, 160), (2, 100), (2, 0, 160), (320,)):
        with pytest.raises(ValueError, match="expects blocks"):
            inf.push_packet(z(*shape))
    with pytest.raises(ValueError, match="shorter than 320"):
        inf.enhance(z(1, 200))
    with pytest.raises(ValueError, match="hops"):
        inf.enhance(z(1, 3200), hops=5)
    with pytest.raises(ValueError, match="frame"):
        inf.push_packet(z(2, 640))
        inf.stage(0, 4)
    # the C side refuses more frames than fit in LDS
    with pytest.raises(RuntimeError, match="fit in LDS"):
        pk = torch.zeros(2, 1, device="cuda", dtype=torch.int32)
        lay, play = ops.stream_layout(big.ch), ops.stream_packet_layout(big.ch)
        ops.stream_encode_n(pk, 1, big.ch, z(1, bound + 1, 160), ops.stream_tables("cuda"), z(lay["wtotal"]), z(1, lay["st_stride"]),
                            z(1, bound + 2, play["wk_stride"]))


def _mean_wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def test_real_time_bound_64_slots_4_hop_packets():
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(rnn_groups=4))
    inf = StreamingInferencer(m, 64, max_hops=4)
    pkt = 0.1 * torch.randn(64, 4, 160, device="cuda")
    for _ in range(20):
        inf.push_packet(pkt)
    mean = _mean_wall(lambda: inf.push_packet(pkt), 300)
    print(f"64 slots, 4-hop packets: mean call wall {mean * 1e6:.1f} us (RTF {mean / 0.04:.4f})")
    assert mean < 0.040                                                    # the audio a packet carries


def test_packets_are_not_slower_per_hop_than_pushes():
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(rnn_groups=4))
    a, b = StreamingInferencer(m, 1, max_hops=4), StreamingInferencer(m, 1)
    pkt = 0.1 * torch.randn(1, 4, 160, device="cuda")
    for _ in range(50):
        a.push_packet(pkt)
        b.push(pkt[:, 0])
    per_hop_packet = _mean_wall(lambda: a.push_packet(pkt), 500) / 4
    per_hop_push = _mean_wall(lambda: b.push(pkt[:, 0]), 2000)
    print(f"1 slot: per hop {per_hop_packet * 1e6:.1f} us in 4-hop packets, {per_hop_push * 1e6:.1f} us in single pushes "
          f"(ratio {per_hop_packet / per_hop_push:.3f})")
    assert per_hop_packet / per_hop_push < 1.0
