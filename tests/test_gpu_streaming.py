"""MI355X: frame-by-frame streaming inference (cruse_amd.inferencer.StreamingInferencer, cruse_stream_* kernels).

Whole clips against the oracle's offline waveform and the GPU Inferencer, every stage of single frames against the per-frame
CPU restatement (tests/stream_ref.py, pinned to the oracle by tests/test_stream_host.py), multi-slot serving, graph replay vs
eager launches, a real-time bound and the rejections."""
import time

import pytest
import torch

from oracle import cruse_oracle as O
from tests.stream_ref import nontrivial_bn, stream_clip
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

CONFIGS = [dict(rnn_groups=4), dict(rnn_groups=1), dict(ch=(1, 4, 8, 16, 32), rnn_groups=2)]
IDS = ["g4", "g1", "small_g2"]


def models(cfg):
    from cruse_amd.model.cruse_net import unet_2
    o = O.unet_2(**cfg)
    O.closed_form_init(o)
    nontrivial_bn(o)
    o.eval()
    m = unet_2(precision="f32", **cfg)
    m.load_state_dict(o.state_dict())
    return o, m.cuda().eval()


def offline(o, x):
    with torch.no_grad():
        _, est, _ = O.enhanced_spectrum(o, x.view(1, -1))
        return O.istft(torch.complex(est[..., 0], est[..., 1]).transpose(1, 2), 320, 160, 320, length=x.numel()).view(-1)


def stream_all(inf, clips):
    """push the clips (one per slot, equal lengths) block by block, flush all; -> [n, L] on the host"""
    n, L = clips.shape
    outs = [[] for _ in range(n)]
    blocks = clips.view(n, L // 160, 160).cuda()
    for b in range(L // 160):
        out, valid = inf.push(blocks[:, b])
        for s in range(n):
            if valid[s]:
                outs[s].append(out[s].cpu())
    last = inf.flush(list(range(n))).cpu()
    return torch.stack([torch.cat(outs[s] + [last[s]]) for s in range(n)])


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_whole_clips_equal_offline(cfg):
    from cruse_amd.inferencer import Inferencer, StreamingInferencer
    o, m = models(cfg)
    clips = torch.cat([O.synth_pair(1, 32000, seed=100 + i)[0] for i in range(3)])
    inf = StreamingInferencer(m, 3)
    got = stream_all(inf, clips)
    ref_gpu = Inferencer(m).mag_mask_to_wave(clips.cuda()).cpu()
    for i in range(3):
        e_o, e_g = rel_l2(got[i], offline(o, clips[i])), rel_l2(got[i], ref_gpu[i])
        print(f"{cfg} clip {i}: streaming vs oracle {e_o:.2e}, vs GPU Inferencer {e_g:.2e}")
        assert got[i].shape == clips[i].shape
        assert e_o <= 2e-5 and e_g <= 2e-5


def _chain(inf, row, modes):
    from cruse_amd import ops
    inf.mode[row].copy_(torch.tensor(modes, dtype=torch.int32))
    inf._chain(row)
    torch.cuda.synchronize()
    return {k: v.cpu().clone() for k, v in inf.stage(0).items()}, inf.out[0].cpu().clone(), ops


def stage_errors(stage, out, ref, t):
    """rel-L2 of every stage of frame t (and of its output block, t >= 1) against the restatement's frame `ref`, in order"""
    # the spectrum as one complex vector (frame 0 is symmetric after windowing: its imaginary part is rounding noise alone)
    errs = {"spectrum": rel_l2(torch.complex(stage["re"], stage["im"]), torch.complex(ref["re"], ref["im"]))}
    for k in ("e1", "e2", "e3", "e4", "skip1", "skip2", "skip3", "skip4", "gru1", "gru2", "mask"):
        errs[k] = rel_l2(stage[k], ref[k].reshape(-1))
    if t >= 1:
        errs["block"] = rel_l2(out, ref["block"])
    return errs


def _check(stage, out, ref, t):
    errs = stage_errors(stage, out, ref, t)
    for k, err in errs.items():
        assert err <= 1e-5, (t, k, err)
    return max(errs.values())


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_every_stage_of_single_frames(cfg):
    from cruse_amd import ops
    from cruse_amd.inferencer import StreamingInferencer
    o, m = models(cfg)
    x = O.synth_pair(1, 160 * 60, seed=7)[0].view(-1)
    _, frames = stream_clip(o, x)
    inf = StreamingInferencer(m, 1, use_graph=False)
    blocks = x.view(60, 160).cuda()
    inf.blocks.copy_(blocks[0:1])
    _chain(inf, 1, [ops.STREAM_STORE])
    inf.blocks.copy_(blocks[1:2])
    st, out, _ = _chain(inf, 0, [ops.STREAM_FRAME0])
    _check(st, out, frames[0], 0)
    st, out, _ = _chain(inf, 1, [ops.STREAM_FRAME])
    _check(st, out, frames[1], 1)
    for b in range(2, 60):
        inf.blocks.copy_(blocks[b:b + 1])
        st, out, _ = _chain(inf, 1, [ops.STREAM_FRAME])
        if b == 37:
            _check(st, out, frames[37], 37)
    st, out, _ = _chain(inf, 1, [ops.STREAM_END])
    _check(st, out, frames[60], 60)


def _serve(inf, plan, n_pushes):
    """plan: slot -> list of (start push, clip, inactive pushes); runs n_pushes pushes (+ flushes); -> {(slot, k): output}"""
    S = inf.S
    res, cur = {}, {}
    queue = {s: list(v) for s, v in plan.items()}
    for p in range(n_pushes):
        blocks = torch.zeros(S, 160)
        active = [False] * S
        for s in range(S):
            if s not in cur and queue.get(s) and queue[s][0][0] <= p:
                start, clip, off = queue[s].pop(0)
                cur[s] = dict(clip=clip.view(-1, 160), b=0, off=set(off), out=[], k=sum(1 for key in res if key[0] == s))
            if s in cur and p not in cur[s]["off"]:
                c = cur[s]
                blocks[s] = c["clip"][c["b"]]
                active[s] = True
        out, valid = inf.push(blocks.cuda(), active)
        out = out.cpu()
        for s in list(cur):
            c = cur[s]
            if not active[s]:
                continue
            if valid[s]:
                c["out"].append(out[s])
            c["b"] += 1
            if c["b"] == c["clip"].shape[0]:
                last = inf.flush([s]).cpu()
                res[(s, c["k"])] = torch.cat(c["out"] + [last[0]])
                del cur[s]
    assert not cur and not any(queue.values())
    return res


def test_serving_staggered_inactive_reused_slots():
    from cruse_amd.inferencer import StreamingInferencer
    o, m = models(dict(rnn_groups=4))
    clip = lambda n, seed: O.synth_pair(1, 160 * n, seed=seed)[0].view(-1)
    A = {0: [(0, clip(40, 1), [])], 1: [(3, clip(30, 2), [])], 2: [(7, clip(25, 3), [12, 13, 14, 15, 16])],
         3: [(1, clip(20, 4), []), (22, clip(18, 5), [])], 4: [(2, clip(2, 6), []), (5, clip(33, 7), [20])]}
    inf = StreamingInferencer(m, 5)
    res = _serve(inf, A, 45)
    for s, items in A.items():
        for k, (_, c, _) in enumerate(items):
            err = rel_l2(res[(s, k)], offline(o, c))
            print(f"slot {s} clip {k}: {err:.2e}")
            assert res[(s, k)].shape == c.shape and err <= 2e-5
    # slot 2's clip alone, the other slots carrying different clips on different schedules: bit-identical
    B = {2: A[2], 0: [(1, clip(43, 11), [5, 6])], 4: [(0, clip(12, 12), []), (14, clip(30, 13), [])], 1: [(9, clip(20, 14), [])]}
    res_b = _serve(StreamingInferencer(m, 5), B, 50)
    assert torch.equal(res_b[(2, 0)], res[(2, 0)])


def test_graph_replay_equals_eager_launches():
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(ch=(1, 4, 8, 16, 32), rnn_groups=2))
    clips = torch.cat([O.synth_pair(1, 160 * 30, seed=40 + i)[0] for i in range(4)])
    a = stream_all(StreamingInferencer(m, 4, use_graph=True), clips)
    b = stream_all(StreamingInferencer(m, 4, use_graph=False), clips)
    assert torch.equal(a, b)


def test_real_time_bound_64_slots():
    from cruse_amd.inferencer import StreamingInferencer
    _, m = models(dict(rnn_groups=4))
    inf = StreamingInferencer(m, 64)
    blocks = 0.1 * torch.randn(64, 160, device="cuda")
    for _ in range(20):
        inf.push(blocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(400):
        inf.push(blocks)
    torch.cuda.synchronize()
    mean = (time.perf_counter() - t0) / 400
    print(f"64 slots: mean push wall {mean * 1e6:.1f} us (RTF {mean / 0.01:.4f})")
    assert mean < 0.010


def test_rejections():
    from cruse_amd.inferencer import StreamingInferencer
    from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
    _, m = models(dict(ch=(1, 4, 8, 16, 32), rnn_groups=2))
    with pytest.raises(ValueError, match="n_fft"):
        StreamingInferencer(m, 2, n_fft=512, win_length=512)
    with pytest.raises(ValueError, match="upsample"):
        StreamingInferencer(CRUSE4MagAddSkipUpsample().cuda(), 2)
    inf = StreamingInferencer(m, 2)
    inf.push(torch.zeros(2, 160, device="cuda"))
    with pytest.raises(ValueError, match="at least 2"):
        inf.flush([0])
