"""MI355X: streaming inference of CRUSE4MagAddSkipUpsample, StreamingInferencer(..., decoder="upsample") on cruse_stream_decode_up / _n_up.

Whole clips against the oracle's offline waveform and the GPU Inferencer, every stage of single frames against the per-frame CPU
restatement (tests/stream_up_ref.py, pinned to the oracle by tests/test_stream_up_host.py), the decoder levels alone on a known input
with the edge bins asserted one by one, packets, graph replay against eager launches, slot independence, one case per constructor
option against the references and bars of that option's own test file, the rejections, and NaN-poisoned buffers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cruse_oracle as O
from oracle import cruse_oracle_ext as X
from tests import postfilter_ref as P
from tests import stream_io_ref as IO
from tests import stream_ref_f16 as R
from tests import stream_rs_ref as RS
from tests.stream_df_ref import offline_df
from tests.stream_up_ref import as_double, nontrivial_bn, stream_clip
from tests.test_gpu_stream_packets import _serve_packets, even_sizes, run_packets
from tests.test_gpu_streaming import _chain, _check, stage_errors, stream_all
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SMALL = dict(ch=(1, 4, 8, 16, 32), rnn_groups=2)
ODD = dict(ch=(1, 3, 5, 6, 8), rnn_groups=1)            # odd channel counts, H = 80
CONFIGS = {"small_g2": SMALL, "odd_g1": ODD, "g4": dict(rnn_groups=4)}
TWO = ["small_g2", "odd_g1"]


@functools.lru_cache(maxsize=None)
def models(name):
    """(oracle module, product module on the device) with the same weights -- built once, shared, never modified"""
    from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
    cfg = CONFIGS[name]
    o = X.CRUSE4MagAddSkipUpsample(**cfg)
    O.closed_form_init(o)
    nontrivial_bn(o)
    o.eval()
    m = CRUSE4MagAddSkipUpsample(precision="f32", **cfg)
    m.load_state_dict(o.state_dict(), strict=True)
    return o, m.cuda().eval()


def server(name, n, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    return StreamingInferencer(models(name)[1], n, decoder="upsample", **kw)


def offline(o, x):
    with torch.no_grad():
        _, est, _ = O.enhanced_spectrum(o, x.view(1, -1))
        return O.istft(torch.complex(est[..., 0], est[..., 1]).transpose(1, 2), 320, 160, 320, length=x.numel()).view(-1)


@functools.lru_cache(maxsize=None)
def frames64(name, seed, nb):
    """(clip, float64 waveform, float64 per-frame intermediates) of the restatement -- computed once, shared, never modified"""
    o, _ = models(name)
    x = O.synth_pair(1, 160 * nb, seed=seed)[0].view(-1)
    y, fr = stream_clip(as_double(o), x, dtype=torch.float64)
    return x, y, fr


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. whole clips -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_whole_clips_equal_offline(name):
    from cruse_amd.inferencer import Inferencer
    o, m = models(name)
    clips = torch.cat([O.synth_pair(1, 32000, seed=100 + i)[0] for i in range(3)])
    got = stream_all(server(name, 3), clips)
    if name == "odd_g1":
        # the offline path runs the training GRU kernels, which take groups of a multiple of 32 units; this model has one group of 80.
        # The streaming GRU kernels take any multiple of 4, so here the server is the only GPU path and the oracle the only reference.
        with pytest.raises(RuntimeError, match="multiple of 32"):
            Inferencer(m).mag_mask_to_wave(clips.cuda())
        ref_gpu = None
    else:
        ref_gpu = Inferencer(m).mag_mask_to_wave(clips.cuda()).cpu()
    for i in range(3):
        e_o = rel_l2(got[i], offline(o, clips[i]))
        e_g = rel_l2(got[i], ref_gpu[i]) if ref_gpu is not None else 0.0
        print(f"{name} clip {i}: streaming vs oracle {e_o:.2e}, vs GPU Inferencer {e_g:.2e}" + (" (refused)" if ref_gpu is None else ""))
        assert got[i].shape == clips[i].shape
        assert e_o <= 2e-5 and e_g <= 2e-5


# ---- 2. every stage of single frames ---------------------------------------------------------------------------------------------------
def push_frames(inf, x, keep):
    """the clip through the single-hop chain, eager: {t: (stages, output block)} of the frames t in `keep`"""
    from cruse_amd import ops
    nb = x.numel() // 160
    blocks = x.view(nb, 160).cuda()
    res = {}
    inf.blocks.copy_(blocks[0:1])
    _chain(inf, 1, [ops.STREAM_STORE])
    inf.blocks.copy_(blocks[1:2])
    res[0] = _chain(inf, 0, [ops.STREAM_FRAME0])[:2]
    res[1] = _chain(inf, 1, [ops.STREAM_FRAME])[:2]
    for b in range(2, nb):
        inf.blocks.copy_(blocks[b:b + 1])
        r = _chain(inf, 1, [ops.STREAM_FRAME])
        if b in keep:
            res[b] = r[:2]
    res[nb] = _chain(inf, 1, [ops.STREAM_END])[:2]
    return {t: v for t, v in res.items() if t in keep}


@pytest.mark.parametrize("name", TWO)
def test_every_stage_of_single_frames(name):
    """spectrum, e1..e4, skip1..4, gru1, gru2, mask, block of frames 0, 1, 37 and the end frame: rel-L2 <= 1e-5 each, the bar of unet_2.
    The mask row is the output of all four decoder levels, columns 0 and 2*Fin - 1 of each included."""
    o, _ = models(name)
    x = O.synth_pair(1, 160 * 60, seed=7)[0].view(-1)
    _, frames = stream_clip(o, x)
    got = push_frames(server(name, 1, use_graph=False), x, (0, 1, 37, 60))
    assert sorted(got) == [0, 1, 37, 60]
    for t, (st, out) in got.items():
        print(f"{name} frame {t}: " + ", ".join(f"{k} {v:.1e}" for k, v in stage_errors(st, out, frames[t], t).items()))
    for t, (st, out) in got.items():
        _check(st, out, frames[t], t)


# ---- 3. the decoder levels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TWO)
def test_decoder_edges_in_isolation(name):
    """One decode launch on work rows written by the test: the GRU output and the four skip rows are sin / cos patterns, so every decoder
    level sees an input whose edge columns differ from their neighbours.  The mask row against the float64 modules, element by element:
    |error| <= 1e-5 -- the mask is a sigmoid in (0, 1), its f32 rounding is 6e-8, and the four levels sum at most 3 * 32 products each, so
    1e-5 absolute leaves two orders for the f32 accumulation and none for a wrong or missing tap (a shifted input moves them by 1e-3 or more
    here, which the last assertion checks on the reference itself)."""
    from cruse_amd import ops
    o, _ = models(name)
    o64 = as_double(o)
    inf = server(name, 2, use_graph=False)
    lay, ch, H = inf.lay, inf.ch, inf.H
    i = lambda n: torch.arange(n, dtype=torch.float64)
    h2 = torch.sin(0.7 * i(H) + 0.3)
    skips = {k: 0.5 * torch.cos(0.31 * i(ch[k] * (160 >> k)) + k) for k in range(1, 5)}
    row = torch.zeros(lay["wk_stride"], dtype=torch.float64)
    row[lay["wk_h2n"]:lay["wk_h2n"] + H] = h2
    row[lay["wk_re"]:lay["wk_re"] + 161] = 1.0
    for k in range(1, 5):
        row[lay[f"wk_skip{k}"]:lay[f"wk_skip{k}"] + skips[k].numel()] = skips[k]
    inf.work[1].copy_(row.float())                                            # slot 1; slot 0 is skipped
    inf.mode[1].copy_(torch.tensor([ops.STREAM_SKIP, ops.STREAM_FRAME], dtype=torch.int32))
    before = inf.work[0].clone()
    ops.stream_decode(inf.mode[1], ch, inf.tab, inf.w, inf.ln2_eps, inf.state, inf.work, inf.out, decoder="upsample")
    torch.cuda.synchronize()
    got = inf.work[1, lay["wk_mask"]:lay["wk_mask"] + 160].cpu().double()
    assert torch.equal(inf.work[0], before)
    with torch.no_grad():
        as4 = lambda v, k: v.view(1, ch[k], 1, 160 >> k)
        # the inputs as the kernel holds them: f32 values
        d = as4(o64.gru.ln2(h2.float().double()), 4) + as4(skips[4].float().double(), 4)
        for k in range(4, 1, -1):
            d = getattr(o64, f"dec{k}")(d) + as4(skips[k - 1].float().double(), k - 1)
        ref = o64.dec1(d).reshape(-1)
        # the same with the two outermost taps of dec1 dropped at the edges' neighbours: what a wrong edge would give
        shifted = o64.dec1(torch.roll(d, 1, dims=-1)).reshape(-1)
    err = (got - ref).abs()
    print(f"{name}: mask row vs float64: worst |error| {float(err.max()):.2e} at bin {int(err.argmax())}; bins 0, 1, 158, 159: "
          + ", ".join(f"{float(err[b]):.1e}" for b in (0, 1, 158, 159)) + f"; mask range {float(ref.min()):.3f} .. {float(ref.max()):.3f}")
    assert float(err.max()) <= 1e-5
    for b in (0, 1, 158, 159):
        assert float(err[b]) <= 1e-5, (b, float(err[b]))
    assert float((shifted - ref).abs()[[0, 1, 158, 159]].min()) > 1e-4       # the edge bins are sensitive to what feeds them


# ---- 4. packets ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 8])
def test_ragged_packets_equal_single_pushes(K):
    """Every call each running clip consumes a seeded random count in [0, K] (zeros included; a clip's last packet is as short as what is
    left, so slots end mid-packet while their neighbours go on).  The relation tests/test_gpu_stream_packets.py holds unet_2 to: packets
    against single pushes of the same clip, rel-L2 <= 2e-5 (the packet chain's GRU sums round differently), and against the oracle's
    offline waveform at the same bar."""
    name = "small_g2"
    o, _ = models(name)
    clip = lambda n, seed: O.synth_pair(1, 160 * n, seed=seed)[0].view(-1)
    plan = {0: [(0, clip(23, 1))], 1: [(1, clip(9, 2)), (12, clip(14, 3))], 2: [(2, clip(2, 4)), (5, clip(17, 5))]}
    res = _serve_packets(server(name, 3, max_hops=K), plan, 60, K, seed=5)
    single = server(name, 1)
    for s, items in plan.items():
        for k, (_, c) in enumerate(items):
            pushes = stream_all(single, c.view(1, -1))[0]
            e_p, e_o = rel_l2(res[(s, k)], pushes), rel_l2(res[(s, k)], offline(o, c))
            print(f"K={K} slot {s} clip {k} ({c.numel() // 160} blocks): packets vs pushes {e_p:.2e}, vs oracle {e_o:.2e}")
            assert res[(s, k)].shape == c.shape and e_p <= 2e-5 and e_o <= 2e-5


@pytest.mark.parametrize("name", TWO)
def test_packet_sizes_stages_and_enhance(name):
    o, _ = models(name)
    x, _, _ = frames64(name, 21, 40)
    _, frames = stream_clip(o, x)
    inf = server(name, 1, max_hops=8, use_graph=False)
    a = stream_all(inf, x.view(1, -1))
    for sizes in (even_sizes(40, 2), even_sizes(40, 8), [1, "p", 8, 3, "p", 5, 2, 7, 6, "p", 4, 1]):
        b = run_packets(inf, x.view(1, -1), sizes)
        err = rel_l2(b[0], a[0])
        print(f"{name} {sizes}: packets vs pushes {err:.2e}")
        assert err <= 2e-5
    # every stage of every frame inside a packet that starts the clip (frames 0..7) and of one mid-clip
    blocks = x.view(1, 40, 160).cuda()
    for first, lo in ((0, 0), (15, 16)):
        if lo:
            inf.push_packet(blocks[:, 8:16])
        inf.push_packet(blocks[:, lo:lo + 8])
        torch.cuda.synchronize()
        for f in range(8):
            st = {k: v.cpu().clone() for k, v in inf.stage(0, f).items()}
            t = lo + f if lo else f
            assert ("block" in st) == (t >= 1)
            _check(st, st.get("block"), frames[t], t)
    inf.reset()
    # enhance(): a length that is no multiple of 160 is the offline result of the zero-padded clip, trimmed
    L = 160 * 30 + 37
    odd = torch.cat([O.synth_pair(1, L, seed=70 + i)[0] for i in range(2)])
    inf2 = server(name, 2, max_hops=8)
    got = inf2.enhance(odd, hops=3).cpu()
    assert got.shape == (2, L)
    for i in range(2):
        padded = torch.cat([odd[i], torch.zeros(160 * 31 - L)])
        err = rel_l2(got[i], offline(o, padded)[:L])
        print(f"{name} enhance L = {L} clip {i}: vs oracle {err:.2e}")
        assert err <= 2e-5
    assert list(inf2.nblk) == [0, 0] and float(inf2.state.abs().max()) == 0.0


# ---- 5. graph replay, slot independence ------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_launches():
    clips = torch.cat([O.synth_pair(1, 160 * 30, seed=40 + i)[0] for i in range(4)])
    a = stream_all(server("small_g2", 4, use_graph=True), clips)
    b = stream_all(server("small_g2", 4, use_graph=False), clips)
    assert torch.equal(bits(a), bits(b))
    sizes = [4, 4, 1, "p", 8, 3, 4, 4, 1]
    a = run_packets(server("small_g2", 4, use_graph=True, max_hops=8), clips, sizes)
    b = run_packets(server("small_g2", 4, use_graph=False, max_hops=8), clips, sizes)
    assert torch.equal(bits(a), bits(b))


def test_a_slot_does_not_see_its_neighbours():
    """slot 1's clip with its neighbours active on other clips, idle throughout, or reset in the middle of theirs: one set of bits"""
    nb = 24
    mine = O.synth_pair(1, 160 * nb, seed=50)[0].view(nb, 160)
    other = [O.synth_pair(1, 160 * nb, seed=51 + i)[0].view(nb, 160) for i in range(2)]

    def run(neighbours):
        inf = server("odd_g1", 3)
        outs = []
        for b in range(nb):
            blk = torch.stack([other[0][b], mine[b], other[1][b]]).cuda()
            act = [neighbours != "idle", True, neighbours != "idle"]
            if neighbours == "reset" and b in (7, 15):
                inf.reset([0, 2] if b == 7 else [2])
            out, valid = inf.push(blk, act)
            if valid[1]:
                outs.append(out[1].cpu())
        outs.append(inf.flush([1])[0].cpu())
        return torch.cat(outs)

    a, b, c = run("active"), run("idle"), run("reset")
    assert a.shape == (160 * nb,) and torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
    # and in packets: slot 1 alone against slot 1 beside two busy neighbours
    def run_k(busy):
        inf = server("odd_g1", 3, max_hops=4)
        outs = []
        for b0 in range(0, nb, 4):
            pkt = torch.stack([other[0][b0:b0 + 4], mine[b0:b0 + 4], other[1][b0:b0 + 4]]).cuda()
            out, n_out = inf.push_packet(pkt, [3 if busy else 0, 4, 2 if busy else 0])
            outs += [out[1, k].cpu() for k in range(int(n_out[1]))]
        outs.append(inf.flush([1])[0].cpu())
        return torch.cat(outs)

    assert torch.equal(bits(run_k(True)), bits(run_k(False)))


# ---- 6. the options compose ------------------------------------------------------------------------------------------------------------
def test_limit_pcm_and_post_filter_together():
    """tests/test_gpu_postfilter.py::test_with_a_limit_and_pcm_out with PCM input as well: int16 in, int16 out, a tau and a limit per slot,
    against the quantised float64 reference, at most 1 LSB apart; the clip counter as there"""
    from tests.test_gpu_stream_io import K, L, S, WAYS, drive
    name, kind = "small_g2", "iam"
    o, _ = models(name)
    o64 = as_double(o)
    taus = (0.02, 0.0, 0.2)
    v = torch.stack([IO.pcm_noise(L, 400 + s) for s in range(S)])             # int16, about -12 dBFS
    x = v.float() / 32768.0
    ref = []
    for s in range(S):
        e = P.e64_pf(stream_clip(o64, x[s], dtype=torch.float64)[1], taus[s], kind)
        ref.append(IO.quantise(P.mix(x[s], e, IO.gain(IO.LIMS_DB[s])).float().numpy()))
    for way in ("pushes", "push+packets"):
        inf = server(name, S, max_hops=K, post_filter=kind, atten_lim=True, pcm_in=True, pcm_out=True)
        inf.set_post_filter(list(taus))
        inf.set_atten_lim(list(IO.LIMS_DB))
        q = drive(inf, v, WAYS[way])
        n = inf.clipped()
        for s in range(S):
            wq, wc = ref[s]
            assert q[s].dtype == torch.int16 and q[s].shape == (L,)
            d = np.abs(q[s].numpy().astype(np.int64) - wq.astype(np.int64))
            print(f"{way} slot {s}: vs the quantised float64 reference {int((d == 0).sum())} of {L} equal, worst {int(d.max())} LSB; "
                  f"clipped() {int(n[s])}, the reference clamps {int(wc.sum())}")
            assert d.max() <= 1, (way, s, int(d.max()))
            sat = int(((q[s] == 32767) | (q[s] == -32768)).sum())
            assert n[s] <= sat and abs(int(n[s]) - int(wc.sum())) <= int((d != 0).sum()), (s, int(n[s]), sat, int(wc.sum()))


def test_f16_mode():
    """the bars of tests/test_gpu_stream_f16.py: the stages in front of the GRU at 1e-5, gru1 / gru2 / mask at 1e-3 against float64; the whole
    clip within twice the distance of the f16-operand emulation from float64.  That the f16 kernels ran shows on gru1, whose operands they
    round (2e-4 measured against 2e-7 in f32 mode); this model's waveform hardly moves with the GRU rows (4.2e-7 in both modes), so the
    whole-clip floor that test file uses for unet_2 says nothing here."""
    name, nb = "small_g2", 60
    o, _ = models(name)
    x, ref64, fr64 = frames64(name, 11, nb)
    e_emu = R.rel(stream_clip(R.emulation(o), x)[0], ref64)
    got = push_frames(server(name, 1, precision="f16", use_graph=False), x, (0, 1, 37, nb))
    for t, (st, out) in got.items():
        errs = stage_errors(st, out, fr64[t], t)
        print(f"f16 frame {t}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert errs["gru1"] > 1e-5, (t, errs["gru1"], "this is the f32 path's error: the f16 kernels did not run")
        for k, e in errs.items():
            if k in R.STAGES_F16:
                assert e <= R.BAR_F16, (t, k, e)
            elif k != "block":
                assert e <= R.BAR_F32, (t, k, e)
    for tag, y in (("pushes", stream_all(server(name, 1, precision="f16"), x.view(1, -1))[0]),
                   ("packets of 4", run_packets(server(name, 1, precision="f16", max_hops=4), x.view(1, -1), even_sizes(nb, 4))[0])):
        err = R.rel(y, ref64)
        print(f"f16 {tag}: whole clip vs float64 {err:.2e}; emulation vs float64 {e_emu:.2e}")
        assert y.shape == ref64.shape and err <= 2 * e_emu, (tag, err, e_emu)


def test_forty_eight_kilohertz():
    """Out(E64(In(u))) of tests/stream_rs_ref.py with E64 this model's float64 restatement; the bar of tests/test_gpu_stream_rs.py"""
    from tests import test_gpu_stream_rs as T
    name, rate = "small_g2", 48000
    o64 = as_double(models(name)[0])
    clips = T.clips_at(rate)
    inf = server(name, T.S, max_hops=T.K, io_rate=rate)
    assert inf.io_block == 480
    for way in ("pushes", "push+packets"):
        got = T.drive(inf, clips, T.WAYS[way])
        for s in range(T.S):
            want = RS.resample_out(stream_clip(o64, RS.resample_in(clips[s], rate), dtype=torch.float64)[0], rate)
            err = rel_l2(got[s], want)
            print(f"48 kHz {way} slot {s}: vs Out(E64(In(u))) {err:.2e}")
            assert got[s].shape == (IO.NB * 480,) and err <= T.BAR, (way, s, err)


def test_df_head():
    """the DeepFilter(1, 5) head reads the work rows alone: against Inferencer(head="df") on the same module and the oracle's offline
    filter, 2e-5 as tests/test_gpu_stream_df.py"""
    from cruse_amd.inferencer import Inferencer
    name, L = "small_g2", 1600
    o, m = models(name)
    x = torch.cat([O.synth_pair(1, L, seed=300 + i)[0] for i in range(3)])
    want = torch.stack([offline_df(o, x[i]) for i in range(3)])
    want_gpu = Inferencer(m, head="df").mag_mask_to_wave(x.cuda()).cpu()
    plain = stream_all(server(name, 3), x)
    inf = server(name, 3, head="df", max_hops=4)
    runs = {"push (single-hop chain)": stream_all(server(name, 3, head="df"), x), "push": stream_all(inf, x),
            "packets of 3": run_packets(inf, x, even_sizes(10, 3)), "enhance": inf.enhance(x.cuda()).cpu()}
    for tag, got in runs.items():
        assert got.shape == x.shape, tag
        for i in range(3):
            e_o, e_g, far = rel_l2(got[i], want[i]), rel_l2(got[i], want_gpu[i]), rel_l2(got[i], plain[i])
            print(f"df {tag} clip {i}: vs oracle df {e_o:.2e}, vs Inferencer(head=df) {e_g:.2e}, vs the mask stream {far:.2f}")
            assert e_o <= 2e-5 and e_g <= 2e-5, (tag, i, e_o, e_g)
            assert far > 1.0, (tag, i, far)


# ---- 7. rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    from cruse_amd.inferencer import StreamingInferencer
    from cruse_amd.model.cruse_net import unet_2
    _, m = models("small_g2")
    u = unet_2(precision="f32", **SMALL).cuda().eval()
    with pytest.raises(ValueError, match="CRUSE4MagAddSkipUpsample"):
        StreamingInferencer(u, 2, decoder="upsample")
    with pytest.raises(ValueError, match="bogus"):
        StreamingInferencer(u, 2, decoder="bogus")
    with pytest.raises(ValueError, match="bogus"):
        StreamingInferencer(m, 2, decoder="bogus")
    for kw in ({}, dict(decoder="transposed")):
        with pytest.raises(ValueError, match=r"upsample.*decoder="):
            StreamingInferencer(m, 2, **kw)
    with pytest.raises(ValueError, match="n_fft"):
        StreamingInferencer(m, 2, decoder="upsample", n_fft=512, win_length=512)
    with pytest.raises(ValueError, match="filter field"):
        StreamingInferencer(m, 2, decoder="upsample", head="df", post_filter="iam")
    with pytest.raises(ValueError, match="decoder"):
        ops.stream_decode(None, SMALL["ch"], None, None, 1e-5, None, None, torch.zeros(1, 160, device="cuda"), decoder="bogus")
    # the C entry points refuse before any launch: the output stays poisoned, the error code is CRUSE_E_SHAPE (-1)
    inf = server("small_g2", 2, use_graph=False, max_hops=2)
    inf.push(torch.zeros(2, 160, device="cuda"))
    inf.push(torch.zeros(2, 160, device="cuda"))
    torch.cuda.synchronize()
    POISON = 777.0
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ch = [int(c) for c in inf.ch]
    tau = torch.zeros(2, device="cuda")

    def single(S=2, out="own", fmt=0, clip=None, pf_kind=0, pf_tau=None):
        inf.out.fill_(POISON)
        work = inf.work.clone()
        rc = lib.cruse_stream_decode_up(p(inf.mode[1]), S, *ch, p(inf.tab), p(inf.w), inf.ln2_eps, p(inf.state), p(inf.work),
                                        p(inf.out) if out == "own" else None, fmt, None, clip, pf_kind, pf_tau, None)
        torch.cuda.synchronize()
        assert bool((inf.out == POISON).all()) and torch.equal(bits(inf.work), bits(work))
        return rc, lib.cruse_last_error().decode()

    def packet(S=2, out="own", fmt=0, out_hops=2, frames=3, pf_kind=0, pf_tau=None):
        inf.pout.fill_(POISON)
        work = inf.pwork.clone()
        rc = lib.cruse_stream_decode_n_up(p(inf.pk), S, 2, out_hops, frames, *ch, p(inf.tab), p(inf.w), inf.ln2_eps, p(inf.state),
                                          p(inf.pwork), p(inf.pout) if out == "own" else None, fmt, None, None, pf_kind, pf_tau, None)
        torch.cuda.synchronize()
        assert bool((inf.pout == POISON).all()) and torch.equal(bits(inf.pwork), bits(work))
        return rc, lib.cruse_last_error().decode()

    clipc = torch.zeros(2, device="cuda", dtype=torch.int32)
    cases = [(single, dict(out=None), "null"), (single, dict(S=0), "S = 0"), (single, dict(fmt=7), "format"),
             (single, dict(clip=p(clipc)), "clip counter"), (single, dict(pf_kind=3, pf_tau=p(tau)), "kind"),
             (single, dict(pf_kind=1), "pf_tau"),
             (packet, dict(out=None), "null"), (packet, dict(S=0), "S = 0"), (packet, dict(fmt=7), "format"),
             (packet, dict(out_hops=1), "out_hops"), (packet, dict(frames=2), "work_frames"), (packet, dict(pf_kind=1), "pf_tau")]
    for fn, kw, word in cases:
        rc, msg = fn(**kw)
        print(f"{fn.__name__} {kw}: rc {rc}: {msg}")
        assert rc == -1 and word in msg, (fn.__name__, kw, rc, msg)


# ---- 8. poisoned buffers ----------------------------------------------------------------------------------------------------------------
def _fields(lay, ch, H, play=None):
    """(name, offset, floats) of every documented field of a work row and of a state row"""
    F = [160 >> k for k in range(5)]
    wk = [("wk_re", 161), ("wk_im", 161), ("wk_x", H), ("wk_h1n", H), ("wk_h2n", H), ("wk_mask", 160)] \
        + [(f"wk_skip{k}", ch[k] * F[k]) for k in range(1, 5)]
    st = [("st_hist", 161), ("st_tail", 160), ("st_h1", H), ("st_h2", H)] + [(f"st_prev{k}", ch[k] * F[k]) for k in range(4)]
    wk = [(n, lay[n], c) for n, c in wk]
    if play is not None:
        wk += [(f"wk_e{k}", play[f"wk_e{k}"], ch[k] * F[k]) for k in range(1, 4)]
    return wk, [(n, lay[n], c) for n, c in st]


def _inside(fields, stride):
    m = torch.zeros(stride, dtype=torch.bool)
    for _, off, n in fields:
        assert not m[off:off + n].any()                                       # the fields do not overlap
        m[off:off + n] = True
    return m


@pytest.mark.parametrize("name", TWO)
def test_poisoned_buffers(name):
    """work, out and the padding between the fields of the state rows are NaN before every chain: each chain writes every field it reads
    and nothing else -- the padding and the rows of an inactive slot keep their NaN, no NaN reaches a field, an output block or the state,
    and the outputs have the bits of an unpoisoned run"""
    nan = float("nan")
    x = torch.cat([O.synth_pair(1, 160 * 12, seed=80 + i)[0] for i in range(3)]).cuda()
    free = server(name, 3, use_graph=False, max_hops=4)
    inf = server(name, 3, use_graph=False, max_hops=4)
    wkf, stf = _fields(inf.lay, inf.ch, inf.H)
    pwf, _ = _fields(inf.lay, inf.ch, inf.H, inf.play)
    wk_in, st_in = _inside(wkf, inf.lay["wk_stride"]).cuda(), _inside(stf, inf.lay["st_stride"]).cuda()
    pw_in = _inside(pwf, inf.play["wk_stride"]).cuda()
    assert int((~wk_in).sum()) > 0 and int((~st_in).sum()) > 0                 # there is padding to watch
    inf.state[:, ~st_in] = nan

    def poison():
        inf.work.fill_(nan)
        inf.pwork.fill_(nan)
        inf.out.fill_(nan)
        inf.pout.fill_(nan)

    # pushes: slot 2 stays inactive; block 0 is STORE (no frame: nothing of work or out is written), block 1 FRAME0 + FRAME
    for b in range(4):
        poison()
        blk = x[:, 160 * b:160 * (b + 1)]
        out, valid = inf.push(blk, [True, True, False])
        ref, _ = free.push(blk, [True, True, False])
        torch.cuda.synchronize()
        assert torch.isnan(inf.work[2]).all() and torch.isnan(inf.out[2]).all() and torch.isnan(inf.pwork).all() and torch.isnan(inf.pout).all()
        if b == 0:
            assert torch.isnan(inf.work).all() and torch.isnan(inf.out).all() and not valid.any()
        else:
            assert valid.tolist() == [True, True, False]
            assert torch.isnan(inf.work[:2][:, ~wk_in]).all() and not torch.isnan(inf.work[:2][:, wk_in]).any()
            assert not torch.isnan(out[:2]).any() and torch.equal(bits(out[:2]), bits(ref[:2]))
        assert torch.isnan(inf.state[:, ~st_in]).all() and not torch.isnan(inf.state[:, st_in]).any()
    # a packet: slot 0 takes 4 blocks (4 frames), slot 1 two, slot 2 starts its clip with three (frames 0..2, two blocks)
    poison()
    pkt = x[:, 640:1280].reshape(3, 4, 160).contiguous()
    out, n_out = inf.push_packet(pkt, [4, 2, 3])
    ref, _ = free.push_packet(pkt, [4, 2, 3])
    torch.cuda.synchronize()
    assert n_out.tolist() == [4, 2, 2]
    for s, (n, nf) in enumerate([(4, 4), (2, 2), (2, 3)]):
        assert not torch.isnan(inf.pout[s, :n]).any() and torch.isnan(inf.pout[s, n:]).all(), s
        assert torch.equal(bits(out[s, :n]), bits(ref[s, :n])), s
        assert not torch.isnan(inf.pwork[s, :nf][:, pw_in]).any() and torch.isnan(inf.pwork[s, :nf][:, ~pw_in]).all(), s
        assert torch.isnan(inf.pwork[s, nf:]).all(), s
    assert torch.isnan(inf.work).all() and torch.isnan(inf.out).all()
    assert torch.isnan(inf.state[:, ~st_in]).all() and not torch.isnan(inf.state[:, st_in]).any()
    # flush of slots 0 and 2: their end frames; slot 1 is not touched
    poison()
    last, ref = inf.flush([0, 2]), free.flush([0, 2])
    torch.cuda.synchronize()
    assert not torch.isnan(last).any() and torch.equal(bits(last), bits(ref))
    assert torch.isnan(inf.work[1]).all() and torch.isnan(inf.out[1]).all()
    assert torch.isnan(inf.work[[0, 2]][:, ~wk_in]).all() and not torch.isnan(inf.work[[0, 2]][:, wk_in]).any()
