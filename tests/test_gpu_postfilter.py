"""MI355X: the perceptual post-filter -- ops.post_filter (cruse_mask_postfilter), StreamingInferencer(post_filter=...) on the PF instances
of the decode kernels (cruse_stream_decode_pf / _n_pf), Inferencer(post_filter=...) and evaluate_files(post_filter=...).

References: tests/postfilter_ref.py, float64 -- pf(g, tau, kind) (pinned on the reference's own outputs by tests/test_postfilter_host.py) and
R(x, lim) = lim x + (1 - lim) E64_pf(x), the float64 per-frame chain with pf on the mask row.  Bars: BAR of tests/test_gpu_stream_io.py for
the chain (2e-5 rel-L2 per clip), 1 LSB for PCM, bit equality wherever the same floats are expected, PF_BAR for the pointwise function.
Models, slots, clips and the three ways through a clip are those of tests/test_gpu_stream_io.py, whose helpers are imported.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import postfilter_ref as P
from tests import stream_io_ref as IO
from tests.test_gpu_stream_io import BAR, K, L, NAMES, PUSH_PACKETS, S, WAYS, drive, server, setup
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

TAUS = (0.02, 0.0, 0.2)                    # per slot: the reference's default, off, strong
# ops.post_filter against float64 on the 4097-gain sweep, both kinds, tau 0.02 and 0.5: the worst absolute error measured on an MI355X is
# PF_MEASURED = 1.571e-7 ("iam", tau 0.02; about one ulp of a value near 1).  The bar is 4 x that, rounded up to one significant digit:
# 7e-7, which leaves room for another ROCm release's sinf / sqrtf
PF_MEASURED = 1.571e-7


def one_digit_up(v: float) -> float:
    e = 10.0 ** math.floor(math.log10(v))
    return float(f"{math.ceil(v / e) * e:.0e}")


PF_BAR = one_digit_up(4 * PF_MEASURED)


@functools.lru_cache(maxsize=None)
def frames(name, s):
    """the float64 chain's per-frame intermediates of slot s's clip -- computed once, shared, never modified"""
    o, _, clips, _ = setup(name)
    return P.frames64(o, clips[s])


@functools.lru_cache(maxsize=None)
def want(name, s, tau, kind):
    return P.e64_pf(frames(name, s), tau, kind)


@functools.lru_cache(maxsize=None)
def plain_outputs(name, way, precision="f32"):
    _, m, clips, _ = setup(name)
    return drive(server(m, precision=precision), clips, WAYS[way])


# ---- 1. the pointwise kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
def test_post_filter_against_float64(kind):
    from cruse_amd import ops
    POISON, PAD = 777.0, 36
    gen = torch.Generator().manual_seed(5)
    for n in (1, 63, 161, 4099):
        g = torch.rand(n, generator=gen)
        g[0] = 1.0
        g[-1] = 0.0
        for off in (0, 1):                                            # an aligned output (16-byte path from n = 4) and a misaligned one
            for tau in (0.0, 0.02, 0.5):
                buf = torch.full((n + 2 * PAD + 4,), POISON, device="cuda")
                src = torch.zeros(n + 4, device="cuda")
                m, out = src[off:off + n], buf[PAD + off:PAD + off + n]
                m.copy_(g)
                assert ops.post_filter(m, tau, kind, out=out) is out
                got = buf.cpu()
                assert bool((got[:PAD + off] == POISON).all()) and bool((got[PAD + off + n:] == POISON).all()), (n, off, tau)
                res = got[PAD + off:PAD + off + n]
                if tau == 0.0:
                    assert torch.equal(res, g), (n, off)
                else:
                    err = float((res.double() - torch.from_numpy(P.pf(g.double().numpy(), tau, kind))).abs().max())
                    assert err <= PF_BAR, (n, off, tau, err)
    # a [3,1,5,160] mask with a tau per clip; in place as well
    mask = torch.rand(3, 1, 5, 160, generator=gen)
    taus = torch.tensor(TAUS)
    got = ops.post_filter(mask.cuda(), taus.cuda(), kind).cpu()
    for b in range(3):
        ref = torch.from_numpy(P.pf(mask[b].double().numpy(), float(taus[b].double()), kind))
        err = float((got[b].double() - ref).abs().max())
        assert err <= PF_BAR and (TAUS[b] != 0.0 or torch.equal(got[b], mask[b])), (b, err)
    inplace = mask.cuda()
    ops.post_filter(inplace, taus.cuda(), kind, out=inplace)
    assert torch.equal(inplace.cpu(), got)
    # a tau group boundary inside a 16-byte vector: rows of 5 elements, a tau per row
    m5 = torch.rand(7, 5, generator=gen)
    t7 = torch.tensor([0.02, 0.0, 0.5, 0.1, 0.0, 0.3, 0.02])
    got = ops.post_filter(m5.cuda(), t7.cuda(), kind).cpu()
    for r in range(7):
        ref = torch.from_numpy(P.pf(m5[r].double().numpy(), float(t7[r].double()), kind))
        assert float((got[r].double() - ref).abs().max()) <= PF_BAR, r
    # the sweep: the figure PF_BAR is derived from, and the properties that survive float32
    sw = torch.from_numpy(P.sweep(4097)).float()
    for tau in (0.02, 0.5):
        res = ops.post_filter(sw.cuda(), tau, kind).cpu()
        err = float((res.double() - torch.from_numpy(P.pf(sw.double().numpy(), tau, kind))).abs().max())
        print(f"post_filter {kind} tau {tau}: worst abs error on the 4097-gain sweep {err:.3e} (measured {PF_MEASURED:.1e}, bar {PF_BAR:.0e})")
        assert err <= PF_BAR, (kind, tau, err)
        assert float(res[0]) == 0.0 and abs(float(res[-1]) - 1.0) <= PF_BAR and bool(torch.isfinite(res).all())
        assert bool((res <= sw + PF_BAR).all()) and bool((res[1:] - res[:-1] >= -PF_BAR).all())
    from cruse_amd.acoustics import postfilter
    shim = postfilter.postfiltering(sw.cuda(), None, 0.02) if kind == "iam" else postfilter.envelope_postfiltering(sw.cuda(), sw.cuda(), 0.02)
    assert torch.equal(shim, ops.post_filter(sw.cuda(), 0.02, kind))


# ---- 2. tau = 0 is the plain server --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_tau_zero_is_the_plain_server(name):
    _, m, clips, _ = setup(name)
    plain, pf = server(m), server(m, post_filter="iam")
    assert plain.pf is None and pf.pf.dtype == torch.float32 and pf.pf.shape == (S,) and float(pf.pf.abs().sum()) == 0.0
    mo = pf.lay["wk_mask"]
    for way in ("pushes", "push+packets"):
        a, b = drive(plain, clips, WAYS[way]), drive(pf, clips, WAYS[way])
        for s in range(S):
            assert a[s].shape == (L,) and torch.equal(a[s], b[s]), (name, way, s)
            assert torch.equal(plain.stage(s)["mask"], pf.stage(s)["mask"])
        assert torch.equal(plain.work[:, mo:mo + 160], pf.work[:, mo:mo + 160])
        assert torch.equal(plain.pwork[:, :, mo:mo + 160], pf.pwork[:, :, mo:mo + 160])
    assert torch.equal(plain.enhance(clips), pf.enhance(clips))


# ---- 3. per-slot tau against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_per_slot_tau_against_the_reference(name, kind, precision):
    """f32: against the float64 reference within BAR.  f16 rounds the GRU operands, so BAR against float64 is not its bar (tests/
    test_gpu_stream_io.py compares that mode with its own float instance only): there the slot with tau = 0 is bit-equal to the plain f16
    server and the filtered slots differ from it."""
    _, m, clips, _ = setup(name)
    inf = server(m, precision=precision, post_filter=kind)
    inf.set_post_filter(list(TAUS))
    assert inf.pf.cpu().tolist() == [np.float32(t) for t in TAUS]
    mo = inf.lay["wk_mask"]
    for way, calls in WAYS.items():
        a, b = plain_outputs(name, way, precision), drive(inf, clips, calls)
        for s in range(S):
            assert b[s].shape == (L,)
            if precision == "f32":
                err = rel_l2(b[s], want(name, s, TAUS[s], kind))
                print(f"{name} {kind} {way} slot {s} tau {TAUS[s]}: vs R {err:.2e}")
                assert err <= BAR, (name, kind, way, s, err)
            if TAUS[s] == 0.0:
                assert torch.equal(a[s], b[s]), (name, kind, way, s)
            else:
                d, d64 = rel_l2(b[s], a[s]), rel_l2(want(name, s, TAUS[s], kind), want(name, s, 0.0, kind))
                print(f"{name} {kind} {precision} {way} slot {s} tau {TAUS[s]}: vs the plain server {d:.2e} (float64 reference: {d64:.2e})")
                assert d > 1e-3, (name, kind, way, s, d, d64)
    got = inf.enhance(clips).cpu()                                        # enhance() keeps the slots' tau: it survives reset / flush
    assert inf.pf.cpu().tolist() == [np.float32(t) for t in TAUS]
    if precision == "f32":
        for s in range(S):
            err = rel_l2(got[s], want(name, s, TAUS[s], kind))
            print(f"{name} {kind} enhance slot {s} tau {TAUS[s]}: vs R {err:.2e}")
            assert err <= BAR, (name, kind, s, err)
        plain = server(m)
        drive(plain, clips, PUSH_PACKETS, flush=False)
        drive(inf, clips, PUSH_PACKETS, flush=False)
        assert torch.equal(plain.pwork[:, :, mo:mo + 160], inf.pwork[:, :, mo:mo + 160])     # the mask rows keep the raw mask
        for s in range(S):
            assert torch.equal(plain.stage(s)["mask"], inf.stage(s)["mask"])


# ---- 4. tau changed mid-clip under a captured graph ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_tau_changed_mid_clip_keeps_the_graphs(name):
    """As test_limit_changed_mid_clip_keeps_the_graphs: tau changes after block 5; output block b overlap-adds frames b and b + 1, so blocks
    0..4 belong to the old tau, blocks 6..11 to the new one, and block 5 to neither."""
    _, m, clips, _ = setup(name)
    old, new = [0.02, 0.0, 0.3], [0.0, 0.1, 0.02]
    ways = {"pushes": ([("p", [True] * S)] * 6, [("p", [True] * S)] * 6),
            "packets": ([("k", [4] * S), ("k", [2] * S)], [("k", [4] * S), ("k", [2] * S)])}
    for way, (first, second) in ways.items():
        inf = server(m, post_filter="iam")
        inf.set_post_filter(old)
        graphs = {}

        def after(i):
            if i == len(first) - 1:
                graphs["before"] = sorted(map(str, inf._graphs))
                inf.set_post_filter(new)
            if i == len(first) + len(second) - 1:
                graphs["after"] = sorted(map(str, inf._graphs))

        got = drive(inf, clips, first + second, after=after)
        assert len(graphs["before"]) == 2 and graphs["after"] == graphs["before"], (way, graphs)
        for s in range(S):
            r_old, r_new = want(name, s, old[s], "iam"), want(name, s, new[s], "iam")
            e_old, e_new = rel_l2(got[s][:5 * 160], r_old[:5 * 160]), rel_l2(got[s][6 * 160:], r_new[6 * 160:])
            cross = rel_l2(got[s][6 * 160:], r_old[6 * 160:])
            print(f"{name} {way} slot {s}: blocks 0..4 vs R(old) {e_old:.2e}, blocks 6..11 vs R(new) {e_new:.2e} (vs R(old) {cross:.2e})")
            assert got[s].shape == (L,) and e_old <= BAR and e_new <= BAR, (name, way, s, e_old, e_new)
            assert cross > 1e-3                                           # the change is visible


# ---- 5. with the attenuation limit and PCM out -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
def test_with_a_limit_and_pcm_out(kind):
    name = "hg20_g1"
    o, m, _, _ = setup(name)
    v = torch.stack([IO.pcm_noise(L, 400 + s) for s in range(S)])          # int16, about -12 dBFS
    x = v.float() / 32768.0
    ref = []
    for s in range(S):
        e = P.e64_pf(P.frames64(o, x[s]), TAUS[s], kind)
        ref.append(IO.quantise(P.mix(x[s], e, IO.gain(IO.LIMS_DB[s])).float().numpy()))
    for way in ("pushes", "push+packets"):
        inf = server(m, post_filter=kind, atten_lim=True, pcm_out=True)
        inf.set_post_filter(list(TAUS))
        inf.set_atten_lim(list(IO.LIMS_DB))
        q = drive(inf, x, WAYS[way])
        n = inf.clipped()
        for s in range(S):
            wq, wc = ref[s]
            assert q[s].dtype == torch.int16 and q[s].shape == (L,)
            d = np.abs(q[s].numpy().astype(np.int64) - wq.astype(np.int64))
            print(f"{kind} {way} slot {s}: vs the quantised float64 reference {int((d == 0).sum())} of {L} equal, worst {int(d.max())} LSB; "
                  f"clipped() {int(n[s])}, the reference clamps {int(wc.sum())}")
            assert d.max() <= 1, (kind, way, s, int(d.max()))
            sat = int(((q[s] == 32767) | (q[s] == -32768)).sum())
            assert n[s] <= sat and abs(int(n[s]) - int(wc.sum())) <= int((d != 0).sum()), (s, int(n[s]), sat, int(wc.sum()))


# ---- 6. another I/O rate ------------------------------------------------------------------------------------------------------------------------
def test_forty_eight_kilohertz():
    from tests import stream_rs_ref as RS
    from tests import test_gpu_stream_rs as T
    name, rate = "hg20_g1", 48000
    o64, m = T.model(name)
    clips = T.clips_at(rate)
    inf = T.server(m, io_rate=rate, post_filter="iam")
    inf.set_post_filter(list(TAUS))
    plain = T.drive(T.server(m, io_rate=rate), clips, T.PUSH_PACKETS)
    got = T.drive(inf, clips, T.PUSH_PACKETS)
    for s in range(S):
        r = RS.resample_out(P.e64_pf(P.frames64(o64, RS.resample_in(clips[s], rate)), TAUS[s], "iam"), rate)
        err = rel_l2(got[s], r)
        print(f"48 kHz slot {s} tau {TAUS[s]}: vs Out(E_pf(In(u))) {err:.2e}")
        assert got[s].shape == (IO.NB * 480,) and err <= T.BAR, (s, err)
        assert torch.equal(got[s], plain[s]) == (TAUS[s] == 0.0)


# ---- 7. offline ---------------------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())


def test_offline_inferencer_and_evaluate(tmp_path):
    from cruse_amd import ops
    from cruse_amd.acoustics import feature
    from cruse_amd.evaluate import evaluate_files
    from cruse_amd.inferencer import Inferencer
    from cruse_amd.loss import enhanced_spectrum
    from oracle import cruse_oracle as O
    name, tau = "g4", 0.05
    _, m, clips, _ = setup(name)
    x = clips.cuda()
    off = Inferencer(m, post_filter="iam", pf_tau=tau)
    got = off.mag_mask_to_wave(x)
    with torch.no_grad():
        spec = feature.pre_stft(x, 320, 160, 320, f_net=160)
        mask = m(spec["mag_net"])
        est = enhanced_spectrum(ops.post_filter(mask.contiguous(), tau, "iam"), spec["real"].squeeze(1), spec["imag"].squeeze(1))
        by_hand = feature.istft_ri(est[..., 0], est[..., 1], 320, 160, length=x.shape[-1])
    assert torch.equal(got, by_hand)
    assert torch.equal(Inferencer(m, post_filter=None).mag_mask_to_wave(x), Inferencer(m).mag_mask_to_wave(x))
    assert torch.equal(Inferencer(m, post_filter="iam", pf_tau=0.0).mag_mask_to_wave(x), Inferencer(m).mag_mask_to_wave(x))
    inf = server(m, post_filter="iam")
    inf.set_post_filter(tau)
    st = inf.enhance(clips).cpu()
    for s in range(S):
        e_pair, e_ref = rel_l2(st[s], got[s].cpu()), rel_l2(got[s].cpu(), want(name, s, tau, "iam"))
        print(f"{name} clip {s} tau {tau}: enhance() vs Inferencer {e_pair:.2e}; Inferencer vs R {e_ref:.2e}")
        assert e_pair <= BAR and e_ref <= BAR, (s, e_pair, e_ref)
    clean, noisy = [], []
    for k, n in enumerate((4000, 4800)):
        nz, c = O.synth_pair(1, n, seed=40 + k)
        for side, w, lst in (("clean", c, clean), ("noisy", nz, noisy)):
            lst.append(str(tmp_path / f"{side}{k}.wav"))
            _write_wav(lst[-1], w[0].numpy())
    a = evaluate_files(m, clean, noisy, metrics=["SI_SDR"], batch_size=1)
    b = evaluate_files(m, clean, noisy, metrics=["SI_SDR"], batch_size=1, post_filter="iam", pf_tau=0.2)
    print(f"SI_SDR enhanced: unfiltered {a['scores']['SI_SDR']['Enhanced'].tolist()}, iam tau 0.2 {b['scores']['SI_SDR']['Enhanced'].tolist()}")
    assert np.array_equal(a["scores"]["SI_SDR"]["Noisy"], b["scores"]["SI_SDR"]["Noisy"])
    assert (a["scores"]["SI_SDR"]["Enhanced"] != b["scores"]["SI_SDR"]["Enhanced"]).all()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from cruse_amd import _lib, ops
    from cruse_amd.inferencer import Inferencer, StreamingInferencer
    _, m, _, _ = setup("hg20_g1")
    for build in (lambda: Inferencer(m, head="df", post_filter="iam"), lambda: StreamingInferencer(m, S, head="df", post_filter="envelope")):
        with pytest.raises(ValueError, match="filter field"):
            build()
    for build in (lambda: Inferencer(m, post_filter="irm"), lambda: StreamingInferencer(m, S, post_filter="IAM"),
                  lambda: ops.post_filter(torch.zeros(4, device="cuda"), 0.02, "other")):
        with pytest.raises(ValueError, match="kind"):
            build()
    with pytest.raises(ValueError, match="non-negative"):
        Inferencer(m, post_filter="iam", pf_tau=-0.1)
    plain = server(m)
    with pytest.raises(ValueError, match="post_filter"):
        plain.set_post_filter(0.02)
    inf = server(m, post_filter="iam")
    inf.set_post_filter([0.02, 0.1, 0.3])
    before = inf.pf.clone()
    for bad in (-0.02, float("nan"), [0.02, -1.0, 0.02]):
        with pytest.raises(ValueError, match="non-negative"):
            inf.set_post_filter(bad)
    with pytest.raises(ValueError, match="values for"):
        inf.set_post_filter([0.1, 0.1], [0, 1, 2])
    with pytest.raises(ValueError, match="out of range"):
        inf.set_post_filter(0.1, [S])
    assert torch.equal(inf.pf, before) and not inf._graphs
    out = torch.full((8,), 5.0, device="cuda")
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="non-negative"):
            ops.post_filter(torch.rand(8, device="cuda"), bad, "iam", out=out)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.post_filter(torch.rand(8, device="cuda", requires_grad=True), 0.02, "iam", out=out)
    # the C entry points: a kind outside {1, 2}, a null pf_tau, negative sizes
    lib, lay, play = _lib.lib, ops.stream_layout(m.ch), ops.stream_packet_layout(m.ch)
    z = lambda n, dt=torch.float32: torch.zeros(n, device="cuda", dtype=dt)
    ctl, tab, w = z(2 * S, torch.int32), ops.stream_tables("cuda"), z(lay["wtotal"])
    ctl[:S] = ops.STREAM_FRAME                                             # would compute if it were launched
    ctl[S:] = 1
    state, work, pwork = z(S * lay["st_stride"]), z(S * lay["wk_stride"]), z(S * (K + 1) * play["wk_stride"])
    io, taus = z(S * K * 160), z(S)
    p = lambda t: t.data_ptr()
    ch = [int(c) for c in m.ch]
    for kind, tp, msg in ((0, p(taus), b"post-filter kind 0"), (3, p(taus), b"post-filter kind 3"), (1, None, b"null pf_tau")):
        assert lib.cruse_stream_decode_pf(p(ctl), S, *ch, p(tab), p(w), 1e-5, p(state), p(work), p(io), 0, None, None, kind, tp, None) != 0
        assert b"cruse_stream_decode_pf" in lib.cruse_last_error() and msg in lib.cruse_last_error()
        assert lib.cruse_stream_decode_n_pf(p(ctl), S, K, K, K + 1, *ch, p(tab), p(w), 1e-5, p(state), p(pwork), p(io), 0, None, None, kind, tp,
                                            None) != 0
        assert b"cruse_stream_decode_n_pf" in lib.cruse_last_error() and msg in lib.cruse_last_error()
    assert lib.cruse_stream_decode_pf(p(ctl), -1, *ch, p(tab), p(w), 1e-5, p(state), p(work), p(io), 0, None, None, 1, p(taus), None) != 0
    src = torch.rand(8, device="cuda")
    for args in ((0, p(src), 1, 8, p(taus), 0, p(out)), (3, p(src), 1, 8, p(taus), 0, p(out)), (1, p(src), 1, 8, None, 0, p(out)),
                 (1, p(src), -1, 8, p(taus), 0, p(out)), (1, p(src), 1, -8, p(taus), 0, p(out)), (1, p(src), 1, 8, p(taus), -1, p(out)),
                 (1, p(src), 1, 8, p(taus), 2, p(out)), (1, None, 1, 8, p(taus), 0, p(out)), (1, p(src), 1, 8, p(taus), 0, None)):
        assert lib.cruse_mask_postfilter(*args, None) != 0, args
        assert b"mask_postfilter" in lib.cruse_last_error()
    torch.cuda.synchronize()
    for t in (state, work, pwork, io):
        assert float(t.abs().sum()) == 0.0                                 # nothing was launched
    assert bool((out == 5.0).all())


# ---- 9. graph replay equals eager launches ------------------------------------------------------------------------------------------------------
def test_graph_equals_eager():
    _, m, clips, _ = setup("hg20_g1")
    outs = []
    for use_graph in (True, False):
        inf = server(m, post_filter="envelope", atten_lim=True, use_graph=use_graph)
        inf.set_post_filter(list(TAUS))
        inf.set_atten_lim(list(IO.LIMS_DB))
        outs.append(drive(inf, clips, PUSH_PACKETS) + [inf.enhance(clips).cpu()])
        assert bool(inf._graphs) == use_graph
    for a, b in zip(*outs):
        assert torch.equal(a, b)
