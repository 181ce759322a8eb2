"""MI355X: the level meters and the voice-activity detector at the end of the streaming chains (cruse_stream_meter / _meter_n,
csrc/stream_meter.hip; StreamingInferencer(meters=True)).

Reference: tests/stream_meter_ref.py in float64 on the same f32 rows -- synthetic work rows at the kernel level, the rows stage() shows at
the server level.  Bars (derived in stream_meter_ref.py from f32 sums of <= 322 non-negative terms and a logistic of slope <= 0.25 per
dB): 1e-3 dB on the levels, 1e-3 on p, vad equal on every frame with no exception allowed; tests/test_stream_meter_host.py holds the
committed inputs at least 1e-3 away from the threshold, which makes the last one safe.

Measured on MI355X (the prints below): levels within 2.0e-5 dB (of at most 120), p within 2.1e-7 at the kernel level; levels within 6.6e-6 dB,
p within 3.8e-7 at the server level; 64 slots with meters 227 us per push."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import stream_meter_ref as M
from tests.test_gpu_stream_packets import even_sizes
from tests.test_gpu_streaming import models

pytestmark = pytest.mark.gpu

S = M.S
LAY = dict(wk_re=4, wk_im=172, wk_mask=340)                   # a work row of the kernel-level tests: the three rows, gaps between them
WS = 512
POISON = 777.25


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def compare(got, want, what):
    """got, want [n, 4]: (max level error in dB, max p error); asserts the bars and vad on every frame"""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not len(want):
        return 0.0, 0.0
    assert np.isfinite(got).all(), what
    e_db, e_p = float(np.abs(got[:, :2] - want[:, :2]).max()), float(np.abs(got[:, 2] - want[:, 2]).max())
    assert e_db <= M.BAR_DB and e_p <= M.BAR_P, (what, e_db, e_p)
    assert np.array_equal(got[:, 3], want[:, 3]), (what, got[:, 3], want[:, 3])
    return e_db, e_p


# ---- 1. the kernels, through ops.stream_meter / _n ---------------------------------------------------------------------------------------
def work_row(row):
    w = np.zeros(WS, dtype=np.float32)
    for k, v in zip(("wk_re", "wk_im", "wk_mask"), row):
        w[LAY[k]:LAY[k] + len(v)] = v
    return w


class Bench:
    """the tensors of a kernel-level call for S slots"""

    def __init__(self, form, hops=0):
        from cruse_amd import ops
        self.ops = ops
        _, lim, kind, tau = form
        d = M.DEFAULTS
        self.tab = ops.stream_tables("cuda")
        self.par = torch.tensor([[d["level_db"], d["threshold"], d["attack"], d["release"]]] * S, dtype=torch.float64).float().cuda()
        self.state = torch.zeros(S, ops.stream_meter_layout()["stride"], device="cuda")
        self.acc = torch.zeros(S, 4, device="cuda", dtype=torch.float64)
        self.lim = None if lim is None else torch.full((S,), lim, dtype=torch.float64).float().cuda()
        self.pf = None if kind == 0 else (kind, torch.full((S,), tau, dtype=torch.float64).float().cuda())
        self.hops = hops
        self.out = torch.full((S, max(hops, 1), 4), POISON, device="cuda")

    def step(self, modes, rows):
        """single hop: modes [S], rows [S] of (re, im, mask) or None -> out [S, 4] on the host"""
        work = torch.from_numpy(np.stack([work_row(r) if r is not None else np.full(WS, POISON, dtype=np.float32) for r in rows])).cuda()
        mode = torch.tensor(modes, dtype=torch.int32, device="cuda")
        self.out.fill_(POISON)
        self.ops.stream_meter(mode, work, LAY, self.tab, self.par, self.state, self.acc, self.out[:, 0], lim=self.lim, pf=self.pf)
        torch.cuda.synchronize()
        return self.out[:, 0].cpu()

    def packet(self, call, frames):
        """call: (start, count) per slot; frames: per slot the list of rows -> out [S, hops, 4] on the host"""
        work = np.full((S, self.hops + 1, WS), POISON, dtype=np.float32)
        for s in range(S):
            for f, r in enumerate(frames[s]):
                work[s, f] = work_row(r)
        pk = torch.tensor([[c[0] for c in call], [c[1] for c in call]], dtype=torch.int32, device="cuda")
        self.out.fill_(POISON)
        self.ops.stream_meter_n(pk, self.hops, torch.from_numpy(work).cuda(), LAY, self.tab, self.par, self.state, self.acc, self.out,
                                lim=self.lim, pf=self.pf)
        torch.cuda.synchronize()
        return self.out.cpu()

    def activity(self):
        acc = self.acc.cpu().numpy()
        n = np.maximum(acc[:, 1], 1.0)
        return np.concatenate([acc[:, :2], 10.0 * np.log10(acc[:, 2:] / n[:, None] + 1e-12)], axis=1)


def check_activity(got, meters, what):
    for s, m in enumerate(meters):
        want = m.activity()
        assert np.array_equal(got[s, :2], want[:2]) and np.abs(got[s, 2:] - want[2:]).max() <= M.BAR_DB, (what, s, got[s], want)


@pytest.mark.parametrize("form", M.KERNEL_FORMS, ids=[f[0] for f in M.KERNEL_FORMS])
def test_single_hop_kernel_against_float64(form):
    from cruse_amd import ops
    _, lim, kind, tau = form
    T = M.KERNEL_FRAMES
    streams = [M.kernel_slot_rows(s)[:T] for s in range(S)]
    b = Bench(form)
    b.state.fill_(0.9)                                        # FRAME0 resets whatever the state and the accumulators held
    b.acc.fill_(5.0)
    got = []
    for t in range(T):
        mode = ops.STREAM_FRAME0 if t == 0 else ops.STREAM_END if t == T - 1 else ops.STREAM_FRAME
        out = b.step([mode] * S, [streams[s][t] for s in range(S)])
        if t == 0:
            assert bool((out == POISON).all())                # frame 0 writes no row
        else:
            got.append(out)
    got = torch.stack(got, dim=1).numpy()                     # [S, T - 1, 4]
    worst = (0.0, 0.0)
    meters = []
    for s in range(S):
        want, m = M.meter_clip(streams[s], lim=lim, tau=tau, kind=kind)
        meters.append(m)
        worst = tuple(max(a, e) for a, e in zip(worst, compare(got[s], want, (form[0], s))))
    check_activity(b.activity(), meters, form[0])
    print(f"single hop {form[0]}: levels within {worst[0]:.2e} dB, p within {worst[1]:.2e}")


@pytest.mark.parametrize("case", list(M.KERNEL_PACKETS))
def test_packet_kernel_against_float64(case):
    calls = M.KERNEL_PACKETS[case]
    worst = (0.0, 0.0)
    for form in M.KERNEL_FORMS:
        plan, meters = M.run_packet_case(calls, form)
        b = Bench(form, hops=M.KERNEL_HOPS)
        for call, per in zip(calls, plan):
            out = b.packet(call, [p[0] for p in per]).numpy()
            for s, (_, _, want) in enumerate(per):
                worst = tuple(max(a, e) for a, e in zip(worst, compare(out[s, :len(want)], want, (case, form[0], s))))
                assert (out[s, len(want):] == POISON).all(), (case, form[0], s)     # rows beyond the slot's frame count keep their poison
        check_activity(b.activity(), meters, (case, form[0]))
    print(f"packets {case}: levels within {worst[0]:.2e} dB, p within {worst[1]:.2e}")


def test_a_frame_has_the_same_bits_from_both_kernels():
    from cruse_amd import ops
    form = M.KERNEL_FORMS[5]                                  # limit and post-filter
    streams = [M.kernel_slot_rows(s)[:9] for s in range(S)]
    one, pkt = Bench(form), Bench(form, hops=4)
    rows = [one.step([ops.STREAM_FRAME0 if t == 0 else ops.STREAM_FRAME] * S, [streams[s][t] for s in range(S)]) for t in range(9)]
    a = torch.stack(rows[1:], dim=1)                          # [S, 8, 4]
    first = pkt.packet([(1, 4)] * S, [streams[s][:5] for s in range(S)])
    second = pkt.packet([(2, 4)] * S, [streams[s][5:9] for s in range(S)])
    assert torch.equal(bits(a), bits(torch.cat([first, second], dim=1)))
    assert torch.equal(bits(one.acc.cpu()), bits(pkt.acc.cpu())) and torch.equal(bits(one.state.cpu()), bits(pkt.state.cpu()))


def test_nothing_is_written_where_nothing_ran():
    from cruse_amd import ops
    form = M.KERNEL_FORMS[0]
    rows = [M.kernel_slot_rows(s)[5] for s in range(S)]
    # single hop: SKIP and STORE slots beside a FRAME slot
    b = Bench(form)
    b.state.fill_(POISON)
    b.acc.fill_(POISON)
    b.state[2].fill_(0.25)
    b.acc[2].zero_()
    out = b.step([ops.STREAM_SKIP, ops.STREAM_STORE, ops.STREAM_FRAME], rows)
    assert bool((out[:2] == POISON).all()) and bool((b.state[:2] == POISON).all()) and bool((b.acc[:2] == POISON).all())
    assert bool((out[2] != POISON).all()) and float(b.acc[2, 0]) == 1.0 and bool((b.state[2, 1:] == 0.25).all())
    # packets: a slot with no block, a slot that only stores its first block, a slot with two frames
    b = Bench(form, hops=4)
    b.state.fill_(POISON)
    b.acc.fill_(POISON)
    b.state[2].fill_(0.25)
    b.acc[2].zero_()
    out = b.packet([(2, 0), (0, 1), (2, 2)], [[], [], [rows[2], rows[0]]])
    assert bool((out[:2] == POISON).all()) and bool((b.state[:2] == POISON).all()) and bool((b.acc[:2] == POISON).all())
    assert bool((out[2, :2] != POISON).all()) and bool((out[2, 2:] == POISON).all()) and float(b.acc[2, 0]) == 2.0


# ---- 2. the server -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(name):
    return models(M.CONFIGS[name])


@functools.lru_cache(maxsize=None)
def clips(L):
    return torch.stack([M.clip(L, i) for i in range(S)])


def server(name, form=M.SERVER_FORMS[0], n=S, meters=True, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    _, vad, lim_db, pf = form
    inf = StreamingInferencer(pair(name)[1], n, meters=meters, atten_lim=lim_db is not None, post_filter=None if pf is None else pf[0], **kw)
    if lim_db is not None:
        inf.set_atten_lim(lim_db)
    if pf is not None:
        inf.set_post_filter(pf[1])
    if vad and meters:
        inf.set_vad(**vad)
    return inf


def stage_rows(inf, s, frame=-1):
    st = inf.stage(s, frame)
    return tuple(st[k].double().cpu().numpy() for k in ("re", "im", "mask"))


def frame0_rows(name, x):
    """the rows of frame 0 of every slot, which a push's second chain overwrites: the same two single-hop chains on a fresh instance,
    stopped after the first (the raw mask does not depend on a limit or a post-filter)"""
    from cruse_amd import ops
    inf = server(name, meters=False, use_graph=False)
    inf.blocks.copy_(x[:, :160])
    inf.mode[1].fill_(ops.STREAM_STORE)
    inf._chain(1)
    inf.blocks.copy_(x[:, 160:320])
    inf.mode[0].fill_(ops.STREAM_FRAME0)
    inf._chain(0)
    torch.cuda.synchronize()
    return [stage_rows(inf, s) for s in range(S)]


def run(inf, name, x, sizes, at=None, then=None):
    """x [S, L] through calls of the given sizes ("p": a push, an int c: a packet of c blocks), then flush; `then()` runs once `at` blocks
    are in.  -> (audio [S, L], meter rows [S, nb, 4] as the calls returned them, the rows (re, im, mask) of frames 0..nb per slot)"""
    n, L = x.shape
    nb = L // 160
    blocks = x.view(n, nb, 160).cuda()
    audio, met, rows = ([[] for _ in range(n)] for _ in range(3))
    b = 0
    for c in sizes:
        if at is not None and b == at:
            then()
        if c == "p":
            out, valid = inf.push(blocks[:, b])
            torch.cuda.synchronize()
            m = inf.last_meters().cpu()
            for s in range(n):
                if b == 1:
                    rows[s].append(None)
                if b >= 1:
                    rows[s].append(stage_rows(inf, s))
                if valid[s]:
                    audio[s].append(out[s].cpu())
                    met[s].append(m[s, 0])
            b += 1
        else:
            out, n_out = inf.push_packet(blocks[:, b:b + c])
            torch.cuda.synchronize()
            m = inf.last_meters().cpu()
            for s in range(n):
                rows[s] += [stage_rows(inf, s, f) for f in range(int(inf._last_frames[s]))]
                audio[s] += [out[s, k].cpu() for k in range(int(n_out[s]))]
                met[s] += [m[s, k] for k in range(int(n_out[s]))]
            b += c
    assert b == nb
    last = inf.flush(list(range(n))).cpu()
    m = inf.last_meters().cpu()
    f0 = None
    for s in range(n):
        rows[s].append(stage_rows(inf, s))
        audio[s].append(last[s])
        met[s].append(m[s, 0])
        if rows[s][0] is None:
            f0 = frame0_rows(name, x.cuda()) if f0 is None else f0
            rows[s][0] = f0[s]
        assert len(rows[s]) == nb + 1 and len(met[s]) == nb == len(audio[s])    # one meter row per block returned
    return torch.stack([torch.cat(a) for a in audio]), torch.stack([torch.stack(r) for r in met]), rows


def check_run(met, rows, kw, what):
    worst = (0.0, 0.0)
    meters = []
    for s in range(S):
        want, m = M.meter_clip(rows[s], **kw)
        meters.append(m)
        worst = tuple(max(a, e) for a, e in zip(worst, compare(met[s].numpy(), want, (what, s))))
    return worst, meters


@pytest.mark.parametrize("L", M.LENGTHS)
@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_server_rows_equal_the_reference_on_the_staged_rows(name, L):
    x = clips(L)
    nb = L // 160
    runs = {"push": (server(name), ["p"] * nb)}
    inf = server(name, max_hops=4)
    for K in (1, 2, 3, 4):
        runs[f"packets of {K}"] = (inf, even_sizes(nb, K))
    runs["pushes and packets"] = (inf, (["p", 3, "p", 4, 1] if nb == 10 else ["p"] + even_sizes(nb - 1, 2)))
    plain = server(name, meters=False, max_hops=4)
    res = {}
    for tag, (srv, sizes) in runs.items():
        audio, met, rows = run(srv, name, x, sizes)
        worst, meters = check_run(met, rows, {}, (name, L, tag))
        check_activity(srv.activity(), meters, (name, L, tag))                 # flush keeps the clip's accumulators
        print(f"{name} L {L} {tag}: levels within {worst[0]:.2e} dB, p within {worst[1]:.2e}; activity {srv.activity()[0].round(2).tolist()}")
        res[tag] = (audio, met)
        if tag != "push":                                                       # the audio of a server without meters, bit for bit
            assert torch.equal(bits(audio), bits(run_audio(plain, x, sizes))), tag
    for K in (None, 3):
        waves, met = inf.enhance(x.cuda(), hops=K, with_meters=True)
        audio, want = res[f"packets of {4 if K is None else K}"]
        assert met.shape == (S, nb, 4) and torch.equal(bits(met.cpu()), bits(want)) and torch.equal(bits(waves.cpu()), bits(audio)), K
        assert torch.equal(bits(inf.enhance(x.cuda(), hops=K).cpu()), bits(audio))
    assert torch.equal(bits(res["push"][0]), bits(run_audio(server(name, meters=False), x, ["p"] * nb)))


def run_audio(inf, x, sizes):
    from tests.test_gpu_stream_packets import run_packets
    return run_packets(inf, x, sizes)


@pytest.mark.parametrize("form", M.SERVER_FORMS[1:], ids=[f[0] for f in M.SERVER_FORMS[1:]])
def test_limit_post_filter_and_detector_settings_enter_the_rows(form):
    for name, L, sizes, hops in (("small_g2", 1600, ["p"] * 10, 1), ("small_g2", 1600, [3, 3, 3, 1], 4), ("g4", 480, [3], 4)):
        inf = server(name, form, max_hops=hops)
        _, met, rows = run(inf, name, clips(L), sizes)
        worst, _ = check_run(met, rows, M.form_kwargs(form), (form[0], name, L, sizes))
        print(f"{form[0]} {name} L {L} {sizes}: levels within {worst[0]:.2e} dB, p within {worst[1]:.2e}")
        if form[0] == "lim0":                                 # a limit of 0 dB passes the input: L_out = L_in
            assert float((met[..., 1] - met[..., 0]).abs().max()) <= M.BAR_DB
        else:
            assert float((met[..., 0] - met[..., 1]).min()) > 1.0             # the model removes something: this is not the input's level


def test_graph_replay_equals_eager_launches():
    x = clips(1600)
    for sizes, hops in ((["p"] * 10, 1), ([4, 4, 2], 4)):
        a, b = (server("small_g2", use_graph=g, max_hops=hops) for g in (True, False))
        ra, rb = run(a, "small_g2", x, sizes), run(b, "small_g2", x, sizes)
        assert torch.equal(bits(ra[0]), bits(rb[0])) and torch.equal(bits(ra[1]), bits(rb[1]))
        assert np.array_equal(a.activity(), b.activity())


def test_set_vad_and_set_atten_lim_change_later_rows_without_a_new_capture():
    name, x = "small_g2", clips(1600)
    inf = server(name, ("switch", {}, float("inf"), None))
    seen = {}

    def change():
        seen["graphs"] = dict(inf._graphs)
        inf.set_vad(**M.SWITCH_VAD)
        inf.set_atten_lim(M.SWITCH_LIM_DB)

    _, met, rows = run(inf, name, x, ["p"] * 10, at=M.SWITCH_AT, then=change)
    assert seen["graphs"] and seen["graphs"].keys() == inf._graphs.keys() and all(inf._graphs[k] is g for k, g in seen["graphs"].items())
    for s in range(S):
        m = M.Meter(lim=0.0)
        a, _ = M.meter_clip(rows[s][:M.SWITCH_AT], meter=m)
        m.set(lim=10.0 ** (-M.SWITCH_LIM_DB / 20.0), **M.SWITCH_VAD)
        b, _ = M.meter_clip(rows[s][M.SWITCH_AT:], first=M.SWITCH_AT, meter=m)
        compare(met[s].numpy(), np.concatenate([a, b]), ("switch", s))
    # one value per listed slot; a parameter that is not given stays
    inf.set_vad(threshold=[0.2, 0.3], slots=[2, 0])
    par = inf.vad_par.cpu()
    assert par[:, 1].tolist() == pytest.approx([0.3, 0.4, 0.2]) and par[:, 0].tolist() == [-45.0] * 3
    with pytest.raises(ValueError, match="attack"):
        inf.set_vad(attack=0.0)
    with pytest.raises(ValueError, match="meters=True"):
        server(name, meters=False).set_vad(threshold=0.5)


def test_silence_reads_minus_120_and_never_nan():
    inf = server("small_g2", max_hops=4)
    x = torch.zeros(S, 1600)
    for sizes in (["p"] * 10, [4, 4, 2]):
        _, met, _ = run(inf, "small_g2", x, sizes)
        assert bool(torch.isfinite(met).all()) and float((met[..., :2] + 120.0).abs().max()) <= M.BAR_DB
        assert float(met[..., 2].abs().max()) <= M.BAR_P and bool((met[..., 3] == 0).all())
        act = inf.activity()
        assert np.isfinite(act).all() and act[:, 0].tolist() == [10.0] * S and act[:, 1].tolist() == [0.0] * S and (act[:, 2:] == -120.0).all()


def test_activity_is_identical_for_every_split_and_reset_clears_it():
    x = clips(1600)
    inf = server("small_g2", max_hops=4)                      # (the default detector finds active frames in this model's output)
    got = []
    for sizes in ([4, 4, 2], [3, 3, 3, 1], [1] * 10, [2, 4, 1, 3], [1, 4, 4, 1]):
        _, met, _ = run(inf, "small_g2", x, sizes)
        got.append((met, inf.activity()))
    for met, act in got[1:]:
        assert torch.equal(bits(met), bits(got[0][0])) and np.array_equal(act, got[0][1])
    act = got[0][1]
    assert act[:, 0].tolist() == [10.0] * S and (act[:, 1] >= 1).all()
    assert np.array_equal(inf.activity(slots=[1], reset=True), act[1:2]) and inf.activity()[1].tolist() == [0.0, 0.0, -120.0, -120.0]
    inf.reset([0])
    assert inf.activity()[0].tolist() == [0.0, 0.0, -120.0, -120.0] and np.array_equal(inf.activity()[2], act[2])
    one = server("small_g2")                                  # pushes on a single-hop instance: the same for every run
    a = run(one, "small_g2", x, ["p"] * 10)
    act = one.activity()
    b = run(one, "small_g2", x, ["p"] * 10)
    assert torch.equal(bits(a[1]), bits(b[1])) and np.array_equal(act, one.activity()) and (act[:, 1] >= 1).all()


def test_head_df_refuses_meters_and_meters_off_has_no_surface():
    from cruse_amd.inferencer import StreamingInferencer
    with pytest.raises(ValueError, match="meters"):
        StreamingInferencer(pair("small_g2")[1], 1, head="df", meters=True)
    inf = server("small_g2", meters=False)
    assert not hasattr(inf, "meter_out") and not hasattr(inf, "vad_par")
    for call in (inf.last_meters, inf.activity, lambda: inf.enhance(clips(320).cuda(), with_meters=True)):
        with pytest.raises(ValueError, match="meters=True"):
            call()


def test_real_time_bound_64_slots_with_meters():
    inf = server("g4", n=64)
    blocks = 0.1 * torch.randn(64, 160, device="cuda")
    for _ in range(20):
        inf.push(blocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(400):
        inf.push(blocks)
    torch.cuda.synchronize()
    mean = (time.perf_counter() - t0) / 400
    print(f"64 slots with meters: mean push wall {mean * 1e6:.1f} us (RTF {mean / 0.01:.4f})")
    assert mean < 0.010
