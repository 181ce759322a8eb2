"""GPU: cruse_df_feat against the float64 restatement tests/df_feat_ref.py and the reference's fixture: accuracy at
the edges of the kernel's frame tile, split invariance compared as integers, states, skipped outputs, guard bands, silence and loudness,
graph capture, DfFeatures.from_wave.

The accuracy bar (the rule of DESIGN 15e / 16f): per case the kernel's maximum error against float64 may be at most 4x the error of the
same formulas evaluated by torch in float32 on the CPU, with a floor of one f32 ulp of the largest output magnitude; relative to the
case's maximum for feat_spec, absolute for feat_erb.  Every case prints both errors before it asserts."""
import functools

import numpy as np
import pytest
import torch

import df_feat_ref as R

pytestmark = pytest.mark.gpu

from cruse_amd.acoustics.df_features import TC  # noqa: E402

T_EDGES = (1, 2, TC - 1, TC, TC + 1, 2 * TC + 3)
# (F, nb_erb, min_nb_freqs, nb_df) with the erb_fb arguments (sr, fft_size) that give F bins; the second has width-1 bands
CONFIGS = {(161, 32, 2, 96): (16000, 320), (161, 24, 1, 161): (16000, 320), (161, 32, 2, 1): (16000, 320), (481, 32, 2, 96): (48000, 960)}


@functools.lru_cache(maxsize=None)
def widths_of(cfg):
    from cruse_amd.model.based_model.cust_conv import erb_fb
    F, nb_erb, mnf, _ = cfg
    w = [int(v) for v in erb_fb(*CONFIGS[cfg], nb_erb, mnf)]
    assert sum(w) == F and (cfg != (161, 24, 1, 161) or min(w) == 1)
    return tuple(w)


@functools.lru_cache(maxsize=None)
def case(B, T, cfg, alpha, scale=1.0, zero=False):
    """(re, im f32 [B,T,F], float64 outputs and states, torch-f32 outputs) -- computed once, shared, read-only"""
    F, nb_erb, _, nb_df = cfg
    re, im = R.spectrum(B, T, F, seed=1000 * B + T)
    if zero:
        re, im = np.zeros_like(re), np.zeros_like(im)
    re, im = re * np.float32(scale), im * np.float32(scale)
    starts = R.starts_of(widths_of(cfg))
    ref = R.df_feat(re, im, starts, nb_df, alpha)
    t32 = R.df_feat_torch32(re, im, starts, nb_df, alpha)
    for a in (re, im) + ref + t32:
        a.setflags(write=False)
    return re, im, ref, t32


def dev(a, interleaved=False):
    """numpy planes -> device tensors placed at the END of their allocation (a read past the last element leaves the block)"""
    if interleaved:
        x = np.stack(a, axis=-1)
        buf = torch.empty(x.size + 64, device="cuda")
        t = buf[64:].view(x.shape)
        t.copy_(torch.from_numpy(np.array(x)))
        return t[..., 0], t[..., 1]
    out = []
    for p in a:
        buf = torch.empty(p.size + 64, device="cuda")
        t = buf[64:].view(p.shape)
        t.copy_(torch.from_numpy(np.array(p)))
        out.append(t)
    return out


def table(cfg):
    from cruse_amd.model.based_model.cust_conv import _band_table
    return _band_table(list(widths_of(cfg)), torch.device("cuda", 0))[0]


def check_bar(tag, got_erb, got_spec, ref, t32, states=None):
    """-> the figures; asserts the bar.  states = (erb_state, unit_state) after the call: the same rule against the restatement's last m
    (absolute) and s (relative to its maximum), ref and t32 then carry theirs as items 2 and 3"""
    figs = {}
    if states is not None:
        ek, et = np.abs(states[0] - ref[2]).max(), np.abs(t32[2] - ref[2]).max()
        figs["erb_state"] = (ek, et, max(4 * et, float(np.spacing(np.float32(np.abs(ref[2]).max())))))
        mx = np.abs(ref[3]).max()
        ek, et = np.abs(states[1] - ref[3]).max() / mx, np.abs(t32[3] - ref[3]).max() / mx
        figs["unit_state"] = (ek, et, max(4 * et, float(np.spacing(np.float32(mx))) / mx))
    if ref[0] is not None and ref[0].size:
        ek, et = np.abs(got_erb - ref[0]).max(), np.abs(t32[0] - ref[0]).max()
        bar = max(4 * et, float(np.spacing(np.float32(np.abs(ref[0]).max()))))
        figs["erb"] = (ek, et, bar)
    if ref[1] is not None and ref[1].size:
        mx = np.abs(ref[1]).max()
        if mx > 0:
            ek, et = np.abs(got_spec - ref[1]).max() / mx, np.abs(t32[1] - ref[1]).max() / mx
            bar = max(4 * et, float(np.spacing(np.float32(mx))) / mx)
            figs["spec"] = (ek, et, bar)
    print(tag, {k: tuple(f"{x:.3e}" for x in v) for k, v in figs.items()}, "(kernel, torch f32, bar)")
    for k, (ek, et, bar) in figs.items():
        assert np.isfinite(ek) and ek <= bar, (tag, k, ek, et, bar)
    return figs


@pytest.mark.parametrize("interleaved", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("alpha", [0.8, 0.99])
@pytest.mark.parametrize("cfg", list(CONFIGS), ids=lambda c: "F%d_e%d_m%d_d%d" % c)
@pytest.mark.parametrize("T", T_EDGES)
@pytest.mark.parametrize("B", [1, 3])
def test_accuracy_against_float64(B, T, cfg, alpha, interleaved):
    from cruse_amd import ops
    re, im, ref, t32 = case(B, T, cfg, alpha)
    dre, dim = dev((re, im), interleaved)
    es, us = ops.df_feat_states(B, cfg[1], cfg[3], "cuda")
    fe, fs = ops.df_feat(dre, dim, table(cfg), cfg[3], alpha, erb_state=es, unit_state=us)
    assert fe.shape == (B, T, cfg[1]) and fs.shape == (B, T, cfg[3], 2)
    # (the returned states are the restatement's last m and s, on the same rule)
    check_bar(f"B{B} T{T} {cfg} a{alpha}", fe.cpu().numpy(), fs.cpu().numpy(), ref, t32, states=(es.cpu().numpy(), us.cpu().numpy()))


@pytest.mark.parametrize("F", [1, 96])
@pytest.mark.parametrize("alpha", [0.8, 0.99])
def test_unit_norm_module_against_the_reference_fixture(golden, F, alpha):
    from cruse_amd.acoustics import ExponentialUnitNorm
    g = golden("dfeat.npz")
    x, y = g[f"x/{F}"], g[f"y/{F}/{alpha}"]
    m = ExponentialUnitNorm(alpha, F).cuda()
    got = m(torch.from_numpy(x).cuda())
    assert got.shape == x.shape
    _, ref, _, _ = R.df_feat(x[:, 0, ..., 0], x[:, 0, ..., 1], None, F, alpha)
    check_bar(f"fixture F{F} a{alpha}", None, got.cpu().numpy()[:, 0], (None, ref), (None, y[:, 0]))
    # a second call starts from init_state again, as the reference does; with state= the module carries it
    assert torch.equal(m(torch.from_numpy(x).cuda()), got)
    st = m.init_state.view(1, 1, F).repeat(2, 1, 1).contiguous()
    parts = [m(torch.from_numpy(x[:, :, a:b]).cuda(), state=st) for a, b in ((0, 1), (1, 20), (20, 37))]
    assert torch.equal(torch.cat(parts, 2).view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("interleaved", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("cfg", [(161, 32, 2, 96), (161, 24, 1, 161)], ids=lambda c: "F%d_e%d_m%d_d%d" % c)
def test_split_invariance_to_the_bit(cfg, interleaved):
    from cruse_amd import ops
    B, T, alpha = 3, 2 * TC + 3, 0.99
    re, im, _, _ = case(B, T, cfg, alpha)
    starts = table(cfg)

    def run(splits):
        es, us = ops.df_feat_states(B, cfg[1], cfg[3], "cuda")
        fe, fs, t0 = [], [], 0
        for n in splits:
            dre, dim = dev((re[:, t0:t0 + n], im[:, t0:t0 + n]), interleaved)
            a, b = ops.df_feat(dre, dim, starts, cfg[3], alpha, erb_state=es, unit_state=us)
            fe.append(a); fs.append(b); t0 += n
        assert t0 == T
        return [t.view(torch.int32) for t in (torch.cat(fe, 1), torch.cat(fs, 1), es, us)]

    one = run([T])
    for splits in ([1, TC, TC + 2], [1] * T):
        for name, a, b in zip(("feat_erb", "feat_spec", "erb_state", "unit_state"), one, run(splits)):
            assert int((a != b).sum()) == 0, (name, splits[:3], int((a != b).sum()))


def test_states_are_honoured_and_defaults_apply():
    from cruse_amd import ops
    cfg, B, T, alpha = (161, 32, 2, 96), 3, TC + 1, 0.8
    re, im, ref, t32 = case(B, T, cfg, alpha)
    dre, dim = dev((re, im))
    # no states: the defaults, and the caller sees no state
    fe, fs = ops.df_feat(dre, dim, table(cfg), cfg[3], alpha)
    check_bar("default states", fe.cpu().numpy(), fs.cpu().numpy(), ref, t32)
    # a non-default incoming state
    rng = np.random.default_rng(3)
    e0, u0 = rng.uniform(-80, -20, (B, 32)), rng.uniform(1e-3, 2.0, (B, 96))
    starts = R.starts_of(widths_of(cfg))
    es, us = torch.from_numpy(e0).float().cuda(), torch.from_numpy(u0).float().cuda()
    e0f, u0f = es.cpu().numpy().astype(np.float64), us.cpu().numpy().astype(np.float64)
    ref2 = R.df_feat(re, im, starts, 96, alpha, erb_state=e0f, unit_state=u0f)
    t32b = R.df_feat_torch32(re, im, starts, 96, alpha, erb_state=e0f, unit_state=u0f)
    fe2, fs2 = ops.df_feat(dre, dim, table(cfg), 96, alpha, erb_state=es, unit_state=us)
    check_bar("given states", fe2.cpu().numpy(), fs2.cpu().numpy(), ref2, t32b, states=(es.cpu().numpy(), us.cpu().numpy()))
    assert not torch.equal(fe2, fe) and not torch.equal(fs2, fs)


def guarded(shape, pad=64):
    """a contiguous view of `shape` inside a NaN-poisoned buffer with `pad` sentinels on both sides -> (view, whole buffer)"""
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), float("nan"), device="cuda")
    return buf[pad:pad + n].view(shape), buf


def sentinels_intact(buf, n, pad=64):
    return bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all())


@pytest.mark.parametrize("interleaved", [False, True], ids=["planar", "interleaved"])
@pytest.mark.parametrize("T", [1, TC - 1, 2 * TC + 3])
@pytest.mark.parametrize("cfg", list(CONFIGS), ids=lambda c: "F%d_e%d_m%d_d%d" % c)
def test_guard_bands_stay_intact(cfg, T, interleaved):
    from cruse_amd import ops
    B, alpha = 3, 0.99
    F, nb_erb, _, nb_df = cfg
    re, im, ref, t32 = case(B, T, cfg, alpha)
    dre, dim = dev((re, im), interleaved)
    d_erb, d_unit = ops.df_feat_states(B, nb_erb, nb_df, "cuda")
    (es, bes), (us, bus) = guarded((B, nb_erb)), guarded((B, nb_df))
    es.copy_(d_erb); us.copy_(d_unit)
    (fe, bfe), (fs, bfs) = guarded((B, T, nb_erb)), guarded((B, T, nb_df, 2))
    ws, bws = guarded((256,))                                            # the op takes a workspace and must not touch it
    ops.df_feat(dre, dim, table(cfg), nb_df, alpha, erb_state=es, unit_state=us, out=(fe, fs), ws=ws)
    torch.cuda.synchronize()
    for name, buf, n in (("erb_state", bes, B * nb_erb), ("unit_state", bus, B * nb_df), ("feat_erb", bfe, B * T * nb_erb),
                         ("feat_spec", bfs, B * T * nb_df * 2), ("ws", bws, 0)):
        assert sentinels_intact(buf, n), name
    assert bool(torch.isnan(ws).all())
    assert not torch.isnan(fe).any() and not torch.isnan(fs).any() and not torch.isnan(es).any() and not torch.isnan(us).any()
    check_bar(f"guard {cfg} T{T}", fe.cpu().numpy(), fs.cpu().numpy(), ref, t32)


def test_skipped_outputs_and_empty_calls_write_nothing():
    from cruse_amd import ops
    cfg, B, T, alpha = (161, 32, 2, 96), 3, TC + 1, 0.99
    re, im, ref, t32 = case(B, T, cfg, alpha)
    dre, dim = dev((re, im))
    nan = float("nan")
    fe, fs = torch.full((B, T, 32), nan, device="cuda"), torch.full((B, T, 96, 2), nan, device="cuda")
    es, us = torch.full((B, 32), nan, device="cuda"), torch.full((B, 96), nan, device="cuda")
    d_erb, d_unit = ops.df_feat_states(B, 32, 96, "cuda")
    # nb_erb = 0 (no table): the ERB side stays poisoned, the other is complete
    us.copy_(d_unit)
    a, b = ops.df_feat(dre, dim, None, 96, alpha, erb_state=es, unit_state=us, out=(fe, fs))
    assert a is None and b is fs and bool(torch.isnan(fe).all()) and bool(torch.isnan(es).all()) and not torch.isnan(fs).any()
    check_bar("spec only", None, fs.cpu().numpy(), (None, ref[1]), (None, t32[1]))
    # nb_df = 0: the complex side stays poisoned
    fs.fill_(nan); us.fill_(nan); es.copy_(d_erb)
    a, b = ops.df_feat(dre, dim, table(cfg), 0, alpha, erb_state=es, unit_state=us, out=(fe, fs))
    assert a is fe and b is None and bool(torch.isnan(fs).all()) and bool(torch.isnan(us).all()) and not torch.isnan(fe).any()
    check_bar("erb only", fe.cpu().numpy(), None, (ref[0], None), (t32[0], None))
    # T = 0: nothing is written, the states stay
    es.copy_(d_erb); us.copy_(d_unit)
    a, b = ops.df_feat(dre[:, :0], dim[:, :0], table(cfg), 96, alpha, erb_state=es, unit_state=us)
    assert a.shape == (B, 0, 32) and b.shape == (B, 0, 96, 2) and torch.equal(es, d_erb) and torch.equal(us, d_unit)


def test_silence_is_finite_and_exact():
    from cruse_amd import ops
    cfg, B, T, alpha = (161, 32, 2, 96), 1, TC + 1, 0.99
    re, im, ref, t32 = case(B, T, cfg, alpha, zero=True)
    for state0 in (None, 0.0):                                           # the defaults, and the all-zero state (s > 0 by unit_eps alone)
        es, us = ops.df_feat_states(B, 32, 96, "cuda")
        want, t32s = ref, t32
        if state0 is not None:
            es.zero_(); us.zero_()
            z = (np.zeros((B, 32)), np.zeros((B, 96)))
            starts = R.starts_of(widths_of(cfg))
            want = R.df_feat(re, im, starts, 96, alpha, erb_state=z[0], unit_state=z[1])
            t32s = R.df_feat_torch32(re, im, starts, 96, alpha, erb_state=z[0], unit_state=z[1])
        fe, fs = ops.df_feat(*dev((re, im)), table(cfg), 96, alpha, erb_state=es, unit_state=us)
        assert bool(torch.isfinite(fe).all()) and bool(torch.isfinite(fs).all()) and bool((fs == 0).all())
        assert bool(torch.isfinite(es).all()) and bool((us > 0).all())
        check_bar(f"silence state0={state0}", fe.cpu().numpy(), None, (want[0], None), (t32s[0], None))


@pytest.mark.parametrize("scale", [2.0 ** 20, 2.0 ** -20])
def test_loud_and_quiet_spectra_stay_inside_the_bar(scale):
    from cruse_amd import ops
    cfg, B, T, alpha = (161, 32, 2, 96), 3, TC + 1, 0.99
    re, im, ref, t32 = case(B, T, cfg, alpha, scale=scale)
    fe, fs = ops.df_feat(*dev((re, im)), table(cfg), 96, alpha)
    assert bool(torch.isfinite(fe).all()) and bool(torch.isfinite(fs).all())
    check_bar(f"scale {scale}", fe.cpu().numpy(), fs.cpu().numpy(), ref, t32)


def test_graph_replays_give_the_bits_of_eager_calls():
    from cruse_amd.acoustics import DfFeatures
    m = DfFeatures()
    B, T = 3, TC + 1
    chunks = [dev(R.spectrum(B, T, 161, seed=70 + i)) for i in range(3)]
    state = m.init_state(B, "cuda")
    eager = []
    for re, im in chunks:
        fe, fs = m(re, im, state)
        eager.append((fe.clone(), fs.clone()))
    eager_state = [s.clone() for s in state]

    sre, sim = torch.empty(B, T, 161, device="cuda"), torch.empty(B, T, 161, device="cuda")
    gstate = m.init_state(B, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sre.copy_(chunks[0][0]); sim.copy_(chunks[0][1])
        m(sre, sim, [s.clone() for s in gstate])                         # warm-up outside the capture, on a throw-away state
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gfe, gfs = m(sre, sim, gstate)
    for (re, im), (fe, fs) in zip(chunks, eager):
        sre.copy_(re); sim.copy_(im)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gfe.view(torch.int32), fe.view(torch.int32)) and torch.equal(gfs.view(torch.int32), fs.view(torch.int32))
    for a, b in zip(gstate, eager_state):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_from_wave_is_forward_of_the_stft():
    from cruse_amd import ops
    from cruse_amd.acoustics import DfFeatures
    m = DfFeatures()
    g = torch.Generator().manual_seed(9)
    wave = (0.05 * torch.randn(2, 4000, generator=g)).cuda()
    s1, s2 = m.init_state(2, "cuda"), m.init_state(2, "cuda")
    fe, fs = m.from_wave(wave, s1)
    want = m(*ops.stft(wave, m.fft_size, m.hop_size)[:2], s2)
    assert fe.shape == (2, 1, 26, 32) and fs.shape == (2, 1, 26, 96, 2)
    assert torch.equal(fe.view(torch.int32), want[0].view(torch.int32)) and torch.equal(fs.view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1]) and not torch.equal(s1[0], m.init_state(2, "cuda")[0])
