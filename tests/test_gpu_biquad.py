"""GPU: cruse_biquad_cascade and the augmentation module on top of it against float64 scipy.signal.lfilter (tests/biquad_ref.py).

The bar is derived, not tuned: per clip  max |y - cascade_ref| <= 2^-23 max(peak |cascade_ref|, 1e-3)  against the float64 oracle
BEFORE any rounding -- one f32 ulp at the clip's peak.  A float64 recurrence rounded once to f32 is within half of it; the chunked
regrouping of the kernel (f64) adds about 1e-13.  Measured on an MI355X over every case of this file: worst |d| / bar = 0.469 (0.452 on
the 40 Hz +15 dB Q 1.5 low shelf, pole radius 0.9966; 0.000 on the identity); every test prints its own figure."""
import numpy as np
import pytest
import torch

import biquad_ref as R

pytestmark = pytest.mark.gpu


def CT():
    from cruse_amd import ops
    return ops.BIQUAD_CHUNK, ops.BIQUAD_TILE


def run(x, coef, clamp, **kw):
    from cruse_amd import ops
    y = ops.biquad_cascade(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(coef)).cuda(), clamp=clamp, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def ratio(got, ref):
    """worst |got - ref| over the clip's bar, per batch"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
    return float((np.abs(got.astype(np.float64) - ref).max(axis=1) / R.bar(ref)).max())


def check(x, coef, clamp, tag):
    ref = R.cascade_ref(x, coef, clamp)
    r = ratio(run(x, coef, clamp), ref)
    print(f"{tag}: worst |d| / bar = {r:.3f}")
    assert r <= 1.0, (tag, r)
    return ref


def corner_mix(B, S, seed):
    """[B, S, 6]: sections out of the corner table, a different run of them per clip"""
    tab = R.corner_table()
    idx = np.random.default_rng(seed).permutation(len(tab) * 4) % len(tab)
    return np.stack([tab[idx[b * S:(b + 1) * S]] for b in range(B)])


def shapes():
    C, T = 32, 32768                                                    # asserted against ops in test_constants
    lengths = [1, 2, 3, C - 1, C, C + 1, 64 * C - 1, 64 * C + 1, T - 1, T, T + 1, 2 * T + C + 1, 4099]
    cases = [(3, L, 4, True) for L in lengths]
    cases += [(1, L, 1, False) for L in (1, 2, 3, C + 1, T + 1)]
    cases += [(3, 4099, 3, False), (1, 4099, 8, True), (3, 2 * T + C + 1, 8, True), (1, 64 * C + 1, 3, True), (2, 64000, 4, True)]
    return cases


def test_constants():
    assert CT() == (32, 32768)                                           # shapes() above is built from them


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("B,L,S,per_clip", shapes())
def test_shapes_against_float64(B, L, S, per_clip, clamp):
    x = R.synth_like(B, L, seed=L % 1000 + S)
    coef = corner_mix(B, S, seed=L + B)
    check(x, coef if per_clip else coef[0], clamp, f"B={B} L={L} S={S} {'per-clip' if per_clip else 'shared'} clamp={clamp}")


@pytest.mark.parametrize("clamp", [True, False])
def test_every_corner_and_the_identity(clamp):
    C, T = CT()
    tab = np.concatenate([R.corner_table(), np.array([R.IDENTITY])])[:, None, :]         # [17, 1, 6]: one section per clip
    x = R.synth_like(len(tab), T + C + 1, seed=21)
    ref = R.cascade_ref(x, tab, clamp)
    got = run(x, tab, clamp)
    for i, name in enumerate(list(R.CORNERS) + ["identity"]):
        r = ratio(got[i], ref[i])
        print(f"{name}: pole radius {R.pole_radius(tab[i, 0]):.4f}  peak {np.abs(ref[i]).max():.3f}  |d| / bar = {r:.3f}")
        assert r <= 1.0, (name, r)


def test_a_drawn_batch():
    from cruse_amd.acoustics import audio_aug as A
    C, T = CT()
    rng = np.random.default_rng(3)
    coef = np.concatenate([A.draw_sec_filters(8, 3, rng=rng), A.draw_hp_filters(8, 1, rng=rng)], axis=1)
    assert coef.shape == (8, 4, 6)
    x = R.synth_like(8, 64 * C + 1, seed=4)
    check(x, coef, True, "drawn, clamp")
    check(x, coef, False, "drawn, no clamp")


def test_loud_input_clips_only_when_asked():
    C, T = CT()
    x = 3.0 * R.synth_like(2, T + 1, seed=8)
    coef = np.stack([R.corner("pk40_+15_q1.5"), R.corner("hs4000_+15_q1.5"), R.corner("hp40_q0.5")])
    ref_c = check(x, coef, True, "loud, clamp")
    ref_n = check(x, coef, False, "loud, no clamp")
    got_c, got_n = run(x, coef, True), run(x, coef, False)
    assert np.abs(got_c).max() <= 1.0 and np.abs(got_n).max() > 1.5 and np.abs(ref_n).max() > 1.5
    first = np.clip(R.cascade_ref(x, coef[:1], False), -1, 1)
    assert (np.abs(first) == 1.0).sum() > 2000                            # the clip acts thousands of times between the sections
    assert np.abs(ref_c - ref_n).max() > 0.1


def test_impulse_responses_across_chunk_and_tile_handoffs():
    C, T = CT()
    L = T + 4 * C
    at = [0, C, T, C - 1, T - 1, 64 * C]
    x = np.zeros((len(at), L), dtype=np.float32)
    for i, t in enumerate(at):
        x[i, t] = 0.9
    for name in ("ls40_+15_q1.5", "pk40_+15_q1.5", "lp7900_q1.5", "notch40_q1.5"):
        coef = np.stack([R.corner(name), R.corner("hp40_q1.5")])
        ref = check(x, coef, False, f"impulse, {name}")
        for i, t in enumerate(at):
            assert np.all(ref[i, :t] == 0) and ref[i, t] != 0
    got = run(x, np.stack([R.corner("ls40_+15_q1.5")]), False)
    for i, t in enumerate(at):
        assert np.all(got[i, :t] == 0)                                    # nothing leaks backwards through the scan


@pytest.mark.parametrize("clamp", [True, False])
def test_identity_cascade_is_exact(clamp):
    C, T = CT()
    x = R.synth_like(3, T + C + 1, seed=12)
    ident = np.tile(np.array(R.IDENTITY), (4, 1))
    assert np.array_equal(run(x, ident, clamp).view(np.uint32), x.view(np.uint32))
    scaled = ident * np.array([[2.0], [0.5], [-3.0], [7.0]])             # a0 != 1: normalised away exactly
    assert np.array_equal(run(x, scaled, clamp).view(np.uint32), x.view(np.uint32))


def test_two_runs_are_bit_identical_and_a_clip_filters_the_same_alone():
    C, T = CT()
    x = R.synth_like(3, 2 * T + C + 1, seed=13)
    coef = corner_mix(3, 4, seed=13)
    a, b = run(x, coef, True), run(x, coef, True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    alone = run(x[1:2], coef[1:2], True)
    assert np.array_equal(alone.view(np.uint32), a[1:2].view(np.uint32))


def test_sentinels_beside_output_and_workspace_survive():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    C, T = CT()
    pad, sent = 64, 12345.678
    # cruse_biquad_ws_bytes is 0 for every shape today (a clip never leaves its workgroup), so `ws` is an EMPTY slice between its
    # sentinels: that half of the check only pins that the call touches nothing around a zero-sized workspace.  It starts to bite
    # the day a shape gets a workspace; the sentinels beside `y` are the live check.
    for B, L, S in ((3, T + C + 1, 4), (2, 3, 1), (1, 64 * C - 1, 8)):
        n, need = B * L, lib.cruse_biquad_ws_bytes(B, L, S)
        assert need % 4 == 0
        ybuf = torch.full((n + 2 * pad,), sent, device="cuda", dtype=torch.float32)
        wsbuf = torch.full((need // 4 + 2 * pad,), sent, device="cuda", dtype=torch.float32)
        y, ws = ybuf[pad:pad + n].view(B, L), wsbuf[pad:pad + need // 4]
        x = R.synth_like(B, L, seed=14)
        coef = corner_mix(B, S, seed=14)
        out = ops.biquad_cascade(torch.from_numpy(x).cuda(), torch.from_numpy(coef).cuda(), clamp=True, out=y, ws=ws)
        torch.cuda.synchronize()
        assert out.data_ptr() == y.data_ptr()
        for buf, m in ((ybuf, n), (wsbuf, need // 4)):
            assert bool((buf[:pad] == sent).all()) and bool((buf[pad + m:] == sent).all()), "a sentinel beside the buffer was overwritten"
        assert ratio(y.cpu().numpy(), R.cascade_ref(x, coef, True)) <= 1.0


def test_replays_from_a_captured_graph_with_new_input():
    from cruse_amd import ops
    C, T = CT()
    B, L, S = 2, T + C + 1, 4
    xs = [R.synth_like(B, L, seed=30 + i) for i in range(3)]
    coef = corner_mix(B, S, seed=30)
    x = torch.from_numpy(xs[0]).cuda()
    cd = torch.from_numpy(coef).cuda()
    y = torch.empty_like(x)
    ops.biquad_cascade(x, cd, clamp=True, out=y)                         # (first call: the kernel's LDS attribute is set outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.biquad_cascade(x, cd, clamp=True, out=y)
    for xi in xs[1:]:
        x.copy_(torch.from_numpy(xi))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert ratio(y.cpu().numpy(), R.cascade_ref(xi, coef, True)) <= 1.0


def test_module_functions_equal_the_oracle_on_the_same_draws():
    from cruse_amd.acoustics import audio_aug as A
    import train_base.acoustics.audioAug as shim
    C, T = CT()
    L = 64 * C + 1
    xb = R.synth_like(3, L, seed=40)
    for x in (xb, xb[0]):
        n = 1 if x.ndim == 1 else x.shape[0]
        xd = torch.from_numpy(x).cuda()
        got = shim.compositeSecFilt(xd, filter_num=3, sr=16000, rng=np.random.default_rng(77))
        torch.cuda.synchronize()
        assert got.shape == xd.shape and got.dtype == torch.float32 and got.is_cuda
        coef = A.draw_sec_filters(n, 3, rng=np.random.default_rng(77))
        ref = R.cascade_ref(x, coef if x.ndim == 2 else coef[0], True)
        assert ratio(got.cpu().numpy(), ref) <= 1.0
        got = shim.hp_filter(xd, filte_num=2, rng=np.random.default_rng(78))
        torch.cuda.synchronize()
        assert got.shape == xd.shape
        coef = A.draw_hp_filters(n, 2, rng=np.random.default_rng(78))
        assert ratio(got.cpu().numpy(), R.cascade_ref(x, coef if x.ndim == 2 else coef[0], True)) <= 1.0
    if xb.shape[0] > 1:                                                   # one independent draw per clip
        c = A.draw_sec_filters(3, 3, rng=np.random.default_rng(77))
        assert not np.array_equal(c[0], c[1])
    with pytest.raises(RuntimeError):
        A.compositeSecFilt(torch.from_numpy(xb), rng=np.random.default_rng(0))      # a host tensor: there is no CPU path


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from cruse_amd import ops
    x = torch.zeros(2, 100, device="cuda")
    c64 = torch.tensor([R.IDENTITY], dtype=torch.float64, device="cuda")
    for bad in (c64.float(), c64.reshape(6), c64.expand(3, 1, 6).contiguous(), torch.zeros(9, 6, dtype=torch.float64, device="cuda"), c64.cpu()):
        with pytest.raises(RuntimeError):
            ops.biquad_cascade(x, bad)
    with pytest.raises(RuntimeError):
        ops.biquad_cascade(x.double(), c64)
    with pytest.raises(RuntimeError):
        ops.biquad_cascade(x[0], c64)
    assert torch.equal(ops.biquad_cascade(x, c64), x)
