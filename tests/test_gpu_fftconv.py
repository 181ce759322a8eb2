"""GPU: cruse_fftconv_prepare / cruse_fftconv_apply and add_reverb on them against float64 (tests/fftconv_ref.py).

The bar is measured per case, not fixed: 4 x the error of scipy's own f32 fftconvolve against float64 (the reference's arithmetic), per
clip in rel-L2 and in max |d| / peak, floor 4 * 2^-23, rel-L2 cap 5e-6; every test prints its worst error / bar.  Measured on an MI355X over
every case of this file: worst error / bar = 0.524 (L = 2047), 0.257 at B = 4, L = 64 000, R = 8 000."""
import numpy as np
import pytest
import torch

import fftconv_ref as F
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
P = F.P


def dv(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def conv(x, h, idx=None, early_len=None):
    """through prepare + apply; -> numpy y, or (y, y_early)"""
    from cruse_amd import ops
    bank = ops.fft_conv_prepare(dv(h), None if early_len is None else dv(np.asarray(early_len, dtype=np.int32)))
    out = ops.fft_conv_apply(dv(x), bank, h_index=None if idx is None else dv(idx), want_early=early_len is not None)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out) if early_len is not None else out.cpu().numpy()


def test_constant():
    from cruse_amd import ops
    assert ops.FFTCONV_PART == P


@pytest.mark.parametrize("L", F.gpu_lengths())
def test_shapes_against_float64(L):
    worst = 0.0
    for R in F.gpu_taps():
        for B, bank in F.BANKS:
            x, h, idx, hb = F.case(B, L, R, bank)
            r = F.ratio(conv(x, h, idx), x, hb)
            worst = max(worst, r)
            print(f"L={L} R={R} B={B} {bank}: error / bar = {r:.3f}")
            assert r <= 1.0, (L, R, B, bank, r)
    print(f"L = {L}: worst error / bar {worst:.3f}")


def test_training_shape():
    x, h = F.signal_like(4, 64000, 3), F.synth_rir(4, 8000, 5)
    r = F.ratio(conv(x, h), x, h)
    print(f"B=4 L=64000 R=8000: error / bar = {r:.3f}")
    assert r <= 1.0


def test_delayed_copies_and_shifted_filters():
    L, R = 2 * P + 1, 2 * P + 1
    x = F.signal_like(1, L, 11)
    for k in (0, 1, P - 1, P, R - 1):
        h = np.zeros((1, R), dtype=np.float32)
        h[0, k] = 1.0
        got = conv(x, h)
        want = np.zeros((1, L))
        want[0, k:] = x[0, :L - k]
        r = F.ratio(got, x, h, want)
        print(f"h = delta_{k}: error / bar = {r:.3f}")
        assert r <= 1.0, (k, r)
    h = F.synth_rir(1, R, 12, max_delay_ms=0)                # the direct path at tap 0: x = delta_{L-1} leaves the one sample h[0], not silence
    for m in (0, P - 1, P, L - 1):
        d = np.zeros((1, L), dtype=np.float32)
        d[0, m] = 1.0
        got = conv(d, h)
        want = np.zeros((1, L))
        want[0, m:] = h[0, :L - m]
        r = F.ratio(got, d, h, want)
        print(f"x = delta_{m}: error / bar = {r:.3f}")
        assert r <= 1.0, (m, r)


def test_early_output():
    L, R = 4099, 1200
    x, h = F.signal_like(3, L, 21), F.synth_rir(3, R, 22)
    plain = conv(x, h)
    for el in (0, 1, 7 + 800, R, R + 5, -3):
        full, early = conv(x, h, early_len=[el] * 3)
        c = min(max(el, 0), R)
        cut = h.copy()
        cut[:, c:] = 0.0
        assert np.array_equal(early.view(np.uint32), conv(x, cut).view(np.uint32)), el       # the same bits as the zeroed filter
        assert np.array_equal(full.view(np.uint32), plain.view(np.uint32)), el               # y does not depend on the request
        if c == 0:
            assert not early.any()
        else:
            assert F.ratio(early, x, cut) <= 1.0
        if c == R:
            assert np.array_equal(early.view(np.uint32), full.view(np.uint32))
    full, early = conv(x, h, early_len=[0, 807, R + 5])                                       # one length per filter
    assert not early[0].any() and np.array_equal(early[2], full[2]) and not np.array_equal(early[1], full[1])


def test_pass_through_and_an_index_beyond_the_bank():
    L, R = 4099, 600
    x, h = F.signal_like(3, L, 31), F.synth_rir(2, R, 32)
    for idx in ([-1, 0, -1], [2, 0, 1 << 20]):                                                # 2 >= NR: clamped to pass-through
        full, early = conv(x, h, idx=np.array(idx, dtype=np.int32), early_len=[100, 100])
        for b in (0, 2):
            assert np.array_equal(full[b].view(np.uint32), x[b].view(np.uint32)) and np.array_equal(early[b].view(np.uint32), x[b].view(np.uint32))
        assert F.ratio(full[1:2], x[1:2], h[0:1]) <= 1.0 and not np.array_equal(full[1], x[1])
    y = conv(x, h, idx=np.array([-5, -1, -1], dtype=np.int32))
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))


def test_against_the_direct_kernel_and_fixture_g20(golden):
    from cruse_amd import ops
    from cruse_amd.data import fir_causal
    g = golden("g20_snr_mix_rir.npz")
    outs = {}
    for name, xs, hs in (("clean", g["clean"], g["rir"]), ("noise", g["noise"], g["rir_noise"])):
        x, h = dv(xs), dv(hs)
        y = ops.fft_conv_causal(x, h)
        e = rel_l2(y, fir_causal(x, h))
        print(f"{name}: fft_conv_causal vs fir_causal rel-L2 {e:.2e}")
        assert e < 5e-6
        outs[name] = y.cpu().numpy().astype(np.float64)
    # snr_mix's normalisation in numpy on the kernel's convolutions, against the reference's own outputs
    c = outs["clean"] / (np.abs(outs["clean"]).max(axis=1, keepdims=True) + 1e-7)
    n = outs["noise"] / (np.abs(outs["noise"]).max(axis=1, keepdims=True) + 1e-7)
    scalar = np.sqrt((c ** 2).mean(axis=1)) / 10 ** (g["snr"].astype(np.float64) / 20) / (np.sqrt((n ** 2).mean(axis=1)) + 1e-7)
    n = n * scalar[:, None]
    for got, key in ((c, "clean_n"), (n, "noise_s"), (c + n, "noisy")):
        e = rel_l2(torch.from_numpy(got), torch.from_numpy(g[key]))
        print(f"{key}: rel-L2 {e:.2e}")
        assert e < 5e-6


def test_two_runs_are_bit_identical_and_a_clip_convolves_the_same_alone():
    L, R = 2 * P + 1, P + 1
    x, h = F.signal_like(3, L, 41), F.synth_rir(3, R, 42)
    a, b = conv(x, h, early_len=[900] * 3), conv(x, h, early_len=[900] * 3)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    alone = conv(x[2:3], h[2:3], early_len=[900])
    assert np.array_equal(alone[0].view(np.uint32), a[0][2:3].view(np.uint32)) and np.array_equal(alone[1].view(np.uint32), a[1][2:3].view(np.uint32))


def test_sentinels_beside_outputs_workspace_and_spectra_survive():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    pad, sent = 64, 12345.678
    for B, L, NR, R in ((3, 2 * P + 1, 2, P + 1), (1, 1, 1, 1), (2, P - 1, 2, 600)):
        sb, wb = lib.cruse_fftconv_spec_bytes(NR, R, 1), lib.cruse_fftconv_ws_bytes(B, L)
        bufs = {k: torch.full((n + 2 * pad,), sent, device="cuda", dtype=torch.float32) for k, n in (("y", B * L), ("ye", B * L), ("ws", wb // 4), ("spec", sb // 4))}
        inner = {k: v[pad:v.numel() - pad] for k, v in bufs.items()}
        x, h = F.signal_like(B, L, 51), F.synth_rir(NR, R, 52, max_delay_ms=0)
        idx = np.arange(B, dtype=np.int32) % NR
        bank = ops.fft_conv_prepare(dv(h), dv(np.full(NR, 300, dtype=np.int32)), spec=inner["spec"].view(torch.uint8))
        y, ye = ops.fft_conv_apply(dv(x), bank, h_index=dv(idx), want_early=True, out=inner["y"].view(B, L), out_early=inner["ye"].view(B, L),
                                   ws=inner["ws"].view(torch.uint8))
        torch.cuda.synchronize()
        assert y.data_ptr() == inner["y"].data_ptr()
        for k, v in bufs.items():
            assert bool((v[:pad] == sent).all()) and bool((v[-pad:] == sent).all()), f"a sentinel beside {k} was overwritten"
        assert F.ratio(y.cpu().numpy(), x, h[idx]) <= 1.0


def test_replays_from_a_captured_graph_with_new_input_and_index():
    from cruse_amd import ops
    B, L, R = 3, 2 * P + 1, 600
    h = F.synth_rir(2, R, 61)
    bank = ops.fft_conv_prepare(dv(h))                                                        # outside the capture
    xs = [F.signal_like(B, L, 62 + i) for i in range(3)]
    idxs = [np.array(v, dtype=np.int32) for v in ([0, 1, 0], [1, -1, 0], [-1, 1, 1])]
    x, idx, y = dv(xs[0]), dv(idxs[0]), torch.empty(B, L, device="cuda")
    ops.fft_conv_apply(x, bank, h_index=idx, out=y)                                           # (the workspace is taken outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.fft_conv_apply(x, bank, h_index=idx, out=y)
    for xi, ii in zip(xs[1:], idxs[1:]):
        x.copy_(torch.from_numpy(xi))
        idx.copy_(torch.from_numpy(ii))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        for b in range(B):
            if ii[b] < 0:
                assert np.array_equal(got[b].view(np.uint32), xi[b].view(np.uint32))
            else:
                assert F.ratio(got[b:b + 1], xi[b:b + 1], h[ii[b]:ii[b] + 1]) <= 1.0


def test_add_reverb_matches_fixture_g23(golden):
    from cruse_amd.data import add_reverb
    from dataset.dataset import SynDataset
    g = golden("g23_add_reverb.npz")
    names = ("peak7", "late", "negative")
    for b, name in enumerate(names):
        x, rir = g["clean"][b], g[f"{name}/rir"]
        want = (g[f"{name}/wav_tgt"], g[f"{name}/wav_early_tgt"])
        et = min(int(F.early_len(rir[:, 0])[0]), len(rir))
        cut = np.where(np.arange(len(rir)) < et, rir[:, 0], 0).astype(np.float32)
        for form in (rir, rir[:, 0]):                                                         # the reference's [R, 1] and a plain [R]
            got = SynDataset.add_reverb(dv(x), dv(form))
            torch.cuda.synchronize()
            assert all(o.shape == (4000, 1) and o.dtype == torch.float32 and o.is_cuda for o in got)
            for o, w, hh in zip(got, want, (rir[:, 0], cut)):
                r = F.ratio(o[:, 0].cpu().numpy()[None], x, hh, w[:, 0][None])
                print(f"{name}: error / bar = {r:.3f}")
                assert r <= 1.0, (name, r)
    # the batch form: three clips, each with its own response (the two 1200-tap ones; `late` has 600 taps and goes alone above)
    xb, hb = g["clean"][[0, 2]], np.stack([g["peak7/rir"][:, 0], g["negative/rir"][:, 0]])
    full, early = add_reverb(dv(xb), dv(hb))
    torch.cuda.synchronize()
    assert full.shape == early.shape == (2, 4000)
    for i, name in enumerate(("peak7", "negative")):
        cut = np.where(np.arange(1200) < 807, hb[i], 0).astype(np.float32)
        assert F.ratio(full[i:i + 1].cpu().numpy(), xb[i], hb[i], g[f"{name}/wav_tgt"][:, 0][None]) <= 1.0
        assert F.ratio(early[i:i + 1].cpu().numpy(), xb[i], cut, g[f"{name}/wav_early_tgt"][:, 0][None]) <= 1.0
    one = add_reverb(dv(xb[0]), dv(hb[0]))
    assert one[0].shape == (4000,) and torch.equal(one[0], full[0]) and torch.equal(one[1], early[0])


def test_wrappers_refuse_what_the_kernel_cannot_take():
    from cruse_amd import ops
    x, h = torch.zeros(2, 100, device="cuda"), torch.ones(3, 10, device="cuda")
    bank = ops.fft_conv_prepare(h)
    with pytest.raises(RuntimeError):
        ops.fft_conv_apply(x, bank)                                                           # 3 filters, 2 clips, no index
    with pytest.raises(RuntimeError):
        ops.fft_conv_apply(x, bank, want_early=True)                                          # prepared without early_len
    with pytest.raises(RuntimeError):
        ops.fft_conv_apply(x, bank, h_index=torch.zeros(2, device="cuda", dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ops.fft_conv_causal(x, h)
    with pytest.raises(RuntimeError):
        ops.fft_conv_prepare(h.cpu())
    y = ops.fft_conv_apply(x, bank, h_index=torch.tensor([2, 0], device="cuda", dtype=torch.int32))
    assert torch.equal(y, x)
