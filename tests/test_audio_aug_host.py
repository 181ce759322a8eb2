"""Host side of the EQ augmentation: the RBJ designers against an independent restatement and their magnitude
responses, the draws, the C interface of cruse_biquad_cascade without a device, the recorded f32 condition, configs and defaults."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import biquad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def A():
    from cruse_amd.acoustics import audio_aug
    return audio_aug


def grid(kind):
    lo, hi = R.FREQ_RANGE[kind]
    fs = list(np.geomspace(lo, min(hi, 7999.0), 5))
    pts = [(f, g, q) for f in fs for g in (-15.0, -3.0, 0.0, 7.5, 15.0) for q in (0.5, 1.0, 1.5)]
    return pts + [c[1:] for c in R.CORNERS.values() if c[0] == kind]


@pytest.mark.parametrize("kind", R.KINDS)
def test_designer_equals_restatement(kind):
    import torch
    for f, g, q in grid(kind):
        got = A().REGISTERED_SecFilter[kind](f, g, q, 16000)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and tuple(got.shape) == (2, 3), (kind, got)
        want = R.design(kind, f, g, q)
        np.testing.assert_allclose(got.numpy().reshape(6), want, rtol=1e-12, atol=1e-15, err_msg=f"{kind} {f} {g} {q}")


def test_designers_take_the_reference_argument_forms():
    import torch
    a = A()
    want = R.design("peaking_eq", 300.0, 6.0, 0.8)
    for f, g, q in ((300.0, 6.0, 0.8), (np.array([300.0]), np.array([6.0]), np.array([0.8])), (torch.tensor(300.0), torch.tensor([6.0]), 0.8)):
        np.testing.assert_allclose(a.peaking_eq(f, g, q, 16000).numpy().reshape(6), want, rtol=1e-6)    # (a tensor input is f32)
    assert a.high_pass(150.0, 0, 1.0, 16000.0).shape == (2, 3)       # sr is a float for high_pass too
    assert set(a.REGISTERED_SecFilter) == set(R.KINDS)
    assert {k: tuple(v) for k, v in a.REGISTERED_SecFilter_freq.items()} == R.FREQ_RANGE
    import train_base.acoustics.audioAug as shim
    assert shim.compositeSecFilt is a.compositeSecFilt and shim.hp_filter is a.hp_filter and shim.notch is a.notch
    assert shim.REGISTERED_SecFilter is a.REGISTERED_SecFilter and shim.draw_sec_filters is a.draw_sec_filters


@pytest.mark.parametrize("g", [-15.0, -6.0, 6.0, 15.0])
@pytest.mark.parametrize("q", [0.5, 1.0, 1.5])
def test_magnitude_responses(g, q):
    a = A()
    c = lambda kind, f: a.REGISTERED_SecFilter[kind](f, g, q, 16000).numpy().reshape(6)
    ls, hs = c("low_shelf", 300.0), c("high_shelf", 2000.0)
    assert abs(R.response_db(ls, 1e-3) - g) < 0.1 and abs(R.response_db(ls, 7999.9)) < 0.1
    assert abs(R.response_db(hs, 7999.9) - g) < 0.1 and abs(R.response_db(hs, 1e-3)) < 0.1
    assert abs(R.response_db(c("peaking_eq", 1000.0), 1000.0) - g) < 1e-6
    assert R.response_db(c("notch", 1000.0), 1000.0) < -60.0
    for kind, far, stop in (("high_pass", 7999.9, 1e-3), ("low_pass", 1e-3, 7999.9)):
        k = c(kind, 1000.0)
        assert abs(R.response_db(k, 1000.0) - 20.0 * np.log10(q)) < 1e-9           # |H(w0)| = Q exactly (-3 dB at Q = 1 / sqrt 2)
        assert abs(R.response_db(k, far)) < 1e-3 and R.response_db(k, stop) < -100.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_designer_refuses_nyquist_and_beyond(kind):
    for f in (8000.0, 8000.1, 12000.0, 0.0, -5.0):
        with pytest.raises(ValueError):
            A().REGISTERED_SecFilter[kind](f, 3.0, 1.0, 16000)
    A().REGISTERED_SecFilter[kind](np.nextafter(8000.0, 0.0), 3.0, 1.0, 16000)


def test_every_drawn_filter_is_stable():
    a, rng = A(), np.random.default_rng(11)
    sec = np.concatenate([a.draw_sec_filters(2000, 5, rng=rng).reshape(-1, 6), a.draw_hp_filters(100, 1, rng=rng).reshape(-1, 6)])
    assert len(sec) >= 10000
    a0, a1, a2 = sec[:, 3], sec[:, 4] / sec[:, 3], sec[:, 5] / sec[:, 3]
    assert np.all(a0 > 0)
    disc = a1 * a1 - 4 * a2
    radius = np.where(disc < 0, np.sqrt(np.abs(a2)), (np.abs(a1) + np.sqrt(np.abs(disc))) / 2)
    assert radius.max() < 1.0, radius.max()
    worst = int(radius.argmax())
    assert abs(R.pole_radius(sec[worst]) - radius[worst]) < 1e-9     # (the closed form above is the root finder's radius)


def test_draws():
    a = A()
    types, freq, gain, q = a.draw_sec_filter_params(500, 3, rng=np.random.default_rng(5))
    assert types.shape == freq.shape == gain.shape == q.shape == (500, 3)
    assert all(len(set(row)) == 3 for row in types.tolist()) and set(types.reshape(-1).tolist()) == set(range(6))
    for t, kind in enumerate(a.FILTER_LIST):
        lo, hi = a.REGISTERED_SecFilter_freq[kind]
        f = freq[types == t]
        assert f.min() >= lo and f.max() <= hi and f.max() < 8000.0
        assert np.median(f) < (lo + hi) / 2                          # log-uniform: the median is the geometric mean
    assert gain.min() >= -15 and gain.max() <= 15 and gain.std() > 5 and q.min() >= 0.5 and q.max() <= 1.5
    c = a.draw_sec_filters(500, 3, rng=np.random.default_rng(5))
    assert c.shape == (500, 3, 6) and c.dtype == np.float64
    for i in (0, 17, 499):                                           # the batch design is the scalar designers on the same draws
        for k in range(3):
            np.testing.assert_allclose(c[i, k], R.design(a.FILTER_LIST[types[i, k]], freq[i, k], gain[i, k], q[i, k]), rtol=1e-12, atol=1e-15)
    assert np.array_equal(c, a.draw_sec_filters(500, 3, rng=np.random.default_rng(5)))
    assert not np.array_equal(c, a.draw_sec_filters(500, 3, rng=np.random.default_rng(6)))
    h = a.draw_hp_filters(50, 2, rng=np.random.default_rng(5))
    assert h.shape == (50, 2, 6) and h.dtype == np.float64 and np.array_equal(h[:, 0], h[:, 1])
    qs = np.random.default_rng(5).uniform(0.5, 1.5, size=50)
    np.testing.assert_allclose(h[7, 0], R.design("high_pass", 150.0, 0.0, qs[7]), rtol=1e-12)
    assert len({tuple(r) for r in h[:, 0].tolist()}) == 50           # one Q per clip
    for bad in (0, 6):
        with pytest.raises(ValueError):
            a.draw_sec_filters(4, bad)
    assert "do NOT replay" in a.draw_sec_filters.__doc__


def test_interface_without_a_device():
    from cruse_amd import ops
    from cruse_amd._abi_check import parse_header
    from cruse_amd._lib import SIGNATURES, lib
    hdr_src = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    hdr = parse_header()
    for name in ("cruse_biquad_ws_bytes", "cruse_biquad_cascade"):
        assert name in hdr and SIGNATURES[name] == hdr[name], name
    assert re.search(r"^#define CRUSE_ABI_VERSION 15$", hdr_src, flags=re.M) and lib.cruse_abi_version() == 15
    defs = dict(re.findall(r"^#define (CRUSE_BIQUAD_\w+) (\d+)$", hdr_src, flags=re.M))
    assert int(defs["CRUSE_BIQUAD_CHUNK"]) == ops.BIQUAD_CHUNK and int(defs["CRUSE_BIQUAD_TILE"]) == ops.BIQUAD_TILE
    assert ops.BIQUAD_TILE % ops.BIQUAD_CHUNK == 0
    assert lib.cruse_biquad_ws_bytes(64, 64000, 4) == 0 and lib.cruse_biquad_ws_bytes(1, 1, 1) == 0
    # refusals come before any device call: host pointers (never dereferenced) on a machine that may have no device at all
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    E_SHAPE = -1
    call = lambda x, c, stride, B, L, S, y: lib.cruse_biquad_cascade(x, c, stride, B, L, S, 1, None, y, None)
    assert call(None, p, 0, 1, 8, 1, p) == E_SHAPE and call(p, None, 0, 1, 8, 1, p) == E_SHAPE and call(p, p, 0, 1, 8, 1, None) == E_SHAPE
    assert call(p, p, 0, 1, 8, 0, p) == E_SHAPE and call(p, p, 0, 1, 8, 9, p) == E_SHAPE
    assert call(p, p, 5, 1, 8, 1, p) == E_SHAPE and call(p, p, 6, 1, 8, 2, p) == E_SHAPE
    assert call(p, p, 0, 0, 8, 1, p) == E_SHAPE and call(p, p, 0, 1, 0, 1, p) == E_SHAPE
    assert b"coef_stride" in lib.cruse_last_error() or b"B = " in lib.cruse_last_error()


def test_f32_recurrence_misses_the_bar_by_two_orders():
    """The recorded condition behind 'coefficients and recurrence are float64': on the 40 Hz +15 dB Q 1.5 low shelf (pole radius
    0.9966) at L = 64 000, a sequential all-f32 recurrence is off by 1.4e-3 against float64 lfilter on this signal (3.2e-4 on the one
    the decision was first measured on), where the GPU test's bar -- one f32 ulp at the clip's peak -- is 3.4e-7 (1.4e-7); float64
    rounded once to f32 stays inside half the bar."""
    x = R.synth_like(1, 64000, seed=7)[0]
    coef = R.corner("ls40_+15_q1.5").reshape(1, 6)
    assert 0.996 < R.pole_radius(coef[0]) < 0.997
    ref = R.cascade_ref(x, coef, clamp=False)
    bar = float(R.bar(ref)[0])
    err = float(np.abs(R.seq_f32(x, coef).astype(np.float64) - ref).max())
    once = float(np.abs(ref.astype(np.float32).astype(np.float64) - ref).max())
    print(f"f32 recurrence max|d| {err:.3e}, bar {bar:.3e} (ratio {err / bar:.0f}), f64 rounded once {once:.3e}")
    assert err > 100 * bar, (err, bar)
    assert once <= 0.5 * bar


def test_configs_parse_and_defaults_are_unchanged():
    from tools.train_stand import load_toml as load_config
    from cruse_amd.data import DevicePairs
    aug = load_config(os.path.join(ROOT, "configs", "cruse_augment.toml"))
    base = load_config(os.path.join(ROOT, "configs", "cruse_device_dataset.toml"))
    args = dict(aug["train_dataset"]["args"])
    assert (args.pop("eq_prob"), args.pop("eq_filters"), args.pop("hp_prob")) == (0.5, 3, 0.5)
    assert args == base["train_dataset"]["args"] and aug["train_dataset"]["path"] == "cruse_amd.data.DevicePairs"
    assert {k: v for k, v in aug.items() if k != "train_dataset"} == {k: v for k, v in base.items() if k != "train_dataset"}
    sig = inspect.signature(DevicePairs.__init__).parameters
    assert [sig[k].default for k in ("num", "length", "seed", "pool", "snr_low", "snr_high")] == [2048, 64000, 0, 128, 0.0, 20.0]
    assert (sig["eq_prob"].default, sig["eq_filters"].default, sig["hp_prob"].default) == (0.0, 3, 0.0)
    d = DevicePairs(**aug["train_dataset"]["args"])
    assert d.augments and not DevicePairs().augments and DevicePairs().aug_coefs is None
    c = d.draw_aug_coefs(200)
    assert c.shape == (200, 4, 6) and c.dtype == np.float64
    ident = np.all(c == np.array(R.IDENTITY), axis=2)
    eq_off, hp_off = ident[:, :3].all(axis=1), ident[:, 3]
    assert np.array_equal(ident[:, :3].any(axis=1), eq_off)          # a clip's EQ cascade is drawn whole or not at all
    assert 60 < eq_off.sum() < 140 and 60 < hp_off.sum() < 140
    assert np.array_equal(DevicePairs(**aug["train_dataset"]["args"]).draw_aug_coefs(200), c)
    with pytest.raises(ValueError):
        DevicePairs(eq_prob=0.5, eq_filters=6)
