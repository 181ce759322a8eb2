"""Host side of the FFT convolution and the reverberation on it: the C interface of cruse_fftconv_* without a
device, the byte layout, the numpy restatement against the bar and against fixture G23, configs, defaults and draws."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import fftconv_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cruse_fftconv_spec_bytes", "cruse_fftconv_ws_bytes", "cruse_fftconv_prepare", "cruse_fftconv_apply", "cruse_peak_scale")
E_SHAPE = -1


def test_header_signatures_and_library_agree():
    from cruse_amd import ops
    from cruse_amd._abi_check import parse_header
    from cruse_amd._lib import SIGNATURES, lib
    hdr_src = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    hdr = parse_header()
    for name in NAMES:
        assert name in hdr and SIGNATURES[name] == hdr[name] and hasattr(lib, name), name
    assert re.search(r"^#define CRUSE_ABI_VERSION 15$", hdr_src, flags=re.M) and lib.cruse_abi_version() == 15
    part = int(re.search(r"^#define CRUSE_FFTCONV_PART (\d+)$", hdr_src, flags=re.M).group(1))
    assert part == ops.FFTCONV_PART == F.P


def test_byte_functions_follow_the_layout():
    """one spectrum = 8 P bytes; ws = [B][ceil(L / P)] spectra; spec = [1 | 2][NR][ceil(R / P)] spectra"""
    from cruse_amd._lib import lib
    P = F.P
    one = 8 * P
    assert lib.cruse_fftconv_ws_bytes(1, 1) == one and lib.cruse_fftconv_spec_bytes(1, 1, 0) == one and lib.cruse_fftconv_spec_bytes(1, 1, 1) == 2 * one
    assert lib.cruse_fftconv_ws_bytes(64, 64000) == 64 * 32 * one == 33554432
    assert lib.cruse_fftconv_spec_bytes(32, 8000, 1) == 2 * 32 * 4 * one
    for n, blocks in ((P - 1, 1), (P, 1), (P + 1, 2), (2 * P, 2), (2 * P + 1, 3), (1 << 30, (1 << 30) // P)):
        assert lib.cruse_fftconv_ws_bytes(3, n) == 3 * blocks * one, n
        assert lib.cruse_fftconv_spec_bytes(5, n, 0) == 5 * blocks * one and lib.cruse_fftconv_spec_bytes(5, n, 7) == 10 * blocks * one, n
    assert lib.cruse_fftconv_ws_bytes(0, 5) == 0 and lib.cruse_fftconv_ws_bytes(5, 0) == 0 and lib.cruse_fftconv_spec_bytes(0, 5, 0) == 0


def test_refusals_come_before_any_device_call():
    """host pointers, never dereferenced, on a machine that may have no device at all"""
    from cruse_amd._lib import lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 40
    err = lambda: lib.cruse_last_error()

    def apply(x=p, B=3, L=100, spec=p, sb=big, NR=3, R=10, idx=None, ws=p, wb=big, y=p, ye=None):
        return lib.cruse_fftconv_apply(x, B, L, spec, sb, NR, R, idx, ws, wb, y, ye, None)

    for kw, word in ((dict(x=None), b"x is null"), (dict(spec=None), b"spec is null"), (dict(ws=None), b"ws is null"), (dict(y=None), b"y is null"),
                     (dict(B=0), b"B = 0"), (dict(L=0), b"L = 0"), (dict(NR=0), b"NR = 0"), (dict(R=-1), b"R = -1"), (dict(L=(1 << 30) + 1), b"L = "),
                     (dict(NR=2), b"h_index"), (dict(sb=3 * 8 * F.P - 1), b"spec_bytes"), (dict(wb=3 * 8 * F.P - 1), b"ws_bytes"),
                     (dict(sb=3 * 8 * F.P, ye=p), b"spec_bytes"), (dict(B=1 << 20, L=1 << 30, NR=1), b"workgroups")):
        assert apply(**kw) == E_SHAPE and word in err(), (kw, err())
    assert apply(sb=3 * 8 * F.P, wb=3 * 8 * F.P, spec=p + 4) == -2                   # CRUSE_E_ALIGN: sizes were enough, nothing launched

    def prepare(h=p, NR=3, R=10, el=None, spec=p, sb=big):
        return lib.cruse_fftconv_prepare(h, NR, R, el, spec, sb, None)

    for kw, word in ((dict(h=None), b"h is null"), (dict(spec=None), b"spec is null"), (dict(NR=0), b"NR = 0"), (dict(R=0), b"R = 0"),
                     (dict(sb=3 * 8 * F.P - 1), b"spec_bytes"), (dict(sb=3 * 8 * F.P, el=p), b"spec_bytes"), (dict(NR=65536), b"NR = 65536")):
        assert prepare(**kw) == E_SHAPE and word in err(), (kw, err())
    assert lib.cruse_peak_scale(None, p, 1, 1, 1e-7, p, None) == E_SHAPE and lib.cruse_peak_scale(p, p, 0, 1, 1e-7, p, None) == E_SHAPE


@pytest.mark.parametrize("L", F.gpu_lengths())
def test_restatement_is_within_the_bar(L):
    """the bar is reachable by the partition schedule in plain f32 at every shape the GPU test runs"""
    worst = 0.0
    for R in F.gpu_taps():
        for B, bank in F.BANKS[1:]:
            x, h, idx, hb = F.case(B, L, R, bank)
            r = F.ratio(F.restatement(x, hb), x, hb)
            worst = max(worst, r)
            assert r <= 1.0, (L, R, B, bank, r)
    print(f"L = {L}: worst error / bar of the restatement {worst:.3f}")


def test_restatement_on_the_training_shape():
    x, h = F.signal_like(2, 64000, 3), F.synth_rir(2, 8000, 5)
    r = F.ratio(F.restatement(x, h), x, h)
    print(f"L = 64000, R = 8000: error / bar {r:.3f}")
    assert r <= 1.0


def test_restatement_add_reverb_reproduces_g23(golden):
    g = golden("g23_add_reverb.npz")
    for b, name in enumerate(("peak7", "late", "negative")):
        x, rir = g["clean"][b], g[f"{name}/rir"][:, 0]
        want = (g[f"{name}/wav_tgt"][:, 0], g[f"{name}/wav_early_tgt"][:, 0])
        et = int(F.early_len(rir)[0])
        assert et == {"peak7": 807, "late": 950, "negative": 807}[name] and (et > len(rir)) == (name == "late")
        assert np.array_equal(want[0], want[1]) == (name == "late")
        if name == "negative":
            assert np.abs(rir).argmax() == 400 and rir.argmax() == 7
        for got64, w in zip(F.add_reverb(x, rir), want):                            # float64 against the reference's float64
            assert np.abs(got64[0] - w).max() <= 1e-12 * np.abs(w).max()
        cut = np.where(np.arange(len(rir)) < et, rir, 0).astype(np.float32)
        full, early = F.restatement(x, rir, early_len=et)
        assert F.ratio(full, x, rir, want[0][None]) <= 1.0 and F.ratio(early, x, cut, want[1][None]) <= 1.0


def test_configs_and_defaults():
    from tools.train_stand import load_toml
    from cruse_amd.data import DevicePairs
    rev = load_toml(os.path.join(ROOT, "configs", "cruse_reverb.toml"))
    base = load_toml(os.path.join(ROOT, "configs", "cruse_device_dataset.toml"))
    args = dict(rev["train_dataset"]["args"])
    assert (args.pop("reverb_proportion"), args.pop("reverb_noise_proportion"), args.pop("reverb_target")) == (0.5, 0.3, "early")
    assert args == base["train_dataset"]["args"] and rev["train_dataset"]["path"] == "cruse_amd.data.DevicePairs"
    assert {k: v for k, v in rev.items() if k != "train_dataset"} == {k: v for k, v in base.items() if k != "train_dataset"}
    assert {k: v for k, v in rev["train_dataset"].items() if k != "args"} == {k: v for k, v in base["train_dataset"].items() if k != "args"}
    sig = inspect.signature(DevicePairs.__init__).parameters
    want = dict(num=2048, length=64000, seed=0, pool=128, snr_low=0.0, snr_high=20.0, eq_prob=0.0, eq_filters=3, hp_prob=0.0,
                reverb_proportion=0.0, reverb_noise_proportion=0.0, reverb_target="full", rir_pool=32, rir_len=8000, rt60_low=0.2, rt60_high=0.8,
                predelay=50)
    assert {k: v.default for k, v in sig.items() if k != "self"} == want
    d = DevicePairs()
    assert not d.augments and not d.reverberates and d.reverb_index is None and d.aug_coefs is None
    r = DevicePairs(**rev["train_dataset"]["args"])
    assert r.reverberates and not r.augments and r.reverb_target == "early"
    assert DevicePairs(eq_prob=0.5).augments and not DevicePairs(eq_prob=0.5).reverberates
    assert DevicePairs(reverb_noise_proportion=0.1).reverberates


def test_index_draws():
    from cruse_amd.data import DevicePairs
    kw = dict(seed=9, reverb_proportion=0.5, reverb_noise_proportion=0.3, rir_pool=5)
    a, b = DevicePairs(**kw), DevicePairs(**kw)
    n = 2000
    for p in (0.5, 0.3):
        ia, ib = a.draw_reverb_index(n, p), b.draw_reverb_index(n, p)
        assert ia.dtype == np.int32 and ia.shape == (n,) and np.array_equal(ia, ib)
        assert ia.min() == -1 and ia.max() == 4 and set(ia.tolist()) == {-1, 0, 1, 2, 3, 4}
        hit, sigma = int((ia >= 0).sum()), (n * p * (1 - p)) ** 0.5
        assert abs(hit - n * p) <= 4 * sigma, (p, hit)
    assert not np.array_equal(a.draw_reverb_index(n, 0.5), DevicePairs(**dict(kw, seed=10)).draw_reverb_index(n, 0.5))
    assert (DevicePairs(**kw).draw_reverb_index(50, 0.0) == -1).all() and (DevicePairs(**kw).draw_reverb_index(50, 1.0) >= 0).all()


def test_eq_draws_do_not_depend_on_reverb():
    from cruse_amd.data import DevicePairs
    eq = dict(seed=4, eq_prob=0.5, eq_filters=3, hp_prob=0.5)
    off, on = DevicePairs(**eq), DevicePairs(reverb_proportion=0.5, reverb_noise_proportion=0.3, **eq)
    for _ in range(3):
        on.draw_reverb_index(64, 0.5)
        on.draw_reverb_index(64, 0.3)
        assert np.array_equal(off.draw_aug_coefs(64), on.draw_aug_coefs(64))


def test_argument_errors():
    import torch
    from cruse_amd.data import DevicePairs, add_reverb
    from dataset.dataset import SynDataset
    for bad in (dict(reverb_proportion=-0.1), dict(reverb_proportion=1.1), dict(reverb_noise_proportion=2.0), dict(reverb_target="late"),
                dict(rir_len=0), dict(rt60_low=0.9, rt60_high=0.8)):
        with pytest.raises(ValueError):
            DevicePairs(**bad)
    with pytest.raises(NotImplementedError):
        add_reverb(torch.zeros(8), torch.ones(4), channels=2)
    with pytest.raises(NotImplementedError):
        SynDataset.add_reverb(torch.zeros(8), torch.ones(4, 2))
    with pytest.raises(RuntimeError):
        add_reverb(torch.zeros(8), torch.ones(4))                                  # host tensors: there is no CPU path
