"""CPU: the STOI definition of DESIGN section 13 as tests/stoi_ref.py restates it (properties, band edges, resampler design, clips
too short for a segment), the Python interface of cruse_amd.metrics, the additive C symbols, and the trainer's TOML keys."""
import os
import re

import numpy as np
import pytest
import torch

from tests import stoi_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- restatement properties ---------------------------------------------------------------------------------------------------
def test_stoi_of_a_clip_with_itself_is_one_and_scale_invariant():
    x = R.speechlike(16000, 1)
    s = R.stoi(x, x)
    assert abs(s - 1.0) <= 1e-12
    assert abs(R.stoi(x, 3.0 * x) - s) <= 1e-12


def test_stoi_decreases_strictly_with_white_noise():
    x = R.speechlike(24000, 2, gap=(6000, 11000))
    s = [R.stoi(x, R.add_noise(x, snr, 7)) for snr in (20.0, 5.0, -5.0)]
    assert 1.0 > s[0] > s[1] > s[2] > 0.0, s


def test_f32_evaluation_of_the_restatement_is_its_own():
    x = R.speechlike(16000, 3, gap=(2000, 5000))
    y = R.add_noise(x, 5.0, 8)
    a, b = R.stoi_stages(x, y), R.stoi_stages(x, y, np.float32)
    assert b["x10"].dtype == np.float32 and b["tob"].dtype == np.float32
    assert np.array_equal(a["kept"], b["kept"])
    assert 0.0 < abs(a["score"] - b["score"]) <= 1e-6


def test_band_edges_are_pinned():
    lo, hi = R.band_edges()
    assert lo.tolist() == [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
    assert hi.tolist() == [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]


def test_resampler_design():
    """The 257-tap prototype as the issue fixes it.  Its stopband meets the 80 dB asked for (measured 91.7 dB at 5.5 kHz and above).
    Its passband does NOT hold 0.01 dB up to 4 kHz: the -6 dB point is 0.9 * 5 kHz = 4.5 kHz and the Kaiser(9) transition band
    reaches down to 3.6 kHz.  Measured: 3.4e-4 dB up to 3.6 kHz, 0.045 dB at 3.8 kHz, 0.372 dB at 4 kHz.  The design is kept and the
    measured figures are pinned."""
    h = R.design()
    assert h.shape == (257,) and abs(h.sum() - 1.0) < 1e-15 and np.array_equal(h, h[::-1])
    H = np.abs(np.fft.rfft(h, 1 << 16))
    f = np.arange(H.shape[0]) * 80000.0 / (1 << 16)
    db = 20.0 * np.log10(H)
    assert np.abs(db[f <= 3600.0]).max() < 0.01
    assert np.abs(db[f <= 3600.0]).max() < 5e-4
    assert 0.36 < np.abs(db[f <= 4000.0]).max() < 0.38
    assert db[f >= 5500.0].max() <= -80.0
    assert db[f >= 5500.0].max() <= -91.0


def test_resampler_is_zero_phase_and_has_unit_gain():
    L = 4000
    t = np.arange(L) / 16000.0
    u = np.sin(2.0 * np.pi * 1000.0 * t)
    x10 = R.resample(u)
    assert x10.shape == ((5 * L + 7) // 8,)
    want = np.sin(2.0 * np.pi * 1000.0 * np.arange(x10.shape[0]) / 10000.0)
    mid = slice(100, x10.shape[0] - 100)                                 # away from the zero extension at the clip's ends
    assert np.abs(x10[mid] - want[mid]).max() < 1e-4
    for L in (1, 2, 3, 5, 8, 13):                                        # nothing assumes L % 8 == 0
        assert R.resample(np.ones(L)).shape == ((5 * L + 7) // 8,)


def test_clips_too_short_for_a_segment_score_1e_5():
    a = R.speechlike(6400, 10)                                           # nF = 30 frames, all kept: nG = 29
    sa = R.stoi_stages(a, R.add_noise(a, 5.0, 1))
    assert R.sizes(6400) == (4000, 30) and len(sa["kept"]) == 30 and sa["tob"].shape[2] == 29
    assert sa["score"] == 1e-5
    b = R.speechlike(6553, 10)                                           # the shortest clip with nF = 31: nG = 30, one segment
    sb = R.stoi_stages(b, R.add_noise(b, 5.0, 1))
    assert R.sizes(6552)[1] == 30 and R.sizes(6553) == (4096, 31) and len(sb["kept"]) == 31 and sb["tob"].shape[2] == 30
    assert 0.5 < sb["score"] < 1.0
    assert R.stoi(a[:400], a[:400]) == 1e-5                              # L10 = 250 < 256: no frame at all


def test_all_zero_inputs_are_finite():
    x = R.speechlike(16000, 4)
    z = np.zeros_like(x)
    for dt in (np.float64, np.float32):
        assert R.stoi(z, x, dt) == 0.0 and R.stoi(x, z, dt) == 0.0


# ---- interface ------------------------------------------------------------------------------------------------------------------
def test_registry_and_refusals():
    from cruse_amd import metrics
    import train_base.metrics as TB
    assert sorted(metrics.REGISTERED_METRICS) == ["SI_SDR", "STOI"]
    assert metrics.REGISTERED_METRICS["SI_SDR"] is metrics.si_sdr and metrics.REGISTERED_METRICS["STOI"] is metrics.stoi
    assert TB.REGISTERED_METRICS is metrics.REGISTERED_METRICS and TB.STOI is metrics.stoi and TB.SI_SDR is metrics.si_sdr
    for name in ("WB_PESQ", "NB_PESQ"):
        assert name not in metrics.REGISTERED_METRICS
        with pytest.raises(KeyError, match="PESQ is not built"):
            metrics.REGISTERED_METRICS[name]
    with pytest.raises(KeyError, match="registered metrics"):
        metrics.REGISTERED_METRICS["MOSNET"]
    x = torch.zeros(2, 800)
    with pytest.raises(ValueError, match="16000"):
        metrics.stoi(x, x, sr=8000)
    with pytest.raises(ValueError, match="shape"):
        metrics.stoi(x, torch.zeros(2, 801))
    with pytest.raises(ValueError, match="shape"):
        metrics.si_sdr(x, torch.zeros(800))
    with pytest.raises(ValueError, match=r"\[B, L\] or \[L\]"):
        metrics.si_sdr(torch.zeros(1, 2, 800), torch.zeros(1, 2, 800))


def test_c_symbols_header_and_abi_version():
    from cruse_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert "#define CRUSE_ABI_VERSION 15" in hdr and _lib.ABI_VERSION == 15 and _lib.lib.cruse_abi_version() == 15
    for name in ("cruse_si_sdr", "cruse_stoi_layout", "cruse_stoi_ws_bytes", "cruse_stoi_tables", "cruse_stoi"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\b(int|size_t) %s\(" % name, hdr), name
        assert hasattr(_lib.lib, name)


def test_layout_and_refusals_need_no_device():
    """cruse_stoi_layout / _ws_bytes are host-side; every refusal of cruse_stoi and cruse_si_sdr comes before the first HIP call."""
    import ctypes
    from cruse_amd import ops
    from cruse_amd._lib import lib
    for L in (1, 400, 6400, 6553, 16037, 32000):
        Y = ops.stoi_layout(3, L)
        L10, nF = R.sizes(L)
        assert (Y["L10"], Y["nF"]) == (L10, nF) and Y["nGs"] == max(nF - 1, 1)
        nFa = max(nF, 1)
        assert Y["x10"] == 0 and Y["e"] == 6 * L10 and Y["nk"] == Y["e"] + 3 * nFa and Y["kept"] == Y["nk"] + 3
        assert Y["tob"] == Y["kept"] + 3 * nFa and Y["part"] >= Y["tob"] + 90 * Y["nGs"] and Y["part"] % 2 == 0
        assert Y["total"] == Y["part"] + 90 * Y["nSB"] and lib.cruse_stoi_ws_bytes(3, L) == 4 * Y["total"]
    arr = (ctypes.c_int * 11)()
    for B, L in ((0, 100), (1, 0), (1, (1 << 28) + 1), (65536, 100), (64, 1 << 27)):       # the last: a workspace beyond 8 GiB
        assert lib.cruse_stoi_layout(B, L, arr) == -1 and lib.cruse_stoi_ws_bytes(B, L) == 0
    assert lib.cruse_stoi_layout(1, 100, None) == -1
    p = ctypes.c_void_p(256)                                             # never dereferenced: the calls are refused first
    n = lib.cruse_stoi_ws_bytes(2, 6400)
    assert lib.cruse_stoi(None, p, 2, 6400, p, p, n, p, None) == -1
    assert lib.cruse_stoi(p, p, 2, 6400, p, None, n, p, None) == -1
    assert lib.cruse_stoi(p, p, 2, 6400, p, p, n, None, None) == -1
    assert lib.cruse_stoi(p, p, 0, 6400, p, p, n, p, None) == -1
    assert lib.cruse_stoi(p, p, 2, 0, p, p, n, p, None) == -1
    assert lib.cruse_stoi(p, p, 2, (1 << 28) + 1, p, p, n, p, None) == -1
    assert lib.cruse_stoi(p, p, 2, 6400, p, p, n - 4, p, None) == -1
    assert b"workspace" in lib.cruse_last_error()
    assert lib.cruse_stoi(p, p, 2, 6400, p, ctypes.c_void_p(260), n, p, None) == -2
    assert lib.cruse_stoi_tables(None, None) == -1
    assert lib.cruse_si_sdr(None, p, 1, 10, p, None) == -1
    assert lib.cruse_si_sdr(p, p, 0, 10, p, None) == -1
    assert lib.cruse_si_sdr(p, p, 1, 0, p, None) == -1
    assert lib.cruse_si_sdr(p, p, 1, (1 << 28) + 1, p, None) == -1


# ---- trainer ---------------------------------------------------------------------------------------------------------------------
def test_trainer_toml_keys():
    from tools.train_stand import load_toml
    from cruse_amd.train.trainer_casual import validation_metrics
    va = load_toml(os.path.join(ROOT, "configs", "cruse_metrics.toml"))["trainer"]["validation"]
    assert va["metrics"] == ["SI_SDR", "STOI"] and va["score_metric"] == "STOI" and va["save_max_metric_score"] is True
    assert validation_metrics(va) == (("SI_SDR", "STOI"), "STOI")
    assert validation_metrics({"metrics": ["SI_SDR", "STOI"]}) == (("SI_SDR", "STOI"), "SI_SDR")       # default: the first entry
    old = load_toml(os.path.join(ROOT, "configs", "cruse_synthetic.toml"))["trainer"]["validation"]
    assert validation_metrics(old) == ((), None)
    with pytest.raises(KeyError, match=r"registered metrics: \['SI_SDR', 'STOI'\]"):
        validation_metrics({"metrics": ["STOI", "MOSNET"]})
    with pytest.raises(KeyError, match="PESQ is not built"):
        validation_metrics({"metrics": ["STOI", "WB_PESQ"]})
    with pytest.raises(ValueError, match="not in metrics"):
        validation_metrics({"metrics": ["STOI"], "score_metric": "SI_SDR"})
    with pytest.raises(ValueError):
        validation_metrics({"metrics": []})
    with pytest.raises(ValueError):
        validation_metrics({"score_metric": "STOI"})
