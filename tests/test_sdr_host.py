"""CPU: the SDR definition of DESIGN section 13g as tests/sdr_ref.py restates it (its two solvers against each other, three closed
forms), the registry with its third dict, the refusals of metrics.sdr that need no device, the two additive C symbols and their
refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sdr_ref as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# the hard cap of the GPU test, as a condition on the restatement itself
CAP_DB, CAP_REL = 1e-6, 1e-9
# (L, K) of tests/test_gpu_sdr.py with the chunk written out (asserted below), and the 1 s clip of the solver check
CASES = [(700, 8), (1500, 33), (4000, 512), (300, 512), (1, 4), (2048, 16), (2049, 16), (16000, 512)]


# ---- restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,K", CASES)
def test_the_two_solvers_of_the_restatement_agree(L, K):
    ref = S.speechlike(L, 20)
    est = S.distort(ref, 21)
    lu, lev = S.sdr_stages(ref, est, K), S.sdr_stages(ref, est, K, solver="levinson")
    assert np.array_equal(lu["raa"], lev["raa"]) and lu["raa"][0] > 0.0
    print(f"({L}, {K}): score {lu['score']:.9f} dB  |d| {abs(lu['score'] - lev['score']):.2e} dB  C rel-L2 {S.rel(lev['C'], lu['C']):.2e}  "
          f"s_target rel-L2 {S.rel(lev['s_target'], lu['s_target']):.2e}")
    assert S.rel(lev["C"], lu["C"]) <= CAP_REL
    assert S.rel(lev["ss"], lu["ss"]) <= CAP_REL
    if L == 1:                                                           # one sample: e is rounding noise or exactly zero
        assert lu["ee"] <= 1e-24 * lu["ss"] and lev["ee"] <= 1e-24 * lev["ss"]
    else:
        assert np.isfinite(lu["score"]) and abs(lu["score"] - lev["score"]) <= CAP_DB


def test_a_scaled_reference_projects_onto_half_a_delta():
    ref = S.speechlike(3000, 30)
    st = S.sdr_stages(ref, (0.5 * ref.astype(np.float64)).astype(np.float32), 16)      # halving is exact in f32
    want = np.zeros(16)
    want[0] = 0.5
    assert np.abs(st["C"] - want).max() <= 1e-9
    assert st["ee"] <= 1e-18 * st["ss"]                                  # e numerically zero: the dB value is not asserted


def test_a_delayed_reference_projects_onto_a_shifted_delta():
    """ref ends in three zeros, so that the delay pushes nothing out of the clip and delta_3 is the exact solution"""
    ref = np.concatenate([S.speechlike(3000, 31), np.zeros(3, np.float32)])
    est = np.concatenate([np.zeros(3, np.float32), ref[:-3]])
    want = np.zeros(8)
    want[3] = 1.0
    for K in (4, 8):
        st = S.sdr_stages(ref, est, K)
        assert np.abs(st["C"] - want[:K]).max() <= 1e-9
        assert st["ee"] <= 1e-18 * st["ss"]


def test_white_noise_scores_the_signal_to_noise_ratio():
    L = 16000
    ref = S.speechlike(L, 32).astype(np.float64)
    w = np.random.default_rng(33).standard_normal(L)
    w *= np.sqrt((ref ** 2).sum() / (w ** 2).sum() / 10.0)              # 10 dB
    est = (ref + w).astype(np.float32)
    snr = 10.0 * np.log10((ref ** 2).sum() / (w ** 2).sum())
    got = S.sdr(ref.astype(np.float32), est)
    print(f"SDR {got:.4f} dB against an SNR of {snr:.4f} dB")
    assert abs(got - snr) <= 0.5


def test_degenerate_clips_of_the_restatement_are_nan():
    x = S.speechlike(100, 1)
    assert np.isnan(S.sdr(np.zeros(100, np.float32), x, 8))
    assert np.isnan(S.sdr_stages(x, x, 8, length=0)["score"])
    p = x.copy()
    p[40:] = np.nan                                                      # nothing beyond the length is touched
    a, b = S.sdr_stages(p, p, 8, length=40), S.sdr_stages(x[:40], x[:40], 8)
    assert np.array_equal(a["raa"], b["raa"]) and np.array_equal(a["C"], b["C"])


# ---- registry ------------------------------------------------------------------------------------------------------------------------
def test_registry_finds_sdr_without_listing_it():
    from cruse_amd import metrics
    from cruse_amd.train.trainer_casual import validation_metrics
    import train_base.metrics as TB
    assert sorted(metrics.REGISTERED_METRICS) == ["SI_SDR", "STOI"]
    assert metrics.EXTENSION_METRICS == {"ESTOI": metrics.estoi}
    assert metrics.UNREGISTERED_REFERENCE_METRICS == {"SDR": metrics.sdr}
    assert metrics.REGISTERED_METRICS["SDR"] is metrics.sdr and "SDR" not in metrics.REGISTERED_METRICS
    assert metrics.SDR is metrics.sdr and TB.SDR is metrics.sdr and TB.sdr is metrics.sdr
    assert TB.UNREGISTERED_REFERENCE_METRICS is metrics.UNREGISTERED_REFERENCE_METRICS
    assert validation_metrics({"metrics": ["SI_SDR", "SDR"], "score_metric": "SDR"}) == (("SI_SDR", "SDR"), "SDR")
    with pytest.raises(KeyError, match=r"registered metrics: \['SI_SDR', 'STOI'\]; extension metrics: \['ESTOI'\]; .*\['SDR'\]"):
        metrics.REGISTERED_METRICS["MOSNET"]
    with pytest.raises(KeyError, match="PESQ is not built"):
        metrics.REGISTERED_METRICS["NB_PESQ"]


def test_example_config_scores_by_sdr():
    from tools.train_stand import load_toml
    from cruse_amd.train.trainer_casual import validation_metrics
    va = load_toml(os.path.join(ROOT, "configs", "cruse_metrics_sdr.toml"))["trainer"]["validation"]
    assert validation_metrics(va) == (("SI_SDR", "SDR"), "SDR") and va["save_max_metric_score"] is True


def test_refusals_of_metrics_sdr_need_no_device():
    from cruse_amd import metrics
    x = torch.zeros(2, 800)                                              # CPU tensors: a call that got past the judgement would fail otherwise
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.sdr(x, torch.zeros(2, 801))
    for bad in (0, 1025, -3, 512.0, True):
        with pytest.raises(ValueError, match="filter_len"):
            metrics.sdr(x, x, filter_len=bad)
    with pytest.raises(ValueError, match="16000"):
        metrics.sdr(x, x, sr=8000)
    with pytest.raises(TypeError, match="integer"):
        metrics.sdr(x, x, lengths=[1.5, 2.0])
    with pytest.raises(ValueError, match=r"0 \.\. L = 800"):
        metrics.sdr(x, x, lengths=[0, 801])
    with pytest.raises(ValueError, match="lengths"):
        metrics.sdr(x, x, lengths=[800])
    with pytest.raises(ValueError, match="empty"):
        metrics.sdr(torch.zeros(2, 0), torch.zeros(2, 0))


# ---- C interface ----------------------------------------------------------------------------------------------------------------------
def test_c_symbols_header_and_constants():
    from cruse_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert "#define CRUSE_ABI_VERSION 15" in hdr and _lib.lib.cruse_abi_version() == 15
    assert _lib.SIGNATURES["cruse_sdr"] == ("pppiiipppp", "i") and _lib.SIGNATURES["cruse_sdr_ws_bytes"] == ("iii", "z")
    assert re.search(r"\bint cruse_sdr\(", hdr) and re.search(r"\bsize_t cruse_sdr_ws_bytes\(", hdr)
    assert hasattr(_lib.lib, "cruse_sdr") and hasattr(_lib.lib, "cruse_sdr_ws_bytes")
    assert f"#define CRUSE_SDR_CHUNK {ops.SDR_CHUNK}\n" in hdr and f"#define CRUSE_SDR_MAX_TAPS {ops.SDR_MAX_TAPS}\n" in hdr
    assert (ops.SDR_CHUNK, 16) in CASES and (ops.SDR_CHUNK + 1, 16) in CASES
    assert "train_base/metrics.py:55-57" in hdr


def test_workspace_size_and_refusals_come_before_any_hip_call():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    C = ops.SDR_CHUNK
    # part [B][NC][2][K] + C [B][K] + en [B][NT][2] doubles + status [B] ints padded to 8 bytes
    for B, L, K in ((1, 1, 1), (3, C, 512), (3, C + 1, 512), (2, 700, 8), (64, 64000, 512)):
        nc, nt = -(-L // C), -(-(L + K - 1) // C)
        assert lib.cruse_sdr_ws_bytes(B, L, K) == 8 * (B * nc * 2 * K + B * K + B * nt * 2 + (B + 1) // 2), (B, L, K)
    for B, L, K in ((0, 10, 4), (1, 0, 4), (1, 10, 0), (1, 10, 1025), (65536, 10, 4), (1, (1 << 28) + 1, 4)):
        assert lib.cruse_sdr_ws_bytes(B, L, K) == 0, (B, L, K)
    p = ctypes.c_void_p(256)                                             # never dereferenced: the calls are refused first
    bad = [lib.cruse_sdr(None, p, p, 2, 100, 8, p, p, p, None), lib.cruse_sdr(p, None, p, 2, 100, 8, p, p, p, None),
           lib.cruse_sdr(p, p, p, 2, 100, 8, None, p, p, None), lib.cruse_sdr(p, p, p, 2, 100, 8, p, None, p, None),
           lib.cruse_sdr(p, p, None, 0, 100, 8, p, p, None, None), lib.cruse_sdr(p, p, None, 2, 0, 8, p, p, None, None),
           lib.cruse_sdr(p, p, None, 2, 100, 0, p, p, None, None), lib.cruse_sdr(p, p, None, 2, 100, 1025, p, p, None, None),
           lib.cruse_sdr(p, p, None, 65536, 100, 8, p, p, None, None), lib.cruse_sdr(p, p, None, 2, (1 << 28) + 1, 8, p, p, None, None)]
    assert bad == [-1] * len(bad), bad
    assert b"K = 8" in lib.cruse_last_error()
    assert lib.cruse_sdr(p, p, None, 2, 100, 8, ctypes.c_void_p(260), p, None, None) == -2
    assert lib.cruse_sdr(p, p, None, 2, 100, 8, p, p, ctypes.c_void_p(260), None) == -2
