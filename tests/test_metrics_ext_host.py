"""CPU: the ESTOI definition and the ragged rule of DESIGN section 13f as tests/estoi_ref.py restates them, the two additive C symbols
and their refusals, the extension registry, the host-side judgement of lengths=, and the refusals of evaluate_files that need no
device."""
import ctypes
import os
import re
import wave

import numpy as np
import pytest
import torch

from tests import estoi_ref as E
from tests import stoi_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- restatement properties ---------------------------------------------------------------------------------------------------
def test_estoi_of_a_clip_with_itself_is_one_and_scale_invariant():
    x = R.speechlike(16000, 1)
    y = R.add_noise(x, 5.0, 7)
    assert abs(E.estoi(x, x) - 1.0) <= 1e-9
    s = E.estoi(x, y)
    assert 0.0 < s < 1.0
    assert abs(E.estoi(x, 3.0 * y) - s) <= 1e-9


def test_estoi_decreases_with_white_noise_and_all_zero_inputs_score_zero():
    x = R.speechlike(24000, 2, gap=(6000, 11000))
    s = [E.estoi(x, R.add_noise(x, snr, 7)) for snr in (20.0, 5.0, -5.0)]
    assert 1.0 > s[0] > s[1] > s[2] > 0.0, s
    z = np.zeros_like(x)
    for dt in (np.float64, np.float32):
        assert E.estoi(z, x, dt) == 0.0 and E.estoi(x, z, dt) == 0.0


def test_estoi_of_clips_too_short_for_a_segment_is_1e_5():
    a = R.speechlike(6400, 10)                                           # nF = 30 frames, all kept: nG = 29
    sa = E.estoi_stages(a, R.add_noise(a, 5.0, 1))
    assert sa["tob"].shape[2] == 29 and sa["score"] == 1e-5
    b = R.speechlike(6553, 10)                                           # nG = 30: one segment
    sb = E.estoi_stages(b, R.add_noise(b, 5.0, 1))
    assert sb["tob"].shape[2] == 30 and 0.0 < sb["score"] < 1.0
    assert E.estoi(a[:408], a[:408]) == 1e-5 and R.sizes(408)[0] == 255 and R.sizes(409)[0] == 256     # 408: the last L10 < 256


@pytest.mark.parametrize("length", [16037, 9000, 6553, 6400, 408, 1, 0])
def test_a_cut_clip_is_the_padded_clip_with_an_explicit_length(length):
    """the ragged rule: a clip of `length` samples inside a padded row (NaN beyond, which must not be touched) scores what the cut
    clip scores -- the stages through the padded row against stoi_ref's on the cut arrays"""
    L = 16037
    x = R.speechlike(L, 10, (2000, 3000))                               # the gap removes frames: the kept list matters
    y = R.add_noise(x, 5.0, 100)
    xp, yp = x.copy(), y.copy()
    xp[length:] = np.nan
    yp[length:] = np.nan
    got = E.estoi_stages(xp, yp, length=length)
    if length == 0:
        assert got["score"] == 1e-5 and got["x10"].shape == (2, 0)
        return
    want = E.estoi_stages(x[:length], y[:length])
    assert got["x10"].shape == want["x10"].shape == (2, R.sizes(length)[0])
    assert np.array_equal(got["kept"], want["kept"])
    assert np.abs(got["x10"] - want["x10"]).max() <= 1e-12
    assert got["tob"].shape == want["tob"].shape and (want["tob"].size == 0 or np.abs(got["tob"] - want["tob"]).max() <= 1e-10)
    assert np.isfinite(got["score"]) and abs(got["score"] - want["score"]) <= 1e-9
    assert (got["score"] == 1e-5) == (len(want["kept"]) < 31) == (length <= 6553)      # 6553 loses frames to the gap


# ---- C interface ----------------------------------------------------------------------------------------------------------------
def test_c_symbols_header_and_abi_version():
    from cruse_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert "#define CRUSE_ABI_VERSION 15" in hdr and _lib.ABI_VERSION == 15 and _lib.lib.cruse_abi_version() == 15
    for name in ("cruse_si_sdr_ragged", "cruse_stoi_ragged"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(_lib.lib, name)


def test_every_refusal_of_the_ragged_entry_points_comes_before_a_hip_call():
    from cruse_amd._lib import lib
    p = ctypes.c_void_p(256)                                             # never dereferenced: the calls are refused first
    n = lib.cruse_stoi_ws_bytes(2, 6400)
    for ext in (0, 1):
        assert lib.cruse_stoi_ragged(None, p, 2, 6400, p, ext, p, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, None, 2, 6400, p, ext, p, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 2, 6400, None, ext, p, p, n, p, None) == -1
        assert b"len" in lib.cruse_last_error()
        assert lib.cruse_stoi_ragged(p, p, 2, 6400, p, ext, None, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 2, 6400, p, ext, p, None, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 2, 6400, p, ext, p, p, n, None, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 0, 6400, p, ext, p, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 65536, 6400, p, ext, p, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 2, 0, p, ext, p, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 2, (1 << 28) + 1, p, ext, p, p, n, p, None) == -1
        assert lib.cruse_stoi_ragged(p, p, 64, 1 << 27, p, ext, p, p, n, p, None) == -1          # a workspace beyond 8 GiB
        assert lib.cruse_stoi_ragged(p, p, 2, 6400, p, ext, p, p, n - 4, p, None) == -1
        assert b"workspace" in lib.cruse_last_error()
        assert lib.cruse_stoi_ragged(p, p, 2, 6400, p, ext, p, ctypes.c_void_p(260), n, p, None) == -2
    assert lib.cruse_si_sdr_ragged(None, p, 1, 10, p, p, None) == -1
    assert lib.cruse_si_sdr_ragged(p, None, 1, 10, p, p, None) == -1
    assert lib.cruse_si_sdr_ragged(p, p, 1, 10, None, p, None) == -1
    assert b"len" in lib.cruse_last_error()
    assert lib.cruse_si_sdr_ragged(p, p, 1, 10, p, None, None) == -1
    assert lib.cruse_si_sdr_ragged(p, p, 0, 10, p, p, None) == -1
    assert lib.cruse_si_sdr_ragged(p, p, 1, 0, p, p, None) == -1
    assert lib.cruse_si_sdr_ragged(p, p, 1, (1 << 28) + 1, p, p, None) == -1


# ---- registry and lengths ---------------------------------------------------------------------------------------------------------
def test_extension_registry():
    from cruse_amd import metrics
    from cruse_amd.train.trainer_casual import validation_metrics
    import train_base.metrics as TB
    assert metrics.REGISTERED_METRICS["ESTOI"] is metrics.estoi
    assert "ESTOI" not in metrics.REGISTERED_METRICS and sorted(metrics.REGISTERED_METRICS) == ["SI_SDR", "STOI"]
    assert metrics.EXTENSION_METRICS == {"ESTOI": metrics.estoi}
    assert TB.ESTOI is metrics.estoi and TB.estoi is metrics.estoi and TB.EXTENSION_METRICS is metrics.EXTENSION_METRICS
    assert validation_metrics({"metrics": ["ESTOI", "STOI"]}) == (("ESTOI", "STOI"), "ESTOI")
    with pytest.raises(KeyError, match=r"registered metrics: \['SI_SDR', 'STOI'\]; extension metrics: \['ESTOI'\]"):
        metrics.REGISTERED_METRICS["MOSNET"]
    with pytest.raises(KeyError, match="PESQ is not built"):
        metrics.REGISTERED_METRICS["WB_PESQ"]
    x = torch.zeros(2, 800)
    with pytest.raises(ValueError, match="16000"):
        metrics.estoi(x, x, sr=8000)
    with pytest.raises(ValueError, match="16000"):
        metrics.stoi(x, x, sr=8000, extended=True)


@pytest.mark.parametrize("fn", ["si_sdr", "stoi", "estoi"])
def test_host_lengths_are_judged_before_the_device_is_touched(fn):
    from cruse_amd import metrics
    f = getattr(metrics, fn)
    x = torch.zeros(2, 800)                                              # CPU tensors: a call that got past the judgement would fail otherwise
    for bad in ([800], [800, 800, 800], [[800, 800]], np.array([[800], [800]])):
        with pytest.raises(ValueError, match="lengths"):
            f(x, x, lengths=bad)
    for bad in ([-1, 800], np.array([800, 801]), torch.tensor([0, 10 ** 6])):
        with pytest.raises(ValueError, match=r"0 \.\. L = 800"):
            f(x, x, lengths=bad)
    with pytest.raises(TypeError, match="integer"):
        f(x, x, lengths=[1.5, 2.0])
    x1 = torch.zeros(800)                                                # [L]: None or one value
    with pytest.raises(ValueError, match="lengths"):
        f(x1, x1, lengths=[800, 800])
    with pytest.raises(ValueError, match=r"0 \.\. L = 800"):
        f(x1, x1, lengths=801)
    with pytest.raises(ValueError, match=r"0 \.\. L = 800"):
        f(x1, x1, lengths=[-3])


# ---- evaluate_files ------------------------------------------------------------------------------------------------------------------
def _write_wav(path, frames, rate=16000, channels=1, seed=0):
    pcm = (np.random.default_rng(seed).standard_normal(frames * channels) * 3000).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    return str(path)


def test_evaluate_files_refusals_need_no_device(tmp_path):
    from cruse_amd.evaluate import evaluate_files
    model = torch.nn.Identity()                                          # never run: every call below is refused while reading
    a = _write_wav(tmp_path / "a.wav", 7000)
    b = _write_wav(tmp_path / "b.wav", 8000, seed=1)
    b_short = _write_wav(tmp_path / "b_short.wav", 7999, seed=2)
    b_8k = _write_wav(tmp_path / "b_8k.wav", 8000, rate=8000, seed=3)
    b_stereo = _write_wav(tmp_path / "b_stereo.wav", 8000, channels=2, seed=4)
    with pytest.raises(ValueError, match="2 clean files but 1 noisy"):
        evaluate_files(model, [a, b], [a])
    lst = tmp_path / "clean.txt"
    lst.write_text(a + "\n" + b + "\n")
    with pytest.raises(ValueError, match="2 clean files but 1 noisy"):
        evaluate_files(model, str(lst), [a])
    with pytest.raises(ValueError, match=r"pair 1 .*b\.wav.*b_short\.wav.*8000 frames.*7999 frames"):
        evaluate_files(model, str(lst), [a, b_short])
    with pytest.raises(ValueError, match=r"pair 1 .*16000 Hz.*8000 Hz"):
        evaluate_files(model, [a, b], [a, b_8k])
    with pytest.raises(KeyError, match="registered metrics"):
        evaluate_files(model, [a, b], [a, b], metrics=("STOI", "MOSNET"))
    with pytest.raises(ValueError, match="batch_size"):
        evaluate_files(model, [a, b], [a, b], batch_size=0)
    from cruse_amd.evaluate import read_pairs
    clean, noisy, fc, fn = read_pairs([a, b], [a, b_stereo])             # channels may differ: channel 0 is what is read
    assert fc[1][1] == 1 and fn[1][1] == 2 and fc[1][0].shape[0] == 8000 and fn[1][0].shape[0] == 16000
