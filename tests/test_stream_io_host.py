"""CPU: the streaming I/O modes (per-slot attenuation limit, int16 PCM in / out) -- what can be pinned without a GPU: the gain of a limit
in dB, the four C entry points, the identity the limit's reference rests on, and the PCM quantiser's restatement."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import cruse_oracle as O
from tests import stream_io_ref as IO
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cruse_stream_encode_io", "cruse_stream_decode_io", "cruse_stream_encode_n_io", "cruse_stream_decode_n_io")


def test_atten_lim_gain():
    from cruse_amd import ops
    assert ops.atten_lim_gain(None) == 0.0 and ops.atten_lim_gain(float("inf")) == 0.0
    assert ops.atten_lim_gain(0) == 1.0 and ops.atten_lim_gain(0.0) == 1.0
    assert ops.atten_lim_gain(20) == pytest.approx(0.1, rel=1e-15)
    assert ops.atten_lim_gain(6.0) == pytest.approx(10.0 ** -0.3, rel=1e-15)
    for bad in (-1e-9, -6, float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="non-negative"):
            ops.atten_lim_gain(bad)
    for db in IO.LIMS_DB:                                             # the tests' own restatement agrees
        assert IO.gain(db) == ops.atten_lim_gain(db)


def test_entry_points_declared_and_bound():
    from cruse_amd._abi_check import parse_header
    from cruse_amd._lib import SIGNATURES
    header = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    lib_py = open(os.path.join(ROOT, "cruse_amd", "_lib.py")).read()
    parsed = parse_header()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\bint {sym}\(", header), f"{sym} is not declared in include/cruse_hip.h"
        assert re.search(rf"\"{sym}\":\s*\(\"[a-zA-Z]+\",\s*\"i\"\)", lib_py), f"{sym} is not in cruse_amd/_lib.py:SIGNATURES"
        assert SIGNATURES[sym] == parsed[sym], (sym, SIGNATURES[sym], parsed[sym])
        sib = sym[:-3]                                                # the sibling's arguments plus the format / limit / counter
        extra = 1 if "encode" in sym else 3
        assert len(SIGNATURES[sym][0]) == len(SIGNATURES[sib][0]) + extra, sym
    assert "#define CRUSE_ABI_VERSION 15" in header                   # (15: cruse_gemm_bf16_plan)


def test_constructor_keywords():
    from cruse_amd.inferencer.base_inferencer import Inferencer
    from cruse_amd.inferencer.streaming import StreamingInferencer
    p = inspect.signature(StreamingInferencer.__init__).parameters
    for k in ("atten_lim", "pcm_in", "pcm_out"):
        assert k in p and p[k].default is False
    assert list(p)[:10] == ["self", "model", "n_slots", "n_fft", "hop_length", "win_length", "device", "use_graph", "max_hops", "precision"]
    q = inspect.signature(Inferencer.__init__).parameters
    assert q["atten_lim_db"].default is None


def test_istft_of_stft_is_the_identity():
    """R(x, lim) = lim * x + (1 - lim) * E64(x) describes kernels that mix on the spectrum only because the STFT / iSTFT pair reconstructs
    its input; measured here on the oracle at the clip length the GPU module uses (expected ~1e-7 in float32)"""
    x = IO.clips()
    assert x.shape == (IO.S, 1920)
    y = O.istft(O.stft(x, 320, 160, 320), 320, 160, 320, length=IO.L)
    err = max(rel_l2(y[s], x[s]) for s in range(IO.S))
    print(f"istft(stft(x), length = {IO.L}) vs x, float32 oracle: worst rel-L2 over {IO.S} clips {err:.3e}")
    assert err < 1e-6


def test_passthrough_of_the_reference():
    """lim = 1 makes R the input itself, whatever the model; lim = 0 makes it E64"""
    x = IO.clips()[2]
    e = IO.e64(IO.oracle("hg20_g1"), x)
    assert torch.equal(IO.mix(x, e, 1.0), x.double()) and torch.equal(IO.mix(x, e, 0.0), e)
    assert rel_l2(e, x) > 1e-2                                        # and the model does change the clip: the limit is not vacuous


def test_quantiser_ties_and_range_ends():
    lsb = 1.0 / 32768.0
    cases = [                                                         # (y * 32768, sample, clamped)
        (0.0, 0, False), (0.5, 0, False), (1.5, 2, False), (2.5, 2, False), (3.5, 4, False), (-0.5, 0, False), (-1.5, -2, False),
        (-2.5, -2, False), (0.4375, 0, False), (0.5625, 1, False), (32766.5, 32766, False), (32767.0, 32767, False), (32767.25, 32767, False),
        (32767.5, 32767, True), (32768.0, 32767, True), (131072.0, 32767, True), (-32768.0, -32768, False), (-32768.5, -32768, False),
        (-32769.0, -32768, True), (-32769.5, -32768, True), (-131072.0, -32768, True)]
    y = np.array([c[0] for c in cases], dtype=np.float64) * lsb
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)   # every case is an exact float32
    q, clamped = IO.quantise(y.astype(np.float32))
    assert q.dtype == np.int16
    for (v, want, wc), got, gc in zip(cases, q, clamped):
        assert int(got) == want and bool(gc) == wc, (v, int(got), want, bool(gc), wc)
    # int16 -> float -> int16 is the identity and never clamps
    allv = np.arange(-32768, 32768, dtype=np.int32)
    q, clamped = IO.quantise(allv.astype(np.float32) / np.float32(32768.0))
    assert np.array_equal(q.astype(np.int32), allv) and not clamped.any()


def test_pcm_noise_level():
    v = IO.pcm_noise(1920, 5).double()
    dbfs = 20.0 * np.log10(float(v.pow(2).mean().sqrt()) / 32768.0)
    assert v.dtype == torch.float64 and abs(dbfs + 12.0) < 0.5, dbfs
