"""Test-only: the references of the streaming I/O modes (StreamingInferencer(atten_lim=..., pcm_in=..., pcm_out=...)), shared by
tests/test_stream_io_host.py (CPU) and tests/test_gpu_stream_io.py.

  R(x, lim) = lim * x + (1 - lim) * E64(x): the attenuation-limited output, E64 the float64 per-frame restatement of tests/stream_ref.py.
      The kernels mix on the spectrum (bins 0..159 scaled by lim + (1 - lim) * mask, bin 160 by lim); the two agree because
      istft(stft(x)) == x, which tests/test_stream_io_host.py pins at the length used here.
  quantise(y): the PCM16 store restated in numpy: clamp(rint(y * 32768), -32768, 32767), ties to even, and which samples were clamped.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import stream_ref_f16 as R
from tests.stream_ref import as_double, stream_clip
from tests.stream_shapes import SHAPES

S, NB, K = 3, 12, 4                       # slots, blocks per clip (L = 1920), max_hops
L = NB * 160
MODELS = {"hg20_g1": SHAPES["hg20_g1"], "g4": R.CONFIGS["g4"]}       # ch (1,2,2,2,2) g 1; the default channels, g 4
LIMS_DB = (None, 6.0, 0.0)                # per slot: no limit, 6 dB, passthrough
CLIP_SEEDS = (300, 301, 302)


def clips() -> torch.Tensor:
    """[S, L]: a different 0.1 * randn clip per slot"""
    return torch.stack([R.clip(NB, seed) for seed in CLIP_SEEDS])


@functools.lru_cache(maxsize=None)
def oracle(name: str):
    """the oracle module of MODELS[name]: for the two-channel model the first seed whose encoder stays alive on slot 0's clip (the
    reference alone decides, see stream_ref_f16.alive_model), seed 0 for the default model"""
    cfg = MODELS[name]
    return R.alive_model(cfg, R.clip(NB, CLIP_SEEDS[0]))[0] if name == "hg20_g1" else R.oracle_model(cfg)


def e64(o, x: torch.Tensor) -> torch.Tensor:
    """E64: the float64 restatement's output for the 1-D clip x"""
    return stream_clip(as_double(o), x, dtype=torch.float64)[0]


def gain(db) -> float:
    """10^(-db / 20); None / inf -> 0"""
    return 0.0 if db is None or db == float("inf") else 10.0 ** (-float(db) / 20.0)


def mix(x: torch.Tensor, enhanced64: torch.Tensor, lim: float) -> torch.Tensor:
    """R(x, lim) in float64"""
    return lim * x.double() + (1.0 - lim) * enhanced64.double()


def quantise(y):
    """(int16 samples, bool clamped) of float32 samples y"""
    v = np.asarray(y, dtype=np.float32) * np.float32(32768.0)         # exact: a power of two
    r = np.rint(v)                                                    # ties to even
    c = np.clip(r, -32768.0, 32767.0)
    return c.astype(np.int16), c != r


def pcm_noise(n: int, seed: int, dbfs: float = -12.0) -> torch.Tensor:
    """n int16 samples of Gaussian noise with an RMS of about `dbfs` dB full scale"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * (32768.0 * 10.0 ** (dbfs / 20.0))
    return v.round().clamp(-32768, 32767).to(torch.int16)
