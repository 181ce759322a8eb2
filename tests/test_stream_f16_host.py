"""CPU: the f16-operand streaming mode (StreamingInferencer(precision="f16"), cruse_stream_gru*_f16) -- what can be pinned without a GPU.

The emulation (tests/stream_ref_f16.py) is the reference the GPU module measures the kernels against; here it is pinned to torch.nn.GRU
(rounding off) and shown to stay inside the project's reduced-precision bar of 1e-3 per stage on the very models and clips the GPU module
uses, so that the bar is reachable by the reference alone.  Interface checks: the constructor keyword, the three C entry points."""
import inspect
import os
import re

import pytest
import torch

from tests import stream_ref_f16 as R
from tests.stream_ref import as_double, stream_clip
from tests.stream_shapes import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cruse_stream_gru_f16", "cruse_stream_gru_proj_n_f16", "cruse_stream_gru_rec_n_f16")


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_cell_without_rounding_is_torch_gru(name):
    o = R.oracle_model(R.CONFIGS[name])
    od = as_double(o)
    x = R.clip(20, 5)
    ref, frames = stream_clip(od, x, dtype=torch.float64)
    emu, frames_e = R.emulate_clip(od, x, dtype=torch.float64, rounding=False)
    worst = max(R.stage_distance(frames_e, frames).values())
    print(f"{name}: unrounded cell vs nn.GRU in float64: clip {R.rel(emu, ref):.2e}, worst stage {worst:.2e}")
    assert R.rel(emu, ref) <= 1e-12 and worst <= 1e-12


def _distance(o, x):
    ref, frames64, emu, frames16, e_clip = R.references(o, x)
    st = R.stage_distance(frames16, frames64)
    return e_clip, st


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_emulation_inside_the_bar_accuracy_clips(name):
    o = R.oracle_model(R.CONFIGS[name])
    e_clip, st = _distance(o, R.clip(R.ACC_BLOCKS, R.ACC_SEED))
    k = max(st, key=st.get)
    print(f"{name}: emulation vs float64, 2 s: clip {e_clip:.2e}, worst stage {st[k]:.2e} ({k})")
    assert all(st[k] <= R.BAR_F32 for k in R.STAGES_F32), st          # nothing in front of the GRU is rounded
    assert all(st[k] <= R.BAR_F16 for k in R.STAGES_F16), st
    assert 0.0 < e_clip <= R.BAR_F16                                   # and the rounding is really on


@pytest.mark.parametrize("name", list(SHAPES))
def test_emulation_inside_the_bar_shape_matrix(name):
    x = R.clip(R.SHAPE_BLOCKS, R.SHAPE_SEED)
    o, seed = R.alive_model(SHAPES[name], x)
    e_clip, st = _distance(o, x)
    k = max(st, key=st.get)
    print(f"{name}: model seed {seed}: emulation vs float64, 12 blocks: clip {e_clip:.2e}, worst stage {st[k]:.2e} ({k})")
    assert all(st[k] <= R.BAR_F32 for k in R.STAGES_F32), st
    assert all(st[k] <= R.BAR_F16 for k in R.STAGES_F16), st
    assert 0.0 < e_clip <= R.BAR_F16


def test_constructor_accepts_precision():
    """signature inspection only: no device is touched (the library is built before the CPU suite runs, as for tests/test_host.py)"""
    from cruse_amd.inferencer.streaming import StreamingInferencer
    p = inspect.signature(StreamingInferencer.__init__).parameters
    assert "precision" in p and p["precision"].default == "f32"
    assert list(p)[:9] == ["self", "model", "n_slots", "n_fft", "hop_length", "win_length", "device", "use_graph", "max_hops"]


def test_new_entry_points_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    lib_py = open(os.path.join(ROOT, "cruse_amd", "_lib.py")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\bint {sym}\(", header), f"{sym} is not declared in include/cruse_hip.h"
        assert re.search(rf"\"{sym}\":\s*\(\"[a-zA-Z]+\",\s*\"i\"\)", lib_py), f"{sym} is not in cruse_amd/_lib.py:SIGNATURES"
    assert "#define CRUSE_ABI_VERSION 15" in header                    # (15: cruse_gemm_bf16_plan)


def test_weight_pack_layout():
    """ops.stream_pack_f16 restated: lane l of (unit tile, k step) holds W[ut*16 + (l & 15)][ks*32 + (l >> 4)*8 + j], zero padded"""
    from cruse_amd import ops
    g, Hg = 2, 20                                                      # UT = 2 (4 padded units), KS = 1 (12 padded k)
    gen = torch.Generator().manual_seed(0)
    w_ih, w_hh = torch.randn(g, 3 * Hg, Hg, generator=gen), torch.randn(g, 3 * Hg, Hg, generator=gen)
    p = ops.stream_pack_f16(w_ih, w_hh).view(2, g, 3, 2, 1, 64, 8)
    assert p.dtype == torch.float16
    for m, w in enumerate((w_ih, w_hh)):
        for gi in range(g):
            for c in range(3):
                for ut in range(2):
                    for lane in range(64):
                        for j in range(8):
                            u, k = ut * 16 + (lane & 15), (lane >> 4) * 8 + j
                            want = w[gi, c * Hg + u, k].half() if u < Hg and k < Hg else torch.tensor(0.0).half()
                            assert p[m, gi, c, ut, 0, lane, j] == want, (m, gi, c, ut, lane, j)


def test_alive_model_rejects_a_dead_encoder():
    """seed 0 at ch = (1,2,2,2,2) leaves one element of e2 alive; the matrix must not measure a rel-L2 on that.  The rule moves exactly
    two of the twelve models off seed 0: hg20_g1 and hg200_odd (e2: 4 of 200 alive)"""
    x = R.clip(R.SHAPE_BLOCKS, R.SHAPE_SEED)
    o, seed = R.alive_model(SHAPES["hg20_g1"], x)
    assert seed != 0
    assert {n: R.alive_model(c, x)[1] for n, c in SHAPES.items() if n in ("hg200_odd", "hg320_g2", "hg100_odd")} == \
        {"hg200_odd": 1, "hg320_g2": 0, "hg100_odd": 0}
    _, frames = stream_clip(as_double(R.oracle_model(SHAPES["hg20_g1"], 0)), x, dtype=torch.float64)
    assert int((frames[1]["e2"] != 0).sum()) <= 2
    assert R.alive_model(R.CONFIGS["g4"], x)[1] == 0
