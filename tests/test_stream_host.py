"""CPU: the per-frame restatement of streaming inference (tests/stream_ref.py) reproduces the oracle's offline waveform.

This pins the block contract of cruse_amd.inferencer.StreamingInferencer (frame 0 reflected, the end frame end-reflected,
one previous row per encoder level, one h per GRU, overlap-add divided by the window envelope), so that the GPU tests can
compare the kernels with the restatement's per-frame intermediates."""
import pytest
import torch

from oracle import cruse_oracle as O
from tests.stream_ref import as_double, frame_of, nontrivial_bn, stream_clip
from tests.stream_shapes import SHAPES, geometry, kq_of
from tests.util import rel_l2

CONFIGS = [dict(rnn_groups=4), dict(rnn_groups=1), dict(ch=(1, 4, 8, 16, 32), rnn_groups=2)]


def oracle_model(cfg):
    m = O.unet_2(**cfg)
    O.closed_form_init(m)
    nontrivial_bn(m)
    return m.eval()


def offline(m, x):
    with torch.no_grad():
        _, est, _ = O.enhanced_spectrum(m, x.view(1, -1))
        return O.istft(torch.complex(est[..., 0], est[..., 1]).transpose(1, 2), 320, 160, 320, length=x.numel()).view(-1)


@pytest.mark.parametrize("cfg", CONFIGS, ids=["g4", "g1", "small_g2"])
def test_per_frame_restatement_equals_offline(cfg):
    m = oracle_model(cfg)
    x, _ = O.synth_pair(1, 160 * 60, seed=11)
    got, frames = stream_clip(m, x.view(-1))
    ref = offline(m, x)
    assert got.shape == ref.shape and len(frames) == 61
    err = rel_l2(got, ref)
    print(f"{cfg}: streaming restatement vs offline rel-L2 {err:.2e}")
    assert err <= 1e-6


def test_frames_are_the_reflect_padded_stft_frames():
    x, _ = O.synth_pair(1, 160 * 5, seed=2)
    x = x.view(-1)
    xp = torch.nn.functional.pad(x.view(1, 1, -1), (160, 160), mode="reflect").view(-1)
    for t in range(6):
        assert torch.equal(frame_of(x, t), xp[160 * t:160 * t + 320])


def test_shortest_clip_two_blocks():
    m = oracle_model(dict(ch=(1, 4, 8, 16, 32), rnn_groups=2))
    x, _ = O.synth_pair(1, 320, seed=4)
    got, _ = stream_clip(m, x.view(-1))
    assert rel_l2(got, offline(m, x)) <= 1e-6


STAGE_KEYS = ("e1", "e2", "e3", "e4", "skip1", "skip2", "skip3", "skip4", "gru1", "gru2", "mask", "block")


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_matrix_f32_restatement_equals_f64_and_offline(name):
    """The new shapes of tests/stream_shapes.py: the f64 restatement (the reference of tests/test_gpu_stream_shapes.py) agrees with the
    f32 one stage by stage and over a 12-block clip, and the f32 one with the oracle's offline path.  The bars are those the
    kernels are held to (1e-5 rel-L2 per stage, 2e-5 per clip): the f32 restatement is one valid f32 evaluation order, so it has to
    pass them too.  Its rounding measures 3e-7 .. 6e-7 per stage (clips 1.7e-7 .. 3.3e-7) except at the widest rows, where skip3 sums
    306 cancelling terms per output: 5.6e-6 (clip 1.1e-6)."""
    cfg = SHAPES[name]
    m = oracle_model(cfg)
    x = O.synth_pair(1, 160 * 12, seed=11)[0].view(-1)
    got32, fr32 = stream_clip(m, x)
    got64, fr64 = stream_clip(as_double(m), x, dtype=torch.float64)
    assert got32.dtype == torch.float32 and got64.dtype == torch.float64 and fr64[3]["gru2"].dtype == torch.float64
    worst = 0.0
    for t, (a, b) in enumerate(zip(fr32, fr64)):
        worst = max(worst, rel_l2(torch.complex(a["re"], a["im"]), torch.complex(b["re"], b["im"])))
        for k in STAGE_KEYS:
            if k != "block" or t >= 1:
                worst = max(worst, rel_l2(a[k], b[k]))
    clip = rel_l2(got32, got64)
    off = rel_l2(got32, offline(m, x))
    _, g, H, Hg = geometry(cfg)
    print(f"{name}: H {H} g {g} Hg {Hg} KQ {kq_of(Hg)}: f32 vs f64 restatement worst stage {worst:.2e}, clip {clip:.2e}; "
          f"f32 restatement vs offline {off:.2e}")
    assert len(fr32) == len(fr64) == 13
    assert worst <= 1e-5 and clip <= 2e-5 and off <= 2e-5


def test_shape_matrix_covers_every_gru_instantiation():
    assert {kq_of(geometry(c)[3]) for c in SHAPES.values()} == {3, 5, 10, 16}
    assert any(geometry(c)[3] < 64 for c in SHAPES.values()) and any(geometry(c)[3] % 64 for c in SHAPES.values())
    for c in SHAPES.values():       # the widths the table claims are those the modules have
        assert oracle_model(c).gru.gru_list1[0].hidden_size == geometry(c)[3]


def test_restatement_refuses_mismatched_dtype():
    m = oracle_model(dict(ch=(1, 2, 2, 2, 2), rnn_groups=1))
    with pytest.raises(ValueError, match="as_double"):
        stream_clip(m, torch.zeros(320), dtype=torch.float64)
