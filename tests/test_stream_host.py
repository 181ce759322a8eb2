"""CPU: the per-frame restatement of streaming inference (tests/stream_ref.py) reproduces the oracle's offline waveform.

This pins the block contract of cruse_amd.inferencer.StreamingInferencer (frame 0 reflected, the end frame end-reflected,
one previous row per encoder level, one h per GRU, overlap-add divided by the window envelope), so that the GPU tests can
compare the kernels with the restatement's per-frame intermediates."""
import pytest
import torch

from oracle import cruse_oracle as O
from tests.stream_ref import frame_of, nontrivial_bn, stream_clip
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
