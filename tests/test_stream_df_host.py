"""CPU: the schedule of StreamingInferencer(head="df") (inferencer/packets.py: df_packet_plan, df_flush_plan) and the frame-by-frame
restatement of the DeepFilter head on the stream (tests/stream_df_ref.py) against the oracle's offline df waveform.

The second pins that the one-frame lag, the frame-0 rule, the block in front of the clip and the drain step give the OFFLINE result and
not an approximation of it: both sides run in float64 and agree to 1e-9."""
import itertools

import pytest
import torch

from cruse_amd.inferencer.packets import df_flush_plan, df_packet_plan, flush_plan, packet_plan
from oracle import cruse_oracle as O
from tests.stream_df_ref import df_stream, offline_df, product_row, window_sum
from tests.stream_ref import as_double, nontrivial_bn, stream_clip
from tests.util import rel_l2


def _splits(nb, cmax):
    """every way to cut nb blocks into packets of 1..cmax blocks"""
    if nb == 0:
        yield ()
        return
    for c in range(1, min(cmax, nb) + 1):
        for rest in _splits(nb - c, cmax):
            yield (c,) + rest


def test_df_plans_keep_the_frames_of_the_mask_plans():
    for b, c in itertools.product(range(7), range(6)):
        p, q = df_packet_plan(b, c), packet_plan(b, c)
        assert (p.first_frame, p.n_frames, p.start) == (q.first_frame, q.n_frames, q.start)
        assert p.first_out == max(b - 2, 0) and p.n_out == max(b + c - 2, 0) - max(b - 2, 0)
    for b in range(2, 9):
        p, q = df_flush_plan(b), flush_plan(b)
        assert (p.first_frame, p.n_frames, p.start) == (q.first_frame, q.n_frames, q.start)
        assert (p.first_out, p.n_out) == (b - 2, 2)
    for bad in (0, 1):
        with pytest.raises(ValueError):
            df_flush_plan(bad)
    with pytest.raises(ValueError):
        df_packet_plan(-1, 1)


def test_every_split_returns_every_block_once_and_in_order():
    n = 0
    for nb in range(2, 9):
        for split in _splits(nb, 5):
            got, b = [], 0
            for c in (0,) + split + (0,):                   # packets of zero blocks return nothing and change nothing
                p = df_packet_plan(b, c)
                got += list(range(p.first_out, p.first_out + p.n_out))
                b += c
            p = df_flush_plan(b)
            got += list(range(p.first_out, p.first_out + p.n_out))
            assert got == list(range(nb)), (nb, split, got)
            n += 1
    assert n == 242                                         # the compositions of 2..8 into parts of at most 5
    # a slot that has consumed b >= 2 blocks has returned b - 2
    for b in range(2, 8):
        assert sum(df_packet_plan(i, 1).n_out for i in range(b)) == b - 2


CONFIGS = {"small_g2": dict(ch=(1, 4, 8, 16, 32), rnn_groups=2), "g4": dict(rnn_groups=4)}


def _model64(cfg):
    m = O.unet_2(**cfg)
    O.closed_form_init(m)
    nontrivial_bn(m)
    return m.eval(), as_double(m)


@pytest.mark.parametrize("L", [320, 480, 1600])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_restatement_is_the_offline_df_waveform(name, L):
    m32, m64 = _model64(CONFIGS[name])
    x = O.synth_pair(1, L, seed=21)[0].view(-1).double()
    _, frames = stream_clip(m64, x, dtype=torch.float64)
    got, rows = df_stream(frames)
    want = offline_df(m64, x)
    err = rel_l2(got, want)
    far = rel_l2(got, offline_df(m64, x, head="mask"))
    print(f"{name} L {L}: restatement vs offline df {err:.2e} (float64), vs the mask waveform {far:.2f}")
    assert got.dtype == torch.float64 and got.shape == x.shape and rows.shape == (L // 160 + 1, 2, 161)
    assert err <= 1e-9
    assert far > 1.0                                        # the other head's waveform is nowhere near
    # the float64 transform pair is the oracle's own f32 path up to f32 rounding
    assert rel_l2(want, offline_df(m32, x.float()).double()) <= 1e-5


def test_rows_are_the_neighbourhood_sums_of_the_stacked_products():
    """E as the plain double loop over (dt, df) of the definition, on the stacked rows of a clip"""
    _, m64 = _model64(CONFIGS["small_g2"])
    x = O.synth_pair(1, 800, seed=5)[0].view(-1).double()
    _, frames = stream_clip(m64, x, dtype=torch.float64)
    _, rows = df_stream(frames)
    P = torch.stack([product_row(f) for f in frames])       # [T, 2, 161]
    T = P.shape[0]
    want = torch.zeros_like(P)
    for t in range(T):
        for f in range(161):
            for dt in (-1, 0, 1):
                for df in range(-5, 6):
                    if 0 <= t + dt < T and 0 <= f + df < 161:
                        want[t, :, f] += P[t + dt, :, f + df]
    assert rel_l2(rows, want) <= 1e-14
    assert torch.equal(P[:, :, 160], torch.zeros(T, 2, dtype=torch.float64))
    z = torch.zeros(2, 161, dtype=torch.float64)
    assert torch.equal(window_sum(z, z, z), z)


def test_attenuation_limit_of_the_restatement():
    """limit gain 1 (0 dB) returns the input; a gain g mixes g * noisy + (1 - g) * enhanced (the transform is linear)"""
    _, m64 = _model64(CONFIGS["small_g2"])
    x = O.synth_pair(1, 960, seed=9)[0].view(-1).double()
    _, frames = stream_clip(m64, x, dtype=torch.float64)
    full, _ = df_stream(frames)
    assert rel_l2(df_stream(frames, lim=1.0)[0], x) <= 1e-12
    g = 10.0 ** (-12.0 / 20.0)
    assert rel_l2(df_stream(frames, lim=g)[0], g * x + (1.0 - g) * full) <= 1e-12
