"""No GPU: the schedule of streaming inference in packets (cruse_amd.inferencer.packets), the pure function that push_packet and
enhance follow.  The per-frame reference the GPU tests of the packet path compare with is tests/stream_ref.stream_clip, which
tests/test_stream_host.py already pins to the oracle."""
import random

import pytest

from cruse_amd.inferencer.packets import HOP, flush_plan, packet_plan, padded_blocks


def _run_clip(nb, calls):
    """calls: counts consumed per call; -> (frames computed, output blocks returned), both as lists of clip indices"""
    b, frames, outs = 0, [], []
    for c in calls:
        p = packet_plan(b, c)
        assert p.n_out == (c if b >= 1 else max(c - 1, 0)), (b, c, p)
        assert p.start == min(b, 2)
        frames += list(range(p.first_frame, p.first_frame + p.n_frames))
        outs += list(range(p.first_out, p.first_out + p.n_out))
        b += c
    assert b == nb
    return frames, outs


def test_random_packetisations_compute_every_frame_once_in_order():
    rng = random.Random(20240)
    n = 0
    for K in (1, 2, 3, 4, 8):
        for _ in range(80):
            nb = rng.randint(2, 60)
            calls, left = [], nb
            while left:
                c = 1 if rng.random() < 0.25 else rng.randint(0, K)      # single pushes mixed in, inactive calls (0) too
                c = min(c, left)
                calls.append(c)
                left -= c
            frames, outs = _run_clip(nb, calls)
            assert frames == list(range(nb)), (K, nb, calls)
            assert outs == list(range(nb - 1)), (K, nb, calls)
            f = flush_plan(nb)
            assert (f.first_frame, f.n_frames, f.first_out, f.n_out) == (nb, 1, nb - 1, 1)
            assert (len(outs) + f.n_out) * HOP == nb * HOP                 # pushes + flush return exactly L samples
            n += 1
    assert n == 400


def test_rule_of_n_out_and_frames_at_the_start_of_a_clip():
    assert packet_plan(0, 1)[:4] == (0, 0, 0, 0)                           # block 0 is only stored
    assert packet_plan(0, 4)[:4] == (0, 4, 0, 3)                           # frames 0..3 in one call
    assert packet_plan(1, 4)[:4] == (0, 5, 0, 4)                           # c + 1 frames for c output blocks
    assert packet_plan(2, 4)[:4] == (2, 4, 1, 4)
    assert packet_plan(7, 0).n_frames == 0 and packet_plan(7, 0).n_out == 0
    for b in range(0, 5):                                                  # a packet of one block is a push
        p = packet_plan(b, 1)
        assert p.n_out == (1 if b >= 1 else 0) and p.n_frames == (0, 2, 1, 1, 1)[b]


def test_rejections_and_padding():
    with pytest.raises(ValueError):
        packet_plan(-1, 1)
    with pytest.raises(ValueError):
        packet_plan(0, -1)
    with pytest.raises(ValueError, match="at least 2"):
        flush_plan(1)
    assert [padded_blocks(L) for L in (320, 321, 479, 480, 48000)] == [2, 3, 3, 3, 300]
