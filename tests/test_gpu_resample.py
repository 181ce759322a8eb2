"""GPU: cruse_resample_poly (ops.resample_poly) against float64 scipy.signal.resample_poly with the designed taps.

The bar is measured per case, as tests/test_gpu_fftconv.py does: 4 x the error of scipy's own f32 resample_poly on that case against
float64, in rel-L2 and in max |d| / peak, the rel-L2 bar never above 1e-6 and neither below 4 * 2^-23 (a clip of one sample is a
single product, where scipy-f32 can be exact by luck); each case first asserts that scipy-f32 itself is inside the cap.  Every case
prints its error / bar.  Measured on an MI355X over every case of this file: rel-L2 1.0e-7 to 1.9e-7 at the five staged rates and up to
3.6e-7 at 192 kHz; worst rel-L2 error / bar 0.281 staged (44.1 kHz, Lout = 1025) and 0.356 at 192 kHz, worst max-abs error / bar 0.373."""
import numpy as np
import pytest
import torch

import filepairs_ref as R
from cruse_amd import resample_design as D

pytestmark = pytest.mark.gpu

SENT = 12345.678
PAD = 64
TILE = 1024
# the five pairs of the issue and 192 kHz: its window of (TILE - 1) * 12 + 386 inputs does not fit the staged 8192 -- the direct path
RATES = R.RATES + (192000,)


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(clips, up, down, channels=1, channel=0):
    """clips: flat arrays (f32 mono or int16 interleaved) -> the outputs per clip; 64 sentinels on both sides of the output stay"""
    from cruse_amd import ops
    frames = np.array([len(c) // channels for c in clips], dtype=np.int64)
    louts = np.array([D.out_len(n, up, down) for n in frames], dtype=np.int64)
    off_in = np.concatenate([[0], np.cumsum(frames)])
    off_out = PAD + np.concatenate([[0], np.cumsum(louts)])
    out = torch.full((int(off_out[-1]) + PAD,), SENT, device="cuda")
    got = ops.resample_poly(dv(np.concatenate(clips)), off_in, off_out, up, down, out, channels=channels, channel=channel)
    torch.cuda.synchronize()
    assert got is out
    o = out.cpu().numpy()
    assert np.all(o[:PAD] == np.float32(SENT)) and np.all(o[-PAD:] == np.float32(SENT))
    return [o[off_out[b]:off_out[b + 1]] for b in range(len(clips))]


def length_for(lout, up, down):
    """the smallest L whose output has at least `lout` samples (exactly `lout` unless up > down skips it: at 2 / 1 every length is even)"""
    L = max(1, (lout - 1) * down // up)
    while D.out_len(L, up, down) < lout:
        L += 1
    assert lout <= D.out_len(L, up, down) <= lout + (up - 1) // down
    return L


def judge(got, x32, up, down, what):
    want, b2, bm = R.bars(x32, up, down)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    e2, em = R.errors(got, want)
    print(f"{what}: rel-L2 {e2:.2e} / bar {b2:.2e} = {e2 / b2:.3f}, max-abs {em:.2e} / bar {bm:.2e} = {em / bm:.3f}")
    assert e2 <= b2 and em <= bm, (what, e2, b2, em, bm)
    return e2 / b2


def test_constant():
    from cruse_amd import ops
    assert ops.RESAMPLE_TILE == TILE


@pytest.mark.parametrize("rate", RATES)
def test_lengths_against_float64(rate):
    up, down = D.ratio(R.POOL_RATE, rate)
    worst = 0.0
    for L in (1, 7, down, 1237, length_for(TILE, up, down), length_for(TILE + 1, up, down)):
        x = R.harmonic(L, rate, 100 + L).astype(np.float32)
        got, = run([x], up, down)
        worst = max(worst, judge(got, x, up, down, f"{rate} Hz ({up}/{down}) L = {L} -> {got.shape[0]}"))
    print(f"{rate} Hz: worst rel-L2 error / bar {worst:.3f}")


def stereo_batch(rate=44100):
    """(1, 1237, 4410) frames of stereo interleaved int16; channel 1 carries the signal under test, channel 0 another one"""
    clips, want = [], []
    for k, L in enumerate((1, 1237, 4410)):
        c1, c0 = R.to_pcm(R.harmonic(L, rate, 40 + k)), R.to_pcm(R.harmonic(L, rate, 80 + k, f0=333.0))
        clips.append(np.stack([c0, c1], axis=1).reshape(-1))
        want.append(c1.astype(np.float32) / np.float32(32768.0))
    return clips, want


@pytest.mark.parametrize("rate", (44100, 192000))
def test_ragged_stereo_pcm_batch_reads_channel_one(rate):
    up, down = D.ratio(R.POOL_RATE, rate)
    clips, x32 = stereo_batch(rate)
    got = run(clips, up, down, channels=2, channel=1)
    for b, (g, x) in enumerate(zip(got, x32)):
        judge(g, x, up, down, f"stereo s16 clip {b} at {rate} Hz")
    other = run(clips, up, down, channels=2, channel=0)
    assert R.errors(other[2], got[2])[0] > 0.1                             # channel 0 is another signal
    # a clip alone gives the samples it gives inside the batch, bit for bit -- also as mono f32 of the same values
    for b in (1, 2):
        alone, = run([clips[b]], up, down, channels=2, channel=1)
        assert np.array_equal(alone.view(np.uint32), got[b].view(np.uint32)), b
        mono, = run([x32[b]], up, down)
        assert np.array_equal(mono.view(np.uint32), got[b].view(np.uint32)), b


def test_unit_ratio_is_the_exact_conversion():
    from cruse_amd import ops
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)        # all 65 536 values
    got, = run([pcm], 1, 1)
    assert torch.equal(torch.from_numpy(got.copy()), torch.from_numpy(pcm).float() / 32768.0)
    got, = run([pcm], 48000, 48000)                                        # reduced by the wrapper
    assert np.array_equal(got, pcm.astype(np.float32) / np.float32(32768.0))
    inter = np.stack([pcm, pcm[::-1]], axis=1).reshape(-1)                 # de-interleave alone
    a, b = run([inter[:2000], inter[2000:]], 1, 1, channels=2, channel=1)
    assert np.array_equal(np.concatenate([a, b]), pcm[::-1].astype(np.float32) / np.float32(32768.0))
    x = R.harmonic(3001, 16000, 9).astype(np.float32)
    got, = run([x], 1, 1)
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from cruse_amd import ops
    up, down = D.ratio(R.POOL_RATE, 44100)
    clips, _ = stereo_batch()
    frames = np.array([len(c) // 2 for c in clips], dtype=np.int64)
    off_in = np.concatenate([[0], np.cumsum(frames)])
    off_out = np.concatenate([[0], np.cumsum([D.out_len(n, up, down) for n in frames])])
    src, di, do = dv(np.concatenate(clips)), dv(off_in), dv(off_out)
    outs = [torch.zeros(int(off_out[-1]), device="cuda") for _ in range(3)]
    for o in outs[:2]:
        ops.resample_poly(src, off_in, off_out, up, down, o, channels=2, channel=1, off_in_dev=di, off_out_dev=do)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0.1
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                              # the tap table exists already; no copy, no allocation inside
        ops.resample_poly(src, off_in, off_out, up, down, outs[2], channels=2, channel=1, off_in_dev=di, off_out_dev=do)
    outs[2].fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[2], outs[0])
    src.copy_(torch.flip(src.view(-1, 2), dims=(0,)).reshape(-1))          # the replay reads the buffers, not a snapshot
    ops.resample_poly(src, off_in, off_out, up, down, outs[0], channels=2, channel=1, off_in_dev=di, off_out_dev=do)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[2], outs[0]) and not torch.equal(outs[0], outs[1])


def test_refusals_are_shape_errors_before_any_launch():
    from cruse_amd import ops
    src, out = torch.zeros(4000, device="cuda"), torch.full((8000,), SENT, device="cuda")
    bad = [dict(up=1025, down=1), dict(up=1, down=1031), dict(up=0, down=1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="cruse_hip error -1"):
            ops.resample_poly(src, [0, 4000], [0, 4000], kw["up"], kw["down"], out)            # the ratio is judged before the lengths
    for off_in, off_out in (([0, 4000], [0, 1999]),                        # not ceil(L up / down)
                            ([0, 3000, 2000], [0, 1500, 1000]),            # not monotone
                            ([0, 0], [0, 0]),                              # an empty clip
                            ([-2, 2], [0, 2])):
        with pytest.raises(RuntimeError, match="cruse_hip error -1"):
            ops.resample_poly(src, off_in, off_out, 1, 2, out)
    with pytest.raises(RuntimeError, match="cruse_hip error -1"):
        ops.resample_poly(src, [0, 100], [0, 50], 1, 2, out, channels=2, channel=0)          # f32 is mono
    with pytest.raises(RuntimeError, match="cruse_hip error -1"):
        ops.resample_poly(src.to(torch.int16), [0, 100], [0, 50], 1, 2, out, channels=2, channel=2)
    with pytest.raises(RuntimeError, match="beyond"):
        ops.resample_poly(src, [0, 4001], [0, 2001], 1, 2, out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                       # nothing was launched
