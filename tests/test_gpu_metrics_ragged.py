"""GPU: cruse_si_sdr_ragged / cruse_stoi_ragged (csrc/metrics.hip): per-clip lengths read on the device, and ESTOI
against the float64 restatement tests/estoi_ref.py.

Inputs as in tests/test_gpu_metrics.py: seeded harmonic stacks with a zeroed gap, est = ref + white noise at 20 / 5 / -5 dB; every
STOI case first asserts on the CPU that no frame energy of the float64 restatement lies within 0.5 dB of the 40 dB threshold.

Bars.  Ragged against alone, graph replay against eager: torch.equal.  ESTOI score: 40 x the largest distance of the f32 restatement
from the float64 one over the clips of this file, measured on the CPU when the cases are built (1.06e-7 -> 4.2e-6), the ratio section
13c uses for STOI.  Measured on the MI355X: scores within 5.4e-8 of float64."""
import functools

import numpy as np
import pytest
import torch

from tests import estoi_ref as E
from tests import stoi_ref as R

pytestmark = pytest.mark.gpu

SISDR_BAR_DB = 1e-4
NAN = float("nan")

# the shapes of tests/test_gpu_metrics.py: name -> (L, [(seed, gap, snr_db, noise seed)] per clip)
CASES = {
    "short_29": (6400, [(10, None, 5.0, 100)]),                                    # 30 kept frames, nG = 29: 1e-5
    "one_segment": (6553, [(10, None, 5.0, 100)]),
    "ragged_kept": (16037, [(10, (2000, 7000), 20.0, 100), (11, (9000, 13000), -5.0, 101), (12, (3000, 13500), 5.0, 102)]),
    "two_seconds": (32000, [(10, (8000, 20000), 5.0, 100), (11, (1000, 16000), -5.0, 101)]),
}
# ragged equals alone: one full clip, the shortest clip with one segment, a 1e-5 clip (30 frames) and a middle one
RAGGED_L, RAGGED_LEN = 16037, (16037, 6553, 6400, 9000)
RAGGED_CLIPS = [(10, (2000, 7000), 20.0, 100), (11, None, 5.0, 101), (12, None, -5.0, 102), (13, (3000, 4500), -5.0, 103)]


def _clips(L, clips):
    ref = np.stack([R.speechlike(L, seed, gap) for seed, gap, _, _ in clips])
    est = np.stack([R.add_noise(ref[i], snr, ns) for i, (_, _, snr, ns) in enumerate(clips)])
    return ref, est


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (ref, est, float64 ESTOI per clip)} and the f32 restatement's largest distance from float64 -- computed once, shared,
    read-only; asserts the CPU condition on the threshold"""
    out, dist = {}, 0.0
    for name, (L, clips) in CASES.items():
        ref, est = _clips(L, clips)
        want = []
        for i in range(len(clips)):
            st = E.estoi_stages(ref[i], est[i])
            assert R.threshold_margin(st["e"]) >= 0.5, (name, i)
            f32 = E.estoi_stages(ref[i], est[i], np.float32)
            assert np.array_equal(f32["kept"], st["kept"])
            d = abs(f32["score"] - st["score"])
            print(f"{name}[{i}]: kept {len(st['kept'])}  ESTOI float64 {st['score']:.9f}  f32 restatement {f32['score']:.9f}  |d| {d:.2e}")
            dist = max(dist, d)
            want.append(st["score"])
        ref.setflags(write=False); est.setflags(write=False)
        out[name] = (ref, est, want)
    assert 1e-8 < dist < 1e-6, dist                                      # an f32 evaluation's own error, not a disagreement
    return out, dist


@functools.lru_cache(maxsize=None)
def ragged_case():
    """(ref, est) [4, 16037] with NaN beyond every clip's length; asserts the CPU condition on every cut clip"""
    ref, est = _clips(RAGGED_L, RAGGED_CLIPS)
    kept = []
    for b, n in enumerate(RAGGED_LEN):
        st = R.stoi_stages(ref[b, :n], est[b, :n])
        assert R.threshold_margin(st["e"]) >= 0.5, (b, R.threshold_margin(st["e"]))
        kept.append(len(st["kept"]))
        ref[b, n:] = np.nan
        est[b, n:] = np.nan
    assert kept[1] == 31 and kept[2] == 30 and kept[3] >= 31 and kept[3] < R.sizes(9000)[1], kept
    ref.setflags(write=False); est.setflags(write=False)
    return ref, est


def test_a_clip_scores_the_same_in_a_ragged_batch_and_alone():
    """the padding is NaN in ref and est: a kernel that loaded one sample of it would not give a finite score"""
    from cruse_amd import metrics
    ref, est = ragged_case()
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    for how in ("device", "host"):
        lengths = torch.tensor(RAGGED_LEN, device="cuda", dtype=torch.int32) if how == "device" else list(RAGGED_LEN)
        got = {"si_sdr": metrics.si_sdr(r, e, lengths=lengths), "stoi": metrics.stoi(r, e, lengths=lengths),
               "estoi": metrics.estoi(r, e, lengths=lengths), "stoi_ext": metrics.stoi(r, e, extended=True, lengths=lengths)}
        assert torch.equal(got["estoi"], got["stoi_ext"])
        for name in ("si_sdr", "stoi", "estoi"):
            fn = getattr(metrics, name)
            alone = torch.cat([fn(r[b:b + 1, :n].contiguous(), e[b:b + 1, :n].contiguous()) for b, n in enumerate(RAGGED_LEN)])
            print(f"{name} ({how} lengths): ragged {got[name].tolist()}  alone {alone.tolist()}")
            assert bool(torch.isfinite(got[name]).all()), (name, got[name])
            assert torch.equal(got[name], alone), (name, got[name], alone)
        s, x = got["stoi"].cpu().numpy(), got["estoi"].cpu().numpy()
        assert s[2] == np.float32(1e-5) and x[2] == np.float32(1e-5) and (np.delete(s, 2) > 0.1).all() and (np.delete(x, 2) > 0.01).all()
    # [L] with one value, and full lengths given through the keyword against the un-keyworded call
    one = metrics.estoi(r[3], e[3], lengths=RAGGED_LEN[3])
    assert one.dim() == 0 and torch.equal(one, got["estoi"][3])
    full_r, full_e = r[:, :6400].contiguous(), e[:, :6400].contiguous()
    assert torch.equal(metrics.stoi(full_r, full_e, lengths=[6400] * 4), metrics.stoi(full_r, full_e))
    assert torch.equal(metrics.si_sdr(full_r, full_e, lengths=[6400] * 4), metrics.si_sdr(full_r, full_e))


@pytest.mark.parametrize("name", list(CASES))
def test_estoi_against_float64(name):
    from cruse_amd import metrics
    table, dist = cases()
    bar = 40.0 * dist
    ref, est, want = table[name]
    got = metrics.estoi(torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")).cpu().numpy()
    for b in range(ref.shape[0]):
        print(f"{name}[{b}]: ESTOI {got[b]:.9f} vs float64 {want[b]:.9f}  |d| {abs(float(got[b]) - want[b]):.2e}  (bar {bar:.2e} = 40 x {dist:.2e})")
        assert abs(float(got[b]) - want[b]) <= bar, (name, b, got[b], want[b], bar)
        if want[b] == 1e-5:
            assert got[b] == np.float32(1e-5)
    if name == "short_29":
        assert want == [1e-5]
    if name == "ragged_kept":
        assert want[2] == 1e-5 and want[0] > 0.5 > want[1] > 0.01         # kept counts differ inside the batch


def test_estoi_of_all_zero_clips_is_zero():
    from cruse_amd import metrics
    ref = torch.tensor(cases()[0]["two_seconds"][0][:1], device="cuda")
    z = torch.zeros_like(ref)
    assert float(metrics.estoi(z, ref)[0]) == 0.0 and float(metrics.estoi(ref, z)[0]) == 0.0


def test_edge_lengths():
    """len = 0, 1 and 408 (the last length with L10 < 256: no frame) in one batch, NaN beyond.  The row of len = 1 has est = ref / 2:
    alpha = 1/2 and the residual 0 exactly, +inf in numpy and here (any other single pair leaves the residual to the last rounding)."""
    from cruse_amd import metrics
    L, lens = 600, (0, 1, 408)
    ref = np.stack([R.speechlike(L, 40 + b) for b in range(3)])
    est = np.stack([R.add_noise(ref[b], 5.0, 50 + b) for b in range(3)])
    est[1] = 0.5 * ref[1]
    assert ref[1, 0] != 0.0
    with np.errstate(divide="ignore"):
        want = [NAN, R.si_sdr(ref[1, :1], est[1, :1]), R.si_sdr(ref[2, :408], est[2, :408])]
    assert want[1] == np.inf and np.isfinite(want[2])
    for b, n in enumerate(lens):
        ref[b, n:] = np.nan
        est[b, n:] = np.nan
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    ln = torch.tensor(lens, device="cuda", dtype=torch.int32)
    short = torch.full((3,), 1e-5, dtype=torch.float32)
    assert torch.equal(metrics.stoi(r, e, lengths=ln).cpu(), short)
    assert torch.equal(metrics.estoi(r, e, lengths=ln).cpu(), short)
    sd = metrics.si_sdr(r, e, lengths=ln).cpu().numpy()
    print(f"si_sdr of len 0 / 1 / 408: {sd.tolist()} vs {want}")
    assert np.isnan(sd[0]) and sd[1] == np.inf and abs(float(sd[2]) - want[2]) <= SISDR_BAR_DB
    # lengths beyond [0, L] on the device are clamped by the kernels: -5 is 0, L + 7 is L
    wild = torch.tensor([-5, L + 7, 408], device="cuda", dtype=torch.int32)
    r2, e2 = torch.nan_to_num(r, nan=0.25), torch.nan_to_num(e, nan=0.125)
    sd2 = metrics.si_sdr(r2, e2, lengths=wild)
    assert bool(torch.isnan(sd2[0])) and torch.equal(sd2[1:2], metrics.si_sdr(r2[1:2], e2[1:2])) and float(sd2[2]) == float(sd[2])
    assert torch.equal(metrics.estoi(r2, e2, lengths=wild).cpu(), short)


def test_a_captured_graph_replays_with_the_lengths_of_the_moment():
    """the host never reads the lengths: one capture serves every set of lengths written into the tensor it captured"""
    from cruse_amd import metrics
    ref, est = ragged_case()
    r, e = torch.nan_to_num(torch.tensor(ref, device="cuda")), torch.nan_to_num(torch.tensor(est, device="cuda"))
    first = torch.tensor(RAGGED_LEN, device="cuda", dtype=torch.int32)
    other = torch.tensor((9000, 16037, 7000, 0), device="cuda", dtype=torch.int32)
    eager = [metrics.estoi(r, e, lengths=ln).clone() for ln in (first, other, first)]     # (the first call builds tables and workspace)
    assert torch.equal(eager[0], eager[2]) and not torch.equal(eager[0], eager[1])
    dev_len = first.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.estoi(r, e, lengths=dev_len)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0])
    dev_len.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1])


def test_a_ragged_estoi_call_stays_inside_out_and_the_workspace():
    from cruse_amd import metrics, ops
    ref, est = ragged_case()
    B, L = ref.shape
    Y = ops.stoi_layout(B, L)
    pad, sent = 64, 12345.678
    wsbuf = torch.full((Y["total"] + 2 * pad,), sent, device="cuda", dtype=torch.float32)
    outbuf = torch.full((B + 2 * pad,), sent, device="cuda", dtype=torch.float32)
    ws, out = wsbuf[pad:pad + Y["total"]], outbuf[pad:pad + B]
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    ln = torch.tensor(RAGGED_LEN, device="cuda", dtype=torch.int32)
    ops.stoi(r, e, ops.stoi_tables("cuda"), ws, out=out, lengths=ln, extended=True)
    torch.cuda.synchronize()
    for buf, n in ((wsbuf, Y["total"]), (outbuf, B)):
        assert bool((buf[:pad] == sent).all()) and bool((buf[pad + n:] == sent).all()), "a sentinel beside the buffer was overwritten"
    assert torch.equal(out, metrics.estoi(r, e, lengths=ln))
    with pytest.raises(RuntimeError, match="lengths"):
        ops.stoi(r, e, ops.stoi_tables("cuda"), ws, lengths=ln.long())
    with pytest.raises(RuntimeError, match="workspace"):
        ops.stoi(r, e, ops.stoi_tables("cuda"), ws[:-1], lengths=ln, extended=True)
