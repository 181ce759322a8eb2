"""GPU: cruse_sdr (csrc/sdr.hip) against the float64 restatement tests/sdr_ref.py, stage by stage through the dbg
array; ragged batches, degenerate clips, determinism, graph capture, placement, refusals, and a trainer run scored by SDR.

Signals: seeded speech-like stacks (harmonics on a gliding pitch under a slow envelope plus a noise floor at -30 dB); est = a short FIR
of ref + an independent stack at -20 dB + 0.05 tanh(3 ref).

Bars.  Kernels and restatement are both float64 on identical f32 inputs: they differ by summation order and solver only.  Per case, on
the energy of s_target (relative) and on the score (dB): 100 x the restatement's own LU-against-Levinson difference on that case,
floored at 1e-10 relative and 1e-9 dB.  Hard cap, as a condition: 1e-6 dB on the score, 1e-9 rel-L2 on raa, rab and C; every case
first asserts that the restatement's two solvers are themselves inside the cap.  The case of one sample has an error signal that is
rounding noise (or exactly zero) in any float64 evaluation, so its dB value is not comparable: there the error energy must lie below
1e-24 of the target's (f64 epsilon squared is 5e-32) in the restatement and on the device alike.  Ragged against alone, repeated calls,
graph replay and tail placement: torch.equal.
Measured on the MI355X, worst over the cases: raa 2.4e-15, rab 2.0e-15, C 9.3e-12 rel-L2, s_target energy 7.8e-15
relative, score 3.2e-14 dB."""
import functools

import numpy as np
import pytest
import torch

from tests import sdr_ref as S

pytestmark = pytest.mark.gpu

CAP_DB, CAP_REL = 1e-6, 1e-9
FLOOR_DB, FLOOR_REL = 1e-9, 1e-10
NOISE_EE = 1e-24


def _chunk():
    from cruse_amd import ops
    return ops.SDR_CHUNK


def case_shapes():
    """(L, K): even and odd K, K = 512, n < K, one sample, L of one time chunk and one more than that"""
    return [(700, 8), (1500, 33), (4000, 512), (300, 512), (1, 4), (_chunk(), 16), (_chunk() + 1, 16)]


@functools.lru_cache(maxsize=None)
def case(L, K):
    """(ref [2, L], est [2, L], LU stages per clip, per-clip bars) -- computed once, shared, read-only; asserts the cap on the restatement"""
    ref = np.stack([S.speechlike(L, 20 + 2 * b) for b in range(2)])
    est = np.stack([S.distort(ref[b], 21 + 2 * b) for b in range(2)])
    stages, bars = [], []
    for b in range(2):
        lu, lev = S.sdr_stages(ref[b], est[b], K), S.sdr_stages(ref[b], est[b], K, solver="levinson")
        assert S.rel(lev["C"], lu["C"]) <= CAP_REL and S.rel(lev["ss"], lu["ss"]) <= CAP_REL, (L, K, b)
        noise = lu["ee"] <= NOISE_EE * lu["ss"]
        if noise:
            assert lev["ee"] <= NOISE_EE * lev["ss"]
            d_db = 0.0
        else:
            d_db = abs(lu["score"] - lev["score"])
            assert np.isfinite(lu["score"]) and d_db <= CAP_DB, (L, K, b, d_db)
        bars.append((max(100.0 * S.rel(lev["ss"], lu["ss"]), FLOOR_REL), min(max(100.0 * d_db, FLOOR_DB), CAP_DB), noise))
        stages.append(lu)
    ref.setflags(write=False); est.setflags(write=False)
    return ref, est, stages, bars


def run_sdr(ref, est, K, lengths=None, pad=64):
    """cruse_sdr through ops with out, dbg and the workspace between `pad` sentinels on both sides -> (scores, dbg [B, 3 K + 2])"""
    from cruse_amd import ops
    B, L = ref.shape
    n = ops.sdr_workspace(B, L, K, "cuda").numel()
    sent = 12345.678
    wsbuf = torch.full((n + 2 * pad,), sent, device="cuda", dtype=torch.float64)
    dbgbuf = torch.full((B * (3 * K + 2) + 2 * pad,), sent, device="cuda", dtype=torch.float64)
    outbuf = torch.full((B + 2 * pad,), sent, device="cuda", dtype=torch.float32)
    ws, dbg, out = wsbuf[pad:pad + n], dbgbuf[pad:pad + B * (3 * K + 2)], outbuf[pad:pad + B]
    ops.sdr(torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda"), ws, K, out=out, lengths=lengths, dbg=dbg)
    torch.cuda.synchronize()
    for buf, m in ((wsbuf, n), (dbgbuf, B * (3 * K + 2)), (outbuf, B)):
        assert bool((buf[:pad] == sent).all()) and bool((buf[pad + m:] == sent).all()), "a sentinel beside the buffer was overwritten"
    return out.cpu().numpy().copy(), dbg.cpu().numpy().reshape(B, 3 * K + 2).copy()


def check_clip(tag, got_score, g, st, bar, K):
    """one clip's dbg row g and score against the restatement's stages st"""
    bar_rel, bar_db, noise = bar
    d = {"raa": S.rel(g[:K], st["raa"]), "rab": S.rel(g[K:2 * K], st["rab"]), "C": S.rel(g[2 * K:3 * K], st["C"]),
         "ss": S.rel(g[3 * K], st["ss"])}
    ss, ee = g[3 * K], g[3 * K + 1]
    print(f"{tag}: raa {d['raa']:.2e}  rab {d['rab']:.2e}  C {d['C']:.2e}  s_target energy {d['ss']:.2e} (bar {bar_rel:.1e})  "
          f"f32 score {float(got_score):.7f} dB, float64 restatement {st['score']:.9f} dB")
    assert d["raa"] <= CAP_REL and d["rab"] <= CAP_REL and d["C"] <= CAP_REL, (tag, d)
    assert d["ss"] <= bar_rel, (tag, d["ss"], bar_rel)
    if noise:
        assert ee <= NOISE_EE * ss and float(got_score) >= 240.0, (tag, ss, ee, got_score)
    else:
        assert S.rel(ee, st["ee"]) <= CAP_REL
        # out is f32 (an ulp at 20 dB is 1.9e-6 dB, far above the bar): it must be the rounding of the log of the two f64 energies, up to
        # one f32 ulp for a log10 that differs in its last f64 bit; the bar is asserted on that f64 value
        s64 = 10.0 * np.log10(ss / ee)
        assert abs(float(got_score) - s64) <= float(np.spacing(np.float32(abs(s64)))), (tag, got_score, s64)
        d64 = abs(s64 - st["score"])
        print(f"{tag}: f64 score from the device's energies {s64:.12f} dB  |d| {d64:.2e} (bar {bar_db:.1e})")
        assert d64 <= bar_db, (tag, d64, bar_db)


@pytest.mark.parametrize("L,K", [(700, 8), (1500, 33), (4000, 512), (300, 512), (1, 4), ("chunk", 16), ("chunk+1", 16)])
def test_stages_and_score_against_float64(L, K):
    L = {"chunk": _chunk(), "chunk+1": _chunk() + 1}.get(L, L)
    assert (L, K) in case_shapes()
    ref, est, stages, bars = case(L, K)
    score, dbg = run_sdr(ref, est, K)
    for b in range(ref.shape[0]):
        check_clip(f"({L}, {K})[{b}]", score[b], dbg[b], stages[b], bars[b], K)


RAGGED_L, RAGGED_K, RAGGED_LEN = 4000, 512, (4000, 1237, 0, 511)


def test_a_clip_scores_the_same_in_a_ragged_batch_and_alone():
    """the padding is NaN in ref and est: a kernel that loaded one sample of it would not give a finite score"""
    from cruse_amd import metrics
    ref = np.stack([S.speechlike(RAGGED_L, 40 + 2 * b) for b in range(4)])
    est = np.stack([S.distort(ref[b], 41 + 2 * b) for b in range(4)])
    want = [S.sdr_stages(ref[b], est[b], RAGGED_K, length=n) for b, n in enumerate(RAGGED_LEN)]
    for b, n in enumerate(RAGGED_LEN):
        ref[b, n:] = np.nan
        est[b, n:] = np.nan
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    for how in ("device", "host"):
        lengths = torch.tensor(RAGGED_LEN, device="cuda", dtype=torch.int32) if how == "device" else list(RAGGED_LEN)
        got = metrics.sdr(r, e, filter_len=RAGGED_K, lengths=lengths)
        print(f"sdr ({how} lengths): {got.tolist()}  float64 {[w['score'] for w in want]}")
        for b, n in enumerate(RAGGED_LEN):
            if n == 0:
                assert bool(torch.isnan(got[b]))
                continue
            alone = metrics.sdr(r[b:b + 1, :n].contiguous(), e[b:b + 1, :n].contiguous(), filter_len=RAGGED_K)
            assert bool(torch.isfinite(got[b])) and torch.equal(got[b:b + 1], alone), (b, got[b], alone)
            assert abs(float(got[b]) - want[b]["score"]) <= 2e-6        # f32 rounding of ~20 dB: half an ulp is 9.5e-7
    one = metrics.sdr(r[1], e[1], filter_len=RAGGED_K, lengths=RAGGED_LEN[1])
    assert one.dim() == 0 and torch.equal(one, got[1])
    # the stages of the ragged call against the restatement of the cut clips, and lengths outside [0, L] clamped by the kernels
    score, dbg = run_sdr(np.nan_to_num(ref, nan=0.25), np.nan_to_num(est, nan=-0.5), RAGGED_K,
                         lengths=torch.tensor((4000 + 9, 1237, -4, 511), device="cuda", dtype=torch.int32))
    assert np.array_equal(score[[0, 1, 3]], got.cpu().numpy()[[0, 1, 3]]) and np.isnan(score[2])
    for b in (1, 3):
        assert S.rel(dbg[b, 2 * RAGGED_K:3 * RAGGED_K], want[b]["C"]) <= CAP_REL and S.rel(dbg[b, 3 * RAGGED_K], want[b]["ss"]) <= CAP_REL
    assert np.isnan(dbg[2, 2 * RAGGED_K:]).all() and (dbg[2, :2 * RAGGED_K] == 0.0).all()


def test_degenerate_clips_score_nan_and_the_process_goes_on():
    from cruse_amd import metrics
    ref, est, stages, _ = case(700, 8)
    r, e = torch.tensor(ref, device="cuda").clone(), torch.tensor(est, device="cuda")
    r[0].zero_()                                                         # an all-zero reference beside a healthy clip
    got = metrics.sdr(r, e, filter_len=8)
    assert bool(torch.isnan(got[0])) and abs(float(got[1]) - stages[1]["score"]) <= 2e-6
    z = torch.zeros_like(e)
    assert bool(torch.isnan(metrics.sdr(z, z, filter_len=8)).all())
    assert bool(torch.isnan(metrics.sdr(torch.tensor(ref, device="cuda"), z, filter_len=8)).all())      # C = 0: 0 / 0
    again = metrics.sdr(torch.tensor(ref, device="cuda"), e, filter_len=8)
    assert bool(torch.isfinite(again).all()) and abs(float(again[0]) - stages[0]["score"]) <= 2e-6
    assert metrics.REGISTERED_METRICS["SDR"] is metrics.sdr and metrics.SDR is metrics.sdr


def test_two_calls_and_a_graph_replay_are_bit_identical():
    from cruse_amd import metrics
    ref, est, _, _ = case(4000, 512)
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    first = metrics.sdr(r, e).clone()                                    # (builds the workspace) filter_len = 512 by default
    second = metrics.sdr(r, e).clone()
    assert torch.equal(first, second) and bool(torch.isfinite(first).all())
    assert torch.equal(first, metrics.sdr(r, e, filter_len=512, lengths=[4000, 4000]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.sdr(r, e)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)


def test_tail_placement_gives_the_same_bits():
    """every operand is the tail of its own buffer (its last element is the buffer's last, its base off the 16-byte grid)"""
    from cruse_amd import ops
    K = 33
    ref, est, _, _ = case(1500, K)
    B, L = ref.shape

    def tail(t, extra):
        buf = torch.full((t.numel() + extra,), float("nan"), device="cuda", dtype=t.dtype)
        v = buf[extra:].view(t.shape)
        v.copy_(t)
        return v

    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    ws = ops.sdr_workspace(B, L, K, "cuda")
    want = ops.sdr(r, e, ws, K).clone()
    out = tail(torch.zeros(B, device="cuda"), 3)
    ops.sdr(tail(r, 3), tail(e, 1), tail(torch.zeros_like(ws), 1), K, out=out, dbg=tail(torch.zeros(B, 3 * K + 2, device="cuda", dtype=torch.float64), 1))
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_refusals_through_the_c_entry_point():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    B, L, K = 2, 700, 8
    ref, est, _, _ = case(L, K)
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    ws = ops.sdr_workspace(B, L, K, "cuda")
    out = torch.full((B,), 7.0, device="cuda")
    P = lambda t: t.data_ptr()      # noqa: E731
    bad = [lib.cruse_sdr(None, P(e), None, B, L, K, P(ws), P(out), None, None), lib.cruse_sdr(P(r), None, None, B, L, K, P(ws), P(out), None, None),
           lib.cruse_sdr(P(r), P(e), None, B, L, K, None, P(out), None, None), lib.cruse_sdr(P(r), P(e), None, B, L, K, P(ws), None, None, None),
           lib.cruse_sdr(P(r), P(e), None, 0, L, K, P(ws), P(out), None, None), lib.cruse_sdr(P(r), P(e), None, B, 0, K, P(ws), P(out), None, None),
           lib.cruse_sdr(P(r), P(e), None, B, L, 0, P(ws), P(out), None, None), lib.cruse_sdr(P(r), P(e), None, B, L, 1025, P(ws), P(out), None, None)]
    assert bad == [-1] * len(bad), bad
    with pytest.raises(RuntimeError, match="workspace"):
        ops.sdr(r, e, ws[:-1], K, out=out)
    with pytest.raises(RuntimeError, match="lengths"):
        ops.sdr(r, e, ws, K, out=out, lengths=torch.tensor([L, L], device="cuda"))
    with pytest.raises(RuntimeError):
        ops.sdr_workspace(B, L, 1025, "cuda")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # refused before any launch
    assert lib.cruse_sdr(P(r), P(e), None, B, L, K, P(ws), P(out), None, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def test_trainer_scores_validation_by_enhanced_sdr(tmp_path, capsys):
    import train_base.loss as TL
    from torch.utils.data import DataLoader
    from cruse_amd import metrics
    from cruse_amd.data import SyntheticPairs
    from cruse_amd.inferencer import Inferencer
    from cruse_amd.model.cruse_net import unet_2
    from cruse_amd.train.trainer_casual import Trainer
    torch.manual_seed(0)
    m = unet_2(ch=(1, 4, 8, 16, 32), rnn_groups=2)
    cfg = {"acoustics": {"n_fft": 320, "hop_length": 160, "win_length": 320, "sr": 16000},
           "trainer": {"train": {"epochs": 1},
                       "validation": {"metrics": ["SI_SDR", "SDR"], "score_metric": "SDR", "save_max_metric_score": True}},
           "meta": {"save_dir": str(tmp_path), "experiment_name": "by_sdr", "precision": "f32", "hip_graph": False}}
    loader = DataLoader(SyntheticPairs(num=4, length=16000, seed=2), batch_size=2, shuffle=False, num_workers=0)
    tr = Trainer(dist=None, rank=0, config=cfg, resume=False, only_validation=True, model=m, loss_function=TL.wo_male_loss(),
                 optimizer=torch.optim.Adam(m.parameters(), lr=1e-3), train_dataloader=None, validation_dataloader=loader)
    assert tr.metric_names == ("SI_SDR", "SDR") and tr.score_metric == "SDR"
    tr.model.eval()
    score = tr._validation_epoch(1)
    out = capsys.readouterr().out
    print(out)
    assert "validation SI_SDR: Noisy" in out and "validation SDR: Noisy" in out and "Enhanced" in out
    inf = Inferencer(tr.model)
    per = {"noisy": [], "enh": []}
    for noisy, clean in loader:
        noisy, clean = noisy.cuda().float(), clean.cuda().float()
        per["enh"] += metrics.sdr(clean, inf.mag_mask_to_wave(noisy)).tolist()
        per["noisy"] += metrics.sdr(clean, noisy).tolist()
    assert len(per["enh"]) == 4 and bool(np.isfinite(per["enh"] + per["noisy"]).all())
    assert abs(score - float(np.mean(per["enh"]))) <= 1e-5
    assert abs(tr.last_metric_means["SDR"]["Noisy"] - float(np.mean(per["noisy"]))) <= 1e-5
    # SDR allows a 512-tap filtering of the reference that SI-SDR counts as error: it is never below SI-SDR (up to f32 rounding)
    assert tr.last_metric_means["SDR"]["Noisy"] >= tr.last_metric_means["SI_SDR"]["Noisy"] - 1e-4
    tr.train()                                                           # only_validation: one epoch, scored, best checkpoint written
    out = capsys.readouterr().out
    assert "validation score (SDR, enhanced)" in out
    ck = torch.load(tmp_path / "by_sdr" / "checkpoints" / "best_model.tar", map_location="cpu", weights_only=False)
    assert abs(ck["best_score"] - score) <= 1e-9
