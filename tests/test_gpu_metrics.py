"""GPU: cruse_si_sdr / cruse_stoi (csrc/metrics.hip) against the float64 restatement of DESIGN section 13 (tests/stoi_ref.py), stage by
stage through cruse_stoi_layout; determinism, graph capture, bounds; the trainer's metric-scored validation.

Bars.  x10 and tob: the project's stage bar, 1e-5 rel-L2.  Kept-frame lists: equal.  Score: 5e-6 absolute, about 40 x the f32
restatement's own distance from float64 (<= 1.3e-7), the ratio of the project's 2e-5 bars to its 4e-7 measurements.  Every STOI case
first asserts, on the CPU, that no frame energy of the float64 restatement lies within 0.5 dB of the 40 dB threshold (so an f32
evaluation cannot legitimately keep another set of frames) and that the f32 restatement scores within 1e-6 of the float64 one.
Measured on the MI355X: x10 and tob 1.3e-7 ... 1.4e-7 rel-L2, scores within 2.2e-8, SI-SDR equal to 5 decimals."""
import functools

import numpy as np
import pytest
import torch

from tests import stoi_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

STAGE_BAR, SCORE_BAR, SISDR_BAR_DB = 1e-5, 5e-6, 1e-4

# name -> (L, [(seed, gap, snr_db, noise seed)] per clip)
CASES = {
    "short_29": (6400, [(10, None, 5.0, 100)]),                                    # nF = 30, all kept: nG = 29, no segment
    "one_segment": (6553, [(10, None, 5.0, 100)]),                                 # the shortest gap-free L with nG = 30
    "ragged_kept": (16037, [(10, (2000, 7000), 20.0, 100), (11, (9000, 13000), -5.0, 101), (12, (3000, 13500), 5.0, 102)]),
    "two_seconds": (32000, [(10, (8000, 20000), 5.0, 100), (11, (1000, 16000), -5.0, 101)]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(ref [B, L] f32, est [B, L] f32, float64 stages per clip) -- computed once, shared, read-only; asserts the CPU conditions"""
    L, clips = CASES[name]
    ref = np.stack([R.speechlike(L, seed, gap) for seed, gap, _, _ in clips])
    est = np.stack([R.add_noise(ref[i], snr, ns) for i, (_, _, snr, ns) in enumerate(clips)])
    stages = [R.stoi_stages(ref[i], est[i]) for i in range(len(clips))]
    for i, st in enumerate(stages):
        assert R.threshold_margin(st["e"]) >= 0.5, (name, i, R.threshold_margin(st["e"]))
        f32 = R.stoi_stages(ref[i], est[i], np.float32)
        assert np.array_equal(f32["kept"], st["kept"]) and abs(f32["score"] - st["score"]) <= 1e-6, (name, i)
    ref.setflags(write=False); est.setflags(write=False)
    return ref, est, stages


def run_stoi(ref, est, pad=64):
    """cruse_stoi through ops with `out` and the workspace between `pad` sentinel floats on both sides -> (scores, layout, ws view)"""
    from cruse_amd import ops
    B, L = ref.shape
    Y = ops.stoi_layout(B, L)
    sent = 12345.678
    wsbuf = torch.full((Y["total"] + 2 * pad,), sent, device="cuda", dtype=torch.float32)
    outbuf = torch.full((B + 2 * pad,), sent, device="cuda", dtype=torch.float32)
    ws, out = wsbuf[pad:pad + Y["total"]], outbuf[pad:pad + B]
    ops.stoi(torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda"), ops.stoi_tables("cuda"), ws, out=out)
    torch.cuda.synchronize()
    for buf, n in ((wsbuf, Y["total"]), (outbuf, B)):
        assert bool((buf[:pad] == sent).all()) and bool((buf[pad + n:] == sent).all()), "a sentinel beside the buffer was overwritten"
    return out.cpu().numpy().copy(), Y, ws.cpu()


def stages_of(ws, Y, B, b):
    """clip b's stages out of a workspace copy, through the layout"""
    f, i = ws.numpy(), ws.view(torch.int32).numpy()
    nFa = max(Y["nF"], 1)
    nk = int(i[Y["nk"] + b])
    nG = max(nk - 1, 0)
    x10 = f[Y["x10"] + b * 2 * Y["L10"]:Y["x10"] + (b + 1) * 2 * Y["L10"]].reshape(2, Y["L10"])
    e = f[Y["e"] + b * nFa:Y["e"] + b * nFa + Y["nF"]]
    kept = i[Y["kept"] + b * nFa:Y["kept"] + b * nFa + nk]
    tob = f[Y["tob"] + b * 30 * Y["nGs"]:Y["tob"] + (b + 1) * 30 * Y["nGs"]].reshape(2, 15, Y["nGs"])[:, :, :nG]
    return {"x10": x10, "e": e, "kept": kept, "tob": tob}


@pytest.mark.parametrize("name", list(CASES))
def test_stoi_stages_and_score_against_float64(name):
    ref, est, want = case(name)
    B = ref.shape[0]
    got, Y, ws = run_stoi(ref, est)
    for b in range(B):
        st, w = stages_of(ws, Y, B, b), want[b]
        ex10 = rel_l2(torch.from_numpy(st["x10"]), torch.from_numpy(w["x10"]))
        assert np.array_equal(st["kept"], w["kept"]), (name, b)
        nG = len(w["kept"]) - 1
        etob = rel_l2(torch.from_numpy(st["tob"]), torch.from_numpy(w["tob"])) if nG >= 1 else 0.0
        ee = float(np.abs(st["e"] - w["e"]).max())
        print(f"{name}[{b}]: kept {len(w['kept'])}/{Y['nF']}  x10 rel-L2 {ex10:.2e}  e max|d| {ee:.2e} dB  tob rel-L2 {etob:.2e}  "
              f"score {got[b]:.7f} vs {w['score']:.7f}  |d| {abs(float(got[b]) - w['score']):.2e}")
        assert ex10 <= STAGE_BAR and etob <= STAGE_BAR, (name, b, ex10, etob)
        assert ee <= 1e-3, (name, b, ee)                                 # 0.5 dB of margin asserted above
        assert abs(float(got[b]) - w["score"]) <= SCORE_BAR, (name, b, got[b], w["score"])
    if name == "short_29":
        assert len(want[0]["kept"]) == 30 and got[0] == np.float32(1e-5)
    if name == "one_segment":
        assert len(want[0]["kept"]) == 31 and want[0]["score"] > 0.5
    if name == "ragged_kept":
        nk = [len(w["kept"]) for w in want]
        assert len(set(nk)) == 3 and nk[2] < 30 and got[2] == np.float32(1e-5), nk


@pytest.mark.parametrize("name", ["ragged_kept", "two_seconds"])
def test_a_clip_scores_the_same_alone_and_in_a_batch(name):
    from cruse_amd import metrics
    ref, est, _ = case(name)
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    batch = metrics.stoi(r, e).cpu()
    sd = metrics.si_sdr(r, e).cpu()
    for b in range(ref.shape[0]):
        assert torch.equal(metrics.stoi(r[b], e[b]).cpu(), batch[b])
        assert torch.equal(metrics.si_sdr(r[b:b + 1], e[b:b + 1]).cpu()[0], sd[b])


def test_stoi_of_all_zero_clips_is_finite_and_matches():
    ref, _, _ = case("two_seconds")
    x = ref[:1]
    z = np.zeros_like(x)
    for r, e in ((z, x), (x, z)):
        want = R.stoi(r[0], e[0])
        got, _, _ = run_stoi(r, e)
        assert np.isfinite(got[0]) and abs(float(got[0]) - want) <= SCORE_BAR, (got, want)


def test_si_sdr_against_float64():
    from cruse_amd import metrics
    rng = np.random.default_rng(5)
    # L = 1 with est = ref / 2 on powers of two: alpha = 1/2 and the residual 0 exactly, +inf in numpy and here
    ref1 = np.array([[1.0], [2.0], [-4.0]], dtype=np.float32)
    got1 = metrics.si_sdr(torch.from_numpy(ref1).cuda(), torch.from_numpy(0.5 * ref1).cuda()).cpu().numpy()
    with np.errstate(divide="ignore"):
        assert all(R.si_sdr(ref1[b], 0.5 * ref1[b]) == np.inf and got1[b] == np.inf for b in range(3)), got1
    L = 16037
    ref = np.stack([R.speechlike(L, 20 + i) for i in range(3)])
    ests = [np.stack([R.add_noise(ref[i], snr, 30 + i) for i in range(3)]) for snr in (20.0, -5.0)]
    ests.append((2.0 * ref + 0.1 * rng.standard_normal(ref.shape)).astype(np.float32))
    for est in ests:
        got = metrics.si_sdr(torch.from_numpy(ref).cuda(), torch.from_numpy(est).cuda()).cpu().numpy()
        for b in range(3):
            want = R.si_sdr(ref[b], est[b])
            print(f"si_sdr L={L} [{b}]: {got[b]:.5f} vs {want:.5f} dB")
            assert abs(float(got[b]) - want) <= SISDR_BAR_DB, (L, b, got[b], want)
    # scale invariance: est = 2 (ref + n) scores what est = ref + n scores
    x = R.speechlike(8000, 3)
    n = (0.05 * rng.standard_normal(8000)).astype(np.float32)
    a = metrics.si_sdr(torch.from_numpy(x).cuda(), torch.from_numpy(2 * x + 2 * n).cuda())
    b = metrics.si_sdr(torch.from_numpy(x).cuda(), torch.from_numpy(x + n).cuda())
    assert a.dim() == 0 and abs(float(a) - float(b)) <= SISDR_BAR_DB


def test_two_calls_and_a_graph_replay_are_bit_identical():
    """no atomics: two calls agree in every bit; no host synchronisation: the call captures into a graph, whose replay agrees too"""
    from cruse_amd import metrics
    ref, est, _ = case("ragged_kept")
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    a = metrics.stoi(r, e).clone()                                       # (the first call builds the tables and the workspace)
    b = metrics.stoi(r, e).clone()
    s1, s2 = metrics.si_sdr(r, e).clone(), metrics.si_sdr(r, e).clone()
    assert torch.equal(a, b) and torch.equal(s1, s2)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.stoi(r, e)
        out_sd = metrics.si_sdr(r, e)
    out.zero_(); out_sd.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a) and torch.equal(out_sd, s1)


def test_refusals_through_the_c_entry_points():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    ref, est, _ = case("short_29")
    r, e = torch.tensor(ref, device="cuda"), torch.tensor(est, device="cuda")
    B, L = r.shape
    tab, ws, out = ops.stoi_tables("cuda"), ops.stoi_workspace(B, L, "cuda"), torch.full((B,), 7.0, device="cuda")
    n = ws.numel() * 4
    assert n == lib.cruse_stoi_ws_bytes(B, L)
    P = lambda t: t.data_ptr()                                          # noqa: E731
    bad = [lib.cruse_stoi(None, P(e), B, L, P(tab), P(ws), n, P(out), None), lib.cruse_stoi(P(r), None, B, L, P(tab), P(ws), n, P(out), None),
           lib.cruse_stoi(P(r), P(e), B, L, None, P(ws), n, P(out), None), lib.cruse_stoi(P(r), P(e), B, L, P(tab), None, n, P(out), None),
           lib.cruse_stoi(P(r), P(e), B, L, P(tab), P(ws), n, None, None), lib.cruse_stoi(P(r), P(e), 0, L, P(tab), P(ws), n, P(out), None),
           lib.cruse_stoi(P(r), P(e), B, 0, P(tab), P(ws), n, P(out), None),
           lib.cruse_stoi(P(r), P(e), B, (1 << 28) + 1, P(tab), P(ws), n, P(out), None),
           lib.cruse_stoi(P(r), P(e), B, L, P(tab), P(ws), n - 4, P(out), None),
           lib.cruse_si_sdr(None, P(e), B, L, P(out), None), lib.cruse_si_sdr(P(r), P(e), B, 0, P(out), None),
           lib.cruse_si_sdr(P(r), P(e), 0, L, P(out), None), lib.cruse_si_sdr(P(r), P(e), B, L, None, None)]
    assert bad == [-1] * len(bad), bad
    with pytest.raises(RuntimeError, match="workspace"):
        ops.stoi(r, e, tab, ws[:-1])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                      # refused before any launch
    assert lib.cruse_stoi(P(r), P(e), B, L, P(tab), P(ws), n, P(out), None) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == float(np.float32(1e-5))


# ---- trainer -------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, validation, name):
    import train_base.loss as L
    from torch.utils.data import DataLoader
    from cruse_amd.data import SyntheticPairs
    from cruse_amd.model.cruse_net import unet_2
    from cruse_amd.train.trainer_casual import Trainer
    torch.manual_seed(0)
    m = unet_2(ch=(1, 4, 8, 16, 32), rnn_groups=2)
    cfg = {"acoustics": {"n_fft": 320, "hop_length": 160, "win_length": 320, "sr": 16000},
           "trainer": {"train": {"epochs": 1}, "validation": validation},
           "meta": {"save_dir": str(tmp_path), "experiment_name": name, "precision": "f32", "hip_graph": False}}
    loader = DataLoader(SyntheticPairs(num=4, length=16000, seed=2), batch_size=2, shuffle=False, num_workers=0)
    tr = Trainer(dist=None, rank=0, config=cfg, resume=False, only_validation=True, model=m, loss_function=L.wo_male_loss(),
                 optimizer=torch.optim.Adam(m.parameters(), lr=1e-3), train_dataloader=None, validation_dataloader=loader)
    return tr, loader


def test_trainer_scores_validation_by_enhanced_stoi(tmp_path, capsys):
    from cruse_amd import metrics
    from cruse_amd.inferencer import Inferencer
    tr, loader = _trainer(tmp_path, {"metrics": ["SI_SDR", "STOI"], "score_metric": "STOI", "save_max_metric_score": True},
                         "with_metrics")
    assert tr.metric_names == ("SI_SDR", "STOI") and tr.score_metric == "STOI"
    tr.model.eval()
    score = tr._validation_epoch(1)
    out = capsys.readouterr().out
    assert "validation SI_SDR: Noisy" in out and "validation STOI: Noisy" in out and "Enhanced" in out
    inf = Inferencer(tr.model)
    per = {"noisy": [], "enh": [], "sd": []}
    for noisy, clean in loader:
        noisy, clean = noisy.cuda().float(), clean.cuda().float()
        enh = inf.mag_mask_to_wave(noisy)
        per["enh"] += metrics.stoi(clean, enh).tolist()
        per["noisy"] += metrics.stoi(clean, noisy).tolist()
        per["sd"] += metrics.si_sdr(clean, enh).tolist()
    assert len(per["enh"]) == 4 and min(per["noisy"]) > 1e-4            # real scores, not the too-short value
    assert abs(score - float(np.mean(per["enh"]))) <= 1e-6
    assert abs(tr.last_metric_means["STOI"]["Noisy"] - float(np.mean(per["noisy"]))) <= 1e-6
    assert abs(tr.last_metric_means["SI_SDR"]["Enhanced"] - float(np.mean(per["sd"]))) <= 1e-4
    tr.train()                                                           # only_validation: one epoch, scored, best checkpoint written
    out = capsys.readouterr().out
    assert "validation score (STOI, enhanced)" in out
    ck = torch.load(tmp_path / "with_metrics" / "checkpoints" / "best_model.tar", map_location="cpu", weights_only=False)
    assert abs(ck["best_score"] - score) <= 1e-9
    with pytest.raises(KeyError, match="registered metrics"):
        _trainer(tmp_path, {"metrics": ["STOI", "MOSNET"]}, "bad")


def test_trainer_without_the_metrics_key_returns_the_validation_loss(tmp_path, capsys):
    tr, loader = _trainer(tmp_path, {"save_max_metric_score": False}, "plain")
    assert tr.metric_names == () and tr.score_metric is None
    tr.model.eval()
    capsys.readouterr()
    score = tr._validation_epoch(1)
    assert capsys.readouterr().out == ""                                 # prints nothing of its own, as before
    want = float(np.mean([tr.engine.eval_loss(n.cuda().float().contiguous(), c.cuda().float().contiguous()) for n, c in loader]))
    assert score == pytest.approx(want, rel=1e-6)
    tr.train()
    assert f"[epoch 1] validation loss {score:.6f}" in capsys.readouterr().out
