"""GPU: cruse_amd.evaluate.evaluate_files and tools/evaluate.py on five pairs of WAV files of different lengths and rates, against the
composition by hand of the pieces it joins (ops.resample_poly per file, zero padding, Inferencer.mag_mask_to_wave, the metrics with
lengths=).  Everything is compared bit for bit: the pieces are deterministic and a clip scores the same alone and in a batch."""
import csv
import functools
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from tests import stoi_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
METRICS = ("SI_SDR", "STOI", "ESTOI")
# (name, rate, channels, frames): 16037, 6554, 9000, 6553 and 12000 samples at 16 kHz, in an order that is not the order of lengths
FILES = [("p0", 16000, 1, 16037), ("p1", 8000, 1, 3277), ("p2", 48000, 2, 27000), ("p3", 16000, 1, 6553), ("p4", 16000, 1, 12000)]
LENGTHS = [16037, 6554, 9000, 6553, 12000]


def _write(path, x, channels, rate, other):
    pcm = np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2")
    if channels == 2:                                                    # channel 1 holds something else: channel 0 is what is read
        pcm = np.stack([pcm, np.round(np.clip(other, -1.0, 1.0) * 32767.0).astype("<i2")], axis=1).reshape(-1)
    with wave.open(path, "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


_ENV = []


@pytest.fixture(scope="module", autouse=True)
def _env(tmp_path_factory):
    _ENV.append(str(tmp_path_factory.mktemp("evaluate")))
    yield
    for f in (setup, alone, result):
        f.cache_clear()
    _ENV.clear()


@functools.lru_cache(maxsize=None)
def setup():
    """the files (in pytest's temporary directory), the two list files, the seeded model and its checkpoint -- made once, shared"""
    from cruse_amd.model.cruse_net import unet_2
    d = _ENV[0]
    clean, noisy = [], []
    for k, (name, rate, ch, frames) in enumerate(FILES):
        x = R.speechlike(frames, 60 + k, (frames // 4, frames // 3) if LENGTHS[k] >= 9000 else None)   # the short clips keep all frames
        y = R.add_noise(x, 5.0, 70 + k)
        os.makedirs(os.path.join(d, "clean"), exist_ok=True)
        os.makedirs(os.path.join(d, "noisy"), exist_ok=True)
        clean.append(os.path.join(d, "clean", name + ".wav"))
        noisy.append(os.path.join(d, "noisy", name + ".wav"))
        _write(clean[-1], x, ch, rate, -y)
        _write(noisy[-1], y, ch, rate, x[::-1])
    lists = [os.path.join(d, "clean.txt"), os.path.join(d, "noisy.txt")]
    for path, names in zip(lists, (clean, noisy)):
        with open(path, "w") as f:
            f.write("\n".join(names) + "\n")
    torch.manual_seed(0)
    model = unet_2()
    ck = os.path.join(d, "model.tar")
    torch.save({"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}}, ck)
    return d, clean, noisy, lists, model.cuda(), ck


@functools.lru_cache(maxsize=None)
def alone():
    """every file converted on its own by one ops.resample_poly call -> ([clean 16 kHz clip], [noisy 16 kHz clip]) on the device"""
    from cruse_amd import ops, wavio
    from cruse_amd import resample_design as D
    _, clean, noisy, _, _, _ = setup()
    out = ([], [])
    for side, paths in enumerate((clean, noisy)):
        for p in paths:
            pcm, ch, rate = wavio.read_pcm16(p)
            up, down = D.ratio(16000, rate)
            n = D.out_len(pcm.shape[0] // ch, up, down)
            y = torch.empty(n, device="cuda", dtype=torch.float32)
            ops.resample_poly(torch.from_numpy(pcm.copy()).cuda(), [0, pcm.shape[0] // ch], [0, n], up, down, y, channels=ch, channel=0)
            out[side].append(y)
    return out


@functools.lru_cache(maxsize=None)
def result(batch_size):
    from cruse_amd.evaluate import evaluate_files
    _, _, _, lists, model, _ = setup()
    return evaluate_files(model, lists[0], lists[1], metrics=METRICS, batch_size=batch_size)


def _padded(clips, idx, L):
    x = torch.zeros(len(idx), L, device="cuda", dtype=torch.float32)
    for row, i in enumerate(idx):
        x[row, :clips[i].shape[0]] = clips[i]
    return x


def test_batches_of_two_equal_the_composition_by_hand():
    from cruse_amd import metrics
    from cruse_amd.filepairs import load_pool
    from cruse_amd.inferencer import Inferencer
    _, clean, noisy, _, model, _ = setup()
    res = result(2)
    assert res["names"] == [name + ".wav" for name, _, _, _ in FILES] and res["lengths"].tolist() == LENGTHS        # list order
    assert sorted(res["scores"]) == sorted(METRICS) and sorted(res["mean"]) == sorted(METRICS)
    c16, n16 = alone()
    assert [c.shape[0] for c in c16] == LENGTHS
    # the 8 kHz and the 48 kHz stereo file inside the shared pool are what the resampler gives for them alone
    pool, start, lens, _ = load_pool(clean + noisy, "cuda")
    for i in (1, 2):
        assert torch.equal(pool[start[i]:start[i] + lens[i]], c16[i]) and torch.equal(pool[start[5 + i]:start[5 + i] + lens[5 + i]], n16[i])
    inf = Inferencer(model)
    order = np.argsort(np.asarray(LENGTHS), kind="stable")
    assert order.tolist() == [3, 1, 2, 4, 0]
    for k in range(0, 5, 2):
        idx = order[k:k + 2].tolist()
        L = max(LENGTHS[i] for i in idx)
        c, x = _padded(c16, idx, L), _padded(n16, idx, L)
        ln = torch.tensor([LENGTHS[i] for i in idx], device="cuda", dtype=torch.int32)
        y = inf.mag_mask_to_wave(x)
        for m in METRICS:
            fn = metrics.REGISTERED_METRICS[m]
            for side, est in (("Noisy", x), ("Enhanced", y)):
                want = fn(c, est, lengths=ln).cpu()
                got = torch.from_numpy(res["scores"][m][side][idx])
                print(f"batch {idx} {m} {side}: {got.tolist()} vs by hand {want.tolist()}")
                assert torch.equal(got, want), (idx, m, side, got, want)
    for m in METRICS:
        for side in ("Noisy", "Enhanced"):
            s = res["scores"][m][side]
            assert s.shape == (5,) and np.isfinite(s).all() and res["mean"][m][side] == float(s.astype(np.float64).mean())
    assert (res["scores"]["STOI"]["Noisy"][[0, 2, 4]] > 0.1).all()         # real scores, not the too-short value


def test_noisy_scores_do_not_depend_on_the_batching():
    a, b = result(2), result(5)
    assert a["names"] == b["names"] and a["lengths"].tolist() == b["lengths"].tolist()
    for m in METRICS:
        assert np.array_equal(a["scores"][m]["Noisy"], b["scores"][m]["Noisy"]), m


def test_batch_size_one_is_every_clip_alone():
    from cruse_amd import metrics
    from cruse_amd.inferencer import Inferencer
    _, _, _, _, model, _ = setup()
    res = result(1)
    c16, n16 = alone()
    inf = Inferencer(model)
    for i in range(5):
        c, x = c16[i].reshape(1, -1), n16[i].reshape(1, -1)
        y = inf.mag_mask_to_wave(x)
        for m in METRICS:
            fn = metrics.REGISTERED_METRICS[m]                           # un-keyworded: the call of a rectangular batch
            assert float(fn(c, y)[0]) == float(res["scores"][m]["Enhanced"][i]), (i, m)
            assert float(fn(c, x)[0]) == float(res["scores"][m]["Noisy"][i]), (i, m)
    for m in METRICS:
        assert np.array_equal(res["scores"][m]["Noisy"], result(2)["scores"][m]["Noisy"]), m


def test_the_command_line_tool_in_a_fresh_process():
    d, _, _, lists, _, ck = setup()
    cfg = os.path.join(d, "eval.toml")
    with open(cfg, "w") as f:
        f.write('[acoustics]\nn_fft = 320\nhop_length = 160\nwin_length = 320\nsr = 16000\n\n'
                '[model]\npath = "model.cruse_net.unet_2"\n[model.args]\nin_feat = 161\n')
    out_csv = os.path.join(d, "scores.csv")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--config", cfg, "--checkpoint", ck, "--clean-list", lists[0],
                          "--noisy-list", lists[1], "--batch-size", "2", "--metrics", *METRICS, "--csv", out_csv],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    res = result(2)
    lines = {ln.split(":")[0]: ln.split() for ln in run.stdout.splitlines() if ln.split(":")[0] in METRICS}
    assert sorted(lines) == sorted(METRICS), run.stdout
    for m in METRICS:                                                    # "NAME: Noisy <repr> Enhanced <repr>"
        assert lines[m][1] == "Noisy" and lines[m][3] == "Enhanced"
        assert float(lines[m][2]) == res["mean"][m]["Noisy"] and float(lines[m][4]) == res["mean"][m]["Enhanced"], (m, lines[m])
    rows = list(csv.reader(open(out_csv)))
    assert rows[0] == ["name", "length"] + [f"{m}_{s}" for m in METRICS for s in ("Noisy", "Enhanced")]
    assert len(rows) == 6 and [r[0] for r in rows[1:]] == res["names"] and [int(r[1]) for r in rows[1:]] == LENGTHS
    assert [float(r[2]) for r in rows[1:]] == [float(v) for v in res["scores"]["SI_SDR"]["Noisy"]]
