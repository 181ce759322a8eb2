"""GPU: cruse_screen_clips and cruse_rt60 against their float64 restatement tests/screen_ref.py, on pools whose gaps
and margins are NaN (a load outside an utterance shows as NaN in the output), and DeviceFilePairs.screen on four tiny WAV files.

screen_clips: peak bit-equal, n_clipped / n_windows / n_active exact, rms within 1e-10 relative (float64 tree sums of <= 40 001 terms).

rt60: the noiseless lines exp(-6.908 n / (T sr)) must give the line's own RT60 to 1e-9 relative.  That value is T 3 ln(10) / 6.908, not
T: 60 dB are 3 ln 10 = 6.90776 nepers of amplitude and 6.908 is its rounding, 3.5e-5 away -- the literal constant is kept and the exact
RT60 of the line it makes is asked for.  The line must be long enough that its missing tail does not bend the curve: the lengths
12 000 (T = 0.3) and 30 000 (T = 0.8) put the end 170 dB down; the restatement then reads 6.4e-11 and 7.7e-10 from the float32 samples.
Against the restatement the bar is ten times the largest relative disagreement of the restatement's own sequential and pairwise
summation orders over these inputs: measured 2.0817e-15 (screen_ref.RT60_MEASURED), bar 2.0817e-14 (screen_ref.RT60_BAR), on rt60 and
edc_floor_db; t_peak and the NaN pattern are exact."""
import numpy as np
import pytest
import torch

from tests import screen_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 799, 800, 801, 1600, 1601, 40001)
GAPS = (3, 1, 6, 2, 7, 3, 7, 10)                         # NaN samples in front of each utterance: every alignment of the first sample
MARGIN_SAMPLES = 64


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def poisoned_pool(clips, gaps):
    """clips laid out with NaN gaps in front of each and a NaN margin at both ends -> (pool float32, start, length)"""
    parts, start, pos = [np.full(MARGIN_SAMPLES, np.nan, dtype=np.float32)], [], MARGIN_SAMPLES
    for x, g in zip(clips, gaps):
        parts.append(np.full(g, np.nan, dtype=np.float32))
        pos += g
        start.append(pos)
        parts.append(x)
        pos += x.shape[0]
    parts.append(np.full(MARGIN_SAMPLES, np.nan, dtype=np.float32))
    return np.concatenate(parts), np.asarray(start, dtype=np.int64), np.asarray([x.shape[0] for x in clips], dtype=np.int64)


@pytest.fixture(scope="module")
def clips():
    """(pool, start, length, the restatement's rows): computed once, left unchanged"""
    out = []
    for i, n in enumerate(LENGTHS):
        x = R.speech_like(n, seed=21 + i, level=(0.05, 0.2)[i % 2])
        if n == 800:
            x = np.zeros(n, dtype=np.float32)                                  # all zero
        if n == 1600:
            x = np.where(np.arange(n) % 10 < 5, 1.0, -1.0).astype(np.float32)  # a full-scale square wave: every sample clipped
        if n == 801:
            x[17] = np.float32(0.999)                                          # exactly the threshold: not clipped
        if n == 1601:
            x[17] = np.float32(0.999)
            x[1600] = np.nextafter(np.float32(0.999), np.float32(2.0))         # the next float32: clipped, in the one-sample last window
        out.append(x)
    pool, start, length = poisoned_pool(out, GAPS)
    assert sorted(set(int(s) % 4 for s in start)) == [0, 1, 2, 3]
    for x in out:
        assert R.min_margin(x) >= R.MARGIN
    want = R.screen_clips(pool, start, length)
    assert want[4, 1] == 0 and want[6, 1] == 1 and want[5, 1] == 1600 and want[3, 4] == 0 and 0 < want[7, 5] < 1
    return pool, start, length, want


def check_screen(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got[:, 0], want[:, 0]), (got[:, 0], want[:, 0])      # peak: bit-equal
    for k in (1, 3, 4):
        assert np.array_equal(got[:, k], want[:, k]), (k, got[:, k], want[:, k])
    print("rms relative error", np.abs(got[:, 2] - want[:, 2]) / np.maximum(want[:, 2], 1e-300))
    assert np.all(np.abs(got[:, 2] - want[:, 2]) <= 1e-10 * want[:, 2])
    assert np.array_equal(got[:, 5], want[:, 5], equal_nan=True)               # a quotient of two exact integers


def test_screen_clips_matches_the_restatement(clips):
    from cruse_amd import ops
    pool, start, length, want = clips
    dpool = torch.from_numpy(pool).to(dev())
    got = ops.screen_clips(dpool, start, length)
    again = ops.screen_clips(dpool, torch.from_numpy(start).to(dev()), torch.from_numpy(length).to(dev()))      # device tables as they are
    check_screen(got.cpu().numpy(), want)
    assert got[0].cpu().tolist()[:5] == [0.0, 0.0, 0.0, 0.0, 0.0] and torch.isnan(got[0, 5])                    # the empty utterance
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))         # the same bits from a second call


def test_screen_clips_one_utterance(clips):
    from cruse_amd import ops
    pool, start, length, want = clips
    dpool = torch.from_numpy(pool).to(dev())
    for i in (0, 7):
        got = ops.screen_clips(dpool, start[i:i + 1], length[i:i + 1])
        check_screen(got.cpu().numpy(), want[i:i + 1])
    assert ops.screen_clips(dpool, [], []).shape == (0, 6)


def test_screen_clips_other_parameters(clips):
    from cruse_amd import ops
    pool, start, length, _ = clips
    dpool = torch.from_numpy(pool).to(dev())
    kw = dict(clip_thr=0.5, target_db=-30.0, act_thr=0.5, window=400)
    want = R.screen_clips(pool, start, length, **kw)
    got = ops.screen_clips(dpool, start, length, sr=8000, clip_threshold=0.5, target_dB_FS=-30.0, activity_threshold=0.5)
    assert all(R.min_margin(pool[s:s + n], act_thr=0.5, window=400, target_db=-30.0) >= R.MARGIN for s, n in zip(start, length))
    check_screen(got.cpu().numpy(), want)


def test_screen_clips_in_a_captured_graph(clips):
    from cruse_amd import ops
    pool, start, length, want = clips
    dpool = torch.from_numpy(pool).to(dev())
    plan = ops.ragged_plan(dpool, start, length)
    eager = ops.screen_clips(dpool, plan=plan).clone()
    out = torch.full((len(start), 6), -1.0, device=dev(), dtype=torch.float64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.screen_clips(dpool, plan=plan, out=out)                            # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.screen_clips(dpool, plan=plan, out=out)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int64), eager.view(torch.int64))
    check_screen(out.cpu().numpy(), want)


@pytest.fixture(scope="module")
def responses():
    inputs = R.rt60_inputs()
    pool, start, length = poisoned_pool([h for _, h, _ in inputs], [3 + (5 * i) % 8 for i in range(len(inputs))])
    return inputs, pool, start, length, R.rt60(pool, start, length)


def check_rt60(got, want, inputs):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(got[:, 1], want[:, 1], equal_nan=True)               # t_peak
    for k in (0, 2):
        fin = np.isfinite(want[:, k])
        assert np.array_equal(got[~fin, k], want[~fin, k], equal_nan=True)     # NaN and -inf alike
        rel = np.abs(got[fin, k] - want[fin, k]) / np.maximum(np.abs(want[fin, k]), 1e-300)
        print(("rt60", "", "edc_floor_db")[k], "relative error vs the restatement", rel, "bar", R.RT60_BAR)
        assert np.all(rel <= R.RT60_BAR), (k, rel)
    for i, (name, _, exact) in enumerate(inputs):
        if isinstance(exact, str):
            assert np.isnan(got[i, 0]), name
        elif exact is not None:
            print(name, "vs the exact line", abs(got[i, 0] - exact) / exact)
            assert abs(got[i, 0] - exact) <= 1e-9 * exact, (name, got[i, 0], exact)


def test_rt60_matches_the_restatement(responses):
    from cruse_amd import ops
    inputs, pool, start, length, want = responses
    names = [n for n, _, _ in inputs]
    assert sorted(length.tolist())[:4] == [0, 2, 64, 100] and 8000 in length and 8001 in length and length.max() > 2048
    dpool = torch.from_numpy(pool).to(dev())
    got = ops.rt60(dpool, start, length)
    again = ops.rt60(dpool, start, length)
    g = got.cpu().numpy()
    check_rt60(g, want, inputs)
    assert g[names.index("predelay37"), 1] == 37.0 and g[names.index("peak_last"), 1] == 299.0
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    i = names.index("line_T0.8")                                               # alone: the same bits as in the batch
    one = ops.rt60(dpool, start[i:i + 1], length[i:i + 1])
    assert torch.equal(one.view(torch.int64), got[i:i + 1].view(torch.int64))
    assert ops.rt60(dpool, [], []).shape == (0, 3)
    with pytest.raises(RuntimeError, match="lo_db"):
        ops.rt60(dpool, start, length, lo_db=-25.0, hi_db=-5.0)


def test_rt60_other_range_and_rate(responses):
    from cruse_amd import ops
    inputs, pool, start, length, _ = responses
    want = R.rt60(pool, start, length, sr=8000, lo_db=-5.0, hi_db=-35.0)       # T30
    got = ops.rt60(torch.from_numpy(pool).to(dev()), start, length, sr=8000, lo_db=-5.0, hi_db=-35.0).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[:, 1], want[:, 1], equal_nan=True)
    fin = np.isfinite(want[:, 0])
    assert fin.sum() >= 6 and np.all(np.abs(got[fin, 0] - want[fin, 0]) <= R.RT60_BAR * np.abs(want[fin, 0]))


# ---- DeviceFilePairs.screen ----------------------------------------------------------------------------------------------------------
def _corpus(root):
    from tests.filepairs_ref import write_wav
    rng = np.random.default_rng(3)
    lists = {}
    for name, specs in (("clean", ((8000, 1, 3000), (16000, 2, 2500))), ("noise", ((16000, 1, 1700), (8000, 2, 2100))),
                        ("rir", ((16000, 1, 900), (8000, 1, 700)))):
        paths = []
        for k, (rate, ch, frames) in enumerate(specs):
            if name == "rir":
                x = np.exp(-6.908 * np.arange(frames) / (0.02 * rate)) * rng.standard_normal(frames) * 0.5
                x = np.repeat(x[:, None], ch, 1)
            else:
                x = 0.2 * rng.standard_normal((frames, ch))
            p = root / f"{name}{k}.wav"
            write_wav(p, np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16).ravel(), rate, ch)
            paths.append(str(p))
        lst = root / f"{name}.txt"
        lst.write_text("".join(f"{p}\n" for p in paths))
        lists[name] = (str(lst), paths)
    return lists


def test_device_file_pairs_screen_reports_and_changes_nothing(tmp_path):
    from cruse_amd import ops
    from cruse_amd.filepairs import DeviceFilePairs, load_pool
    lists = _corpus(tmp_path)

    def make():
        return DeviceFilePairs(clean_dataset=lists["clean"][0], noise_dataset=lists["noise"][0], rir_dataset=lists["rir"][0], snr_range=[0, 20],
                               silence_length=0.02, sub_sample_length=0.25, sr=16000, dataset_length=4, seed=7, reverb_proportion=1.0,
                               rir_len=1000)
    a, b = make(), make()
    idx = torch.arange(4)
    first_a, first_b = a.device_batch(idx, dev()), b.device_batch(idx, dev())
    rep = a.screen(dev())
    second_a, second_b = a.device_batch(idx, dev()), b.device_batch(idx, dev())
    torch.cuda.synchronize()
    for x, y in zip(first_a + second_a, first_b + second_b):                  # the batches before and after are those of a dataset never screened
        assert torch.equal(x, y)
    assert sorted(rep) == ["clean", "noise", "rir"] and len(a) == 4
    for name in ("clean", "noise"):
        paths = lists[name][1]
        pool, start, lens, _ = load_pool(paths, dev(), 16000)
        want = ops.screen_clips(pool, start, lens).cpu().numpy()
        t = rep[name]
        assert t["names"] == paths and np.array_equal(t["seconds"], lens / 16000.0)
        for k, col in enumerate(ops.SCREEN_COLUMNS):
            assert np.array_equal(t[col], want[:, k]), (name, col)
        assert t["reason"] == ["", ""] and t["keep"].tolist() == [0, 1] and "rt60" not in t
    t = rep["rir"]
    assert t["rt60"].shape == (2,) and np.all(np.isfinite(t["rt60"])) and np.all(np.abs(t["rt60"] - 0.02) < 0.01)
    assert t["seconds"].tolist() == [900 / 16000.0, 1000 / 16000.0]           # the second response (1400 samples at 16 kHz) is cut to rir_len


def test_screen_files_and_the_command_line(tmp_path, capsys):
    from cruse_amd import ops, screen as S, wavio
    from cruse_amd.filepairs import load_pool
    lists = _corpus(tmp_path)
    paths = lists["clean"][1] + lists["noise"][1]                              # 6000, 2500, 1700, 4200 samples at 16 kHz
    res = S.screen_files(paths, device=dev(), min_duration=0.15, total_hrs=0.3 / 3600)
    pool, start, lens, _ = load_pool(paths, dev(), 16000)
    want = ops.screen_clips(pool, start, lens).cpu().numpy()
    assert res["names"] == paths and res["seconds"].tolist() == [6000 / 16000, 2500 / 16000, 1700 / 16000, 4200 / 16000]
    for k, col in enumerate(ops.SCREEN_COLUMNS):
        assert np.array_equal(res[col], want[:, k]), col
    assert res["reason"] == ["", "", "too_short", ""] and res["keep"].tolist() == [0]      # 0.375 s reaches the budget of 0.3 s
    assert "rt60" not in res
    rir = S.screen_files(lists["rir"][1], device=dev(), max_rt60=0.001)        # max_rt60 implies the RT60 columns
    assert rir["reason"] == ["large_rt60", "large_rt60"] and rir["keep"].size == 0 and np.all(rir["t_peak"] >= 0)
    out, csv_path = tmp_path / "selected.txt", tmp_path / "stats.csv"
    assert S.main(["--list", lists["clean"][0], "--out", str(out), "--rejected-prefix", str(tmp_path / "rej"), "--csv", str(csv_path),
                   "--min-duration", "0.2", "--device", str(dev())]) == 0
    assert wavio.read_list(str(out)) == lists["clean"][1][:1] and wavio.read_list(str(tmp_path / "rej_too_short.txt")) == lists["clean"][1][1:]
    said = capsys.readouterr().out
    assert "\t Original files: 2" in said and "1 files. " in said and "\t is_too_short: 1" in said and said.rstrip().endswith("succeed")
    rows = csv_path.read_text().splitlines()
    assert rows[0].startswith("name,seconds,peak,n_clipped,rms,n_windows,n_active,activity,reason,keep") and len(rows) == 3
    assert S.main(["--dir", str(tmp_path), "--out", str(out), "--device", str(dev())]) == 0
    assert len(wavio.read_list(str(out))) == 6
