"""CPU: the float64 restatement of the file-screening kernels (tests/screen_ref.py) against the reference's own results
(tests/golden/screen.npz), the host surface of cruse_screen_clips / cruse_rt60 (header, ctypes table, library, every refusal), and the
list builder's decisions (cruse_amd.screen) on a hand-made statistics table."""
import os
import re

import numpy as np
import pytest

from tests import screen_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("cruse_screen_ws_bytes", "cruse_screen_clips", "cruse_rt60_ws_bytes", "cruse_rt60")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_reference(golden):
    g = golden("screen.npz")
    inputs = R.golden_inputs()
    assert [n for n, _ in inputs] == g["names"].tolist()
    dist = float(g["rms_distance"])
    assert 0.0 < dist < 1e-6 and float(g["margin"]) >= R.MARGIN              # float32 sums of up to 40 001 squares
    for i, (name, x) in enumerate(inputs):
        s, n = int(g["start"][i]), int(g["length"][i])
        assert np.array_equal(g["pool"][s:s + n], x), name                   # the committed inputs are the generator's
        row = R.screen_row(x)
        assert R.min_margin(x) >= R.MARGIN, name
        assert row[5] == g["perc_active"][i], name                           # exact: no decision is near the threshold
        assert (row[1] > 0) == bool(g["is_clipped"][i]), name
        assert abs(row[2] - g["rms"][i]) <= 2.0 * dist * max(row[2], 1e-30), name
    by = dict(zip(g["names"].tolist(), range(len(inputs))))
    assert not g["is_clipped"][by["edge_below"]] and g["is_clipped"][by["edge_above"]] and g["is_clipped"][by["square"]]
    assert g["perc_active"][by["zeros"]] == 0.0 and 0.0 < g["perc_active"][by["speech40001"]] < 1.0


def test_restatement_edge_rows():
    assert np.array_equal(R.screen_row(np.zeros(0, np.float32)), [0, 0, 0, 0, 0, np.nan], equal_nan=True)
    sq = np.where(np.arange(1601) % 2 == 0, 1.0, -1.0).astype(np.float32)
    assert R.screen_row(sq).tolist() == [1.0, 1601.0, 1.0, 3.0, 3.0, 1.0]
    x = np.zeros(800, np.float32)
    x[5] = np.float32(0.999)
    assert R.screen_row(x)[1] == 0.0                                         # compared in float32, as numpy compares the reference's
    x[5] = np.nextafter(np.float32(0.999), np.float32(2.0))
    assert R.screen_row(x)[1] == 1.0


def test_rt60_restatement():
    for name, h, want in R.rt60_inputs():
        row = R.rt60_row(h)
        if isinstance(want, str):
            assert np.isnan(row[0]), name
        elif want is not None:
            assert abs(row[0] - want) <= 1e-9 * want, (name, row[0], want)   # the float32 samples of an exact line
    rows = dict((n, R.rt60_row(h)) for n, h, _ in R.rt60_inputs())
    assert rows["predelay37"][1] == 37.0 and rows["peak_last"][1] == 299.0 and rows["zeros"][1] == 0.0
    assert np.isnan(rows["empty"]).all() and rows["truncated"][2] > -25.0
    worst = R.rt60_order_disagreement()
    print(f"sequential vs pairwise: {worst:.3e} (recorded {R.RT60_MEASURED:.3e}, bar {R.RT60_BAR:.3e})")
    assert worst < R.RT60_BAR


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from cruse_amd._abi_check import parse_header
    from cruse_amd._lib import ABI_VERSION, SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert "#define CRUSE_ABI_VERSION 15" in header and ABI_VERSION == 15 and lib.cruse_abi_version() == 15       # additive symbols
    parsed = parse_header()
    for sym in SYMBOLS:
        assert re.search(rf"\b(int|long long) {sym}\(", header), f"{sym} is not declared in include/cruse_hip.h"
        assert SIGNATURES[sym] == parsed[sym]
        assert hasattr(lib, sym)
    assert re.search(r"\bscreen\b", open(os.path.join(ROOT, "cruse_amd", "csrc", "build.sh")).read())
    assert lib.cruse_screen_ws_bytes(8, 58) == 58 * 16 and lib.cruse_screen_ws_bytes(0, 0) == 0
    assert lib.cruse_rt60_ws_bytes(3, 2049) == 3 * 2 * 8 and lib.cruse_rt60_ws_bytes(5, 0) == 0
    for bad in ((-1, 0), (1, -1), (1, 2 ** 31)):
        assert lib.cruse_screen_ws_bytes(*bad) == -1, bad
    for bad in ((-1, 8), (1, -1), (1, (1 << 24) + 1)):
        assert lib.cruse_rt60_ws_bytes(*bad) == -1, bad


SCREEN_GOOD = dict(pool=1, start=1, len=1, win_first=1, n=2, total_windows=5, window=800, clip_thr=0.999, target_db=-25.0, act_thr=0.13, ws=1,
                   out=1)
RT60_GOOD = dict(pool=1, start=1, len=1, n=2, max_len=8000, sr=16000, lo_db=-5.0, hi_db=-25.0, ws=1, out=1)
SCREEN_REFUSALS = [(dict(n=-1), "n = -1"), (dict(window=0), "window = 0"), (dict(window=-800), "window = -800"),
                   (dict(total_windows=-1), "total_windows = -1"), (dict(total_windows=2 ** 31), "total_windows = 2147483648"),
                   (dict(pool=0), "null buffer"), (dict(start=0), "null buffer"), (dict(len=0), "null buffer"),
                   (dict(win_first=0), "null buffer"), (dict(ws=0), "null buffer"), (dict(out=0), "null buffer")]
RT60_REFUSALS = [(dict(n=-1), "n = -1"), (dict(max_len=-1), "max_len = -1"), (dict(max_len=(1 << 24) + 1), "max_len = 16777217"),
                 (dict(sr=0), "sr = 0"), (dict(lo_db=-25.0), "lo_db = -25 <= hi_db = -25"), (dict(lo_db=-30.0), "lo_db = -30 <= hi_db = -25"),
                 (dict(pool=0), "null buffer"), (dict(start=0), "null buffer"), (dict(len=0), "null buffer"), (dict(ws=0), "null buffer"),
                 (dict(out=0), "null buffer")]
POINTERS = ("pool", "start", "len", "win_first", "ws", "out")


def _call(name, good, **change):
    """(return code, message) of the real entry point on stand-in pointers: the host only asks whether a pointer is null"""
    from cruse_amd._lib import lib
    from tests.test_stream_boundary_host import standin
    P = standin()
    vals = [(P if v else None) if k in POINTERS else v for k, v in dict(good, **change).items()]
    rc = getattr(lib, name)(*vals, None)
    return rc, lib.cruse_last_error().decode()


@pytest.mark.parametrize("name,good,refusals", [("cruse_screen_clips", SCREEN_GOOD, SCREEN_REFUSALS), ("cruse_rt60", RT60_GOOD, RT60_REFUSALS)],
                         ids=["screen_clips", "rt60"])
def test_every_refusal_comes_with_its_code_and_message(name, good, refusals):
    for change, msg in refusals:
        rc, said = _call(name, good, **change)
        assert rc == -1 and said.startswith(name + ":") and msg in said, (change, rc, said)
    from cruse_amd._lib import lib
    from tests.test_stream_boundary_host import standin
    vals = [(standin() + 4 if k in ("ws",) else standin()) if k in POINTERS else v for k, v in good.items()]
    assert getattr(lib, name)(*vals, None) == -2 and b"aligned" in lib.cruse_last_error()                       # CRUSE_E_ALIGN
    assert _call(name, good, n=0)[0] == 0                                     # nothing to do is no launch and no error


def test_tables_are_judged_on_the_host():
    from cruse_amd import ops
    for start, length in (([-1], [4]), ([0], [-1]), ([8], [3]), ([0, 1], [1])):
        with pytest.raises(ValueError, match="screen:"):
            ops.RaggedPlan(10, start, length, "cpu")
    with pytest.raises(ValueError, match="integer"):
        ops.RaggedPlan(10, [0.5], [1], "cpu")


# ---- the list builder ------------------------------------------------------------------------------------------------------------------
def test_reason_order_and_hours_budget():
    from cruse_amd import screen as S
    #          0      1      2      3      4      5      6      7
    seconds = [1.0, 10.0, 10.0, 10.0, 10.0, 1.0, 10.0, 10.0]
    nclip = [3, 2, 0, 0, 0, 0, 0, 0]
    act = [0.1, 0.1, 0.1, 0.9, 0.9, 0.1, np.nan, 0.9]
    rt = [2.0, 2.0, 2.0, 2.0, 0.5, 2.0, np.nan, 0.5]
    kw = dict(min_duration=3.0, min_activity=0.6, max_rt60=1.0)
    reason, keep = S.decide(seconds, nclip, act, rt, **kw)
    # the first that applies, in the reference's order: too_short, clipped, low_activity, large_rt60; a NaN statistic rejects nothing
    assert reason == ["too_short", "clipped", "low_activity", "large_rt60", "", "too_short", "", ""]
    assert keep.tolist() == [4, 6, 7]
    assert S.decide(seconds, nclip, act, rt)[0] == ["clipped", "clipped", "", "", "", "", "", ""]                # thresholds off
    assert S.decide(seconds, nclip, act, None, **kw)[0][3] == ""                                                  # no rt60 column
    # the budget is looked at after a file was added: the file that reaches it is kept, the next is not
    for hrs, want in ((None, [4, 6, 7]), (1.0, [4, 6, 7]), (29.9 / 3600, [4, 6, 7]), (19.9 / 3600, [4, 6]), (15.0 / 3600, [4, 6]),
                      (9.9 / 3600, [4]), (0.0, [4])):
        assert S.decide(seconds, nclip, act, rt, total_hrs=hrs, **kw)[1].tolist() == want, hrs
    res = dict(names=[f"f{i}.wav" for i in range(8)], seconds=np.asarray(seconds), reason=reason, keep=keep)
    text = S.summary(res)
    assert "\t Original files: 8" in text and f"\t Selected files: {30.0 / 3600} hrs, 3 files. " in text
    for line in ("\t is_clipped_wav: 1", "\t is_low_activity: 1", "\t is_too_short: 2", "\t is_too_largeRT60: 1"):
        assert line in text


def test_write_lists_round_trips_through_read_list(tmp_path):
    from cruse_amd import screen as S
    from cruse_amd import wavio
    names = [str(tmp_path / f"a b {i}.wav") for i in range(5)]
    res = dict(names=names, seconds=np.ones(5), reason=["", "clipped", "", "too_short", "large_rt60"], keep=np.array([0, 2]))
    out = str(tmp_path / "selected.txt")
    written = S.write_lists(res, out, rejected_prefix=str(tmp_path / "rejected"))
    assert wavio.read_list(out) == [names[0], names[2]]
    assert len(written) == 5
    for r, want in (("clipped", [names[1]]), ("too_short", [names[3]]), ("large_rt60", [names[4]]), ("low_activity", [])):
        assert wavio.read_list(str(tmp_path / f"rejected_{r}.txt")) == want
    assert S.write_lists(res, out) == [out]


def test_the_reexport_imports_without_side_effects(tmp_path, monkeypatch):
    import importlib
    monkeypatch.chdir(tmp_path)
    mod = importlib.import_module("dataset.preprocess_dataset")
    from cruse_amd import screen as S
    assert mod.screen_files is S.screen_files and mod.write_lists is S.write_lists and mod.main is S.main
    assert os.listdir(tmp_path) == []                                         # the reference's module writes two lists when run
    with pytest.raises(SystemExit):
        S.main(["--out", "x.txt"])                                            # --list or --dir is required
