"""Which files belong on a training list: the reference's list builder dataset/preprocess_dataset.py with its four
rejections -- too short, clipped, low speech activity, RT60 too large -- and its hours budget, on statistics computed on the device by
cruse_screen_clips and cruse_rt60 from the pool filepairs.load_pool leaves in HBM.  In the reference the four tests are stubs set to 0
(preprocess_dataset.py:130-133) and utils.cal_rt60 cannot run, so the tests here are the functions it names (feature.is_clipped,
feature.activity_detector) and a broadband T20 (ops.rt60 states the departure from cal_rt60)."""
from __future__ import annotations

import argparse
import csv
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

REASONS = ("too_short", "clipped", "low_activity", "large_rt60")          # the reference's order (preprocess_dataset.py:135-145)
SUMMARY_NAMES = {"clipped": "is_clipped_wav", "low_activity": "is_low_activity", "too_short": "is_too_short", "large_rt60": "is_too_largeRT60"}


def decide(seconds, n_clipped, activity, rt60=None, min_duration=None, min_activity=None, max_rt60=None, total_hrs=None):
    """-> (reason per file, keep): reason is "" or the FIRST of REASONS that applies -- seconds < min_duration, n_clipped > 0,
    activity < min_activity, rt60 > max_rt60 (a test whose threshold is None is off; a NaN statistic rejects nothing) -- and keep the
    indices of the files without a reason, in list order, up to and including the one with which their accumulated duration reaches
    total_hrs * 3600 (preprocess_dataset.py:147-153: the budget is looked at after a file was added)."""
    seconds = np.asarray(seconds, dtype=np.float64)
    n = seconds.shape[0]
    tests = (
        seconds < min_duration if min_duration is not None else np.zeros(n, dtype=bool),
        np.asarray(n_clipped) > 0,
        np.asarray(activity, dtype=np.float64) < min_activity if min_activity is not None else np.zeros(n, dtype=bool),
        np.asarray(rt60, dtype=np.float64) > max_rt60 if (max_rt60 is not None and rt60 is not None) else np.zeros(n, dtype=bool),
    )
    reason = [""] * n
    for name, hit in reversed(list(zip(REASONS, tests))):                 # the first that applies wins
        for i in np.flatnonzero(hit):
            reason[i] = name
    keep, acc = [], 0.0
    for i in range(n):
        if reason[i]:
            continue
        acc += float(seconds[i])
        keep.append(i)
        if total_hrs is not None and acc >= float(total_hrs) * 3600.0:
            break
    return reason, np.asarray(keep, dtype=np.int64)


def table(names: Sequence[str], lengths, sr: int, stats: np.ndarray, rt: Optional[np.ndarray], **thresholds) -> Dict:
    """the result of screen_files from the read-back statistics: names, seconds, one numpy column per statistic, reason, keep"""
    from . import ops
    out = {"names": list(names), "seconds": np.asarray(lengths, dtype=np.float64) / float(sr)}
    for k, col in enumerate(ops.SCREEN_COLUMNS):
        out[col] = stats[:, k].copy()
    if rt is not None:
        for k, col in enumerate(ops.RT60_COLUMNS):
            out[col] = rt[:, k].copy()
    out["reason"], out["keep"] = decide(out["seconds"], out["n_clipped"], out["activity"], out.get("rt60"), **thresholds)
    return out


def stats_of(pool, start, lengths, sr: int, clipping_threshold: float = 0.999, with_rt60: bool = False):
    """both ops on one pool and ONE read-back -> (stats [n, 6], rt60 rows [n, 3] or None) as numpy"""
    import torch
    from . import ops
    plan = ops.ragged_plan(pool, start, lengths)
    dev = [ops.screen_clips(pool, sr=sr, clip_threshold=clipping_threshold, plan=plan)]
    if with_rt60:
        dev.append(ops.rt60(pool, sr=sr, plan=plan))
    host = torch.cat(dev, dim=1).cpu().numpy()
    return host[:, :6], (host[:, 6:] if with_rt60 else None)


def screen_files(paths: Sequence[str], device="cuda", sr: int = 16000, min_duration: Optional[float] = None,
                 clipping_threshold: float = 0.999, min_activity: Optional[float] = None, max_rt60: Optional[float] = None,
                 total_hrs: Optional[float] = None, rt60: bool = False) -> Dict:
    """Read the 16-bit PCM WAV files once (filepairs.load_pool: resampled to `sr`, channel 0), compute their statistics on the device
    and decide (decide()).  rt60 = True treats the files as impulse responses and adds the columns of ops.rt60; max_rt60 implies it.
    -> dict: names, seconds, peak, n_clipped, rms, n_windows, n_active, activity (, rt60, t_peak, edc_floor_db), reason, keep."""
    from .filepairs import load_pool
    paths = list(paths)
    with_rt = bool(rt60) or max_rt60 is not None
    if not paths:
        z = np.zeros((0, 6))
        return table([], [], sr, z, np.zeros((0, 3)) if with_rt else None)
    pool, start, lens, _ = load_pool(paths, device, sr)
    stats, rt = stats_of(pool, start, lens, sr, clipping_threshold, with_rt)
    return table(paths, lens, sr, stats, rt, min_duration=min_duration, min_activity=min_activity, max_rt60=max_rt60, total_hrs=total_hrs)


def write_lists(result: Dict, dist_file: str, rejected_prefix: Optional[str] = None) -> List[str]:
    """The selected files, one path per line (what wavio.read_list reads; preprocess_dataset.py:155-156) -> dist_file; with
    rejected_prefix also one list per reason, <rejected_prefix>_<reason>.txt (the reference writes the low-activity one, :157-158).
    -> the files written."""
    written = []

    def put(path, names):
        with open(os.path.abspath(os.path.expanduser(path)), "w") as f:
            f.writelines(f"{name}\n" for name in names)
        written.append(path)
    put(dist_file, [result["names"][i] for i in result["keep"]])
    if rejected_prefix:
        for r in REASONS:
            put(f"{rejected_prefix}_{r}.txt", [n for n, why in zip(result["names"], result["reason"]) if why == r])
    return written


def write_csv(result: Dict, path: str) -> None:
    cols = [c for c in result if c not in ("names", "reason", "keep")]
    kept = set(int(i) for i in result["keep"])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name"] + cols + ["reason", "keep"])
        for i, name in enumerate(result["names"]):
            w.writerow([name] + [repr(float(result[c][i])) for c in cols] + [result["reason"][i], int(i in kept)])


def summary(result: Dict) -> str:
    """the reference's closing block (preprocess_dataset.py:163-173)"""
    hrs = float(np.sum(result["seconds"][result["keep"]])) / 3600.0
    lines = ["=" * 70, "Speech Preprocessing", f"\t Original files: {len(result['names'])}",
             f"\t Selected files: {hrs} hrs, {len(result['keep'])} files. "]
    for r in ("clipped", "low_activity", "too_short", "large_rt60"):
        lines.append(f"\t {SUMMARY_NAMES[r]}: {sum(1 for why in result['reason'] if why == r)}")
    return "\n".join(lines)


def find_files(directory: str, ext: Sequence[str] = ("wav",)) -> List[str]:
    """every file below `directory` with one of the extensions, sorted (librosa.util.find_files at :112-113; WAV only here)"""
    found = []
    for root, _, files in os.walk(os.path.abspath(os.path.expanduser(directory))):
        found += [os.path.join(root, f) for f in files if f.rsplit(".", 1)[-1].lower() in ext]
    return sorted(found)


def main(argv=None) -> int:
    from . import wavio
    ap = argparse.ArgumentParser(prog="preprocess_dataset", description="Screen a WAV file list on the device and write the selected list.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--list", help="a list file, one WAV path per line")
    src.add_argument("--dir", help="a directory searched for *.wav")
    ap.add_argument("--out", required=True, help="the selected list")
    ap.add_argument("--rejected-prefix", help="also write <prefix>_<reason>.txt per reason")
    ap.add_argument("--csv", help="write every file's statistics here")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--sr", type=int, default=16000)
    ap.add_argument("--min-duration", type=float, default=None, help="seconds")
    ap.add_argument("--clipping-threshold", type=float, default=0.999)
    ap.add_argument("--min-activity", type=float, default=None, help="fraction of active 50 ms windows")
    ap.add_argument("--max-rt60", type=float, default=None, help="seconds (implies --rt60)")
    ap.add_argument("--total-hrs", type=float, default=None)
    ap.add_argument("--rt60", action="store_true", help="the files are impulse responses: compute T20")
    a = ap.parse_args(argv)
    paths = wavio.read_list(a.list) if a.list else find_files(a.dir)
    result = screen_files(paths, device=a.device, sr=a.sr, min_duration=a.min_duration, clipping_threshold=a.clipping_threshold,
                          min_activity=a.min_activity, max_rt60=a.max_rt60, total_hrs=a.total_hrs, rt60=a.rt60)
    write_lists(result, a.out, a.rejected_prefix)
    if a.csv:
        write_csv(result, a.csv)
    print(summary(result))
    print("succeed")
    return 0
