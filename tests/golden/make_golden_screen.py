#!/usr/bin/env python3
"""tests/golden/screen.npz: the reference's own tailor_dB_FS, is_clipped and activity_detector (train_base/acoustics/feature.py:99-107,
:194-236) RUN on the inputs of tests/screen_ref.golden_inputs(), lifted from their source file at run time as make_golden_r2.py lifts
PreProcess (top_level_block; the module itself imports librosa and is never imported).  Only inputs, outputs and the observed distance
between the reference's float32 results and the float64 restatement are stored -- no reference text.

    python tests/golden/make_golden_screen.py [--ref /root/reference]

Asserted here, on the CPU: every window's smoothed probability of every input is at least screen_ref.MARGIN away from the activity
threshold in the float64 restatement (so float32-vs-float64 summation cannot flip a decision), and under that condition the
reference's perc_active and is_clipped equal the restatement's exactly."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import read_src, top_level_block  # noqa: E402
from tests import screen_ref as R  # noqa: E402


def lift(ref):
    ns = {"np": np}
    src = read_src(ref, "train_base/acoustics/feature.py")
    for fn in ("tailor_dB_FS", "is_clipped", "activity_detector"):
        exec(top_level_block(src, f"def {fn}("), ns)
    return ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    ns = lift(args.ref)
    inputs = R.golden_inputs()
    names, pool, start, length = [], [], [], []
    perc, clipped, rms32, dist, margin = [], [], [], 0.0, np.inf
    pos = 0
    for name, x in inputs:
        assert x.dtype == np.float32
        names.append(name)
        start.append(pos)
        length.append(x.shape[0])
        pool.append(x)
        pos += x.shape[0]
        row = R.screen_row(x)
        m = R.min_margin(x)
        margin = min(margin, m)
        assert m >= R.MARGIN, (name, m)
        _, rms, _ = ns["tailor_dB_FS"](x.copy(), R.TARGET_DB)                     # float32 arithmetic, as the reference runs it
        c = bool(ns["is_clipped"](x.copy(), R.CLIP_THR))
        p = float(ns["activity_detector"](x.copy(), 16000, R.ACT_THR, R.TARGET_DB))
        assert p == row[5], (name, p, row[5])
        assert c == (row[1] > 0), (name, c, row[1])
        if row[2] > 0:
            dist = max(dist, abs(float(rms) - row[2]) / row[2])
        perc.append(p)
        clipped.append(c)
        rms32.append(float(rms))
    out = os.path.join(HERE, "screen.npz")
    np.savez_compressed(out, names=np.array(names), pool=np.concatenate(pool), start=np.array(start, dtype=np.int64),
                        length=np.array(length, dtype=np.int64), perc_active=np.array(perc), is_clipped=np.array(clipped),
                        rms=np.array(rms32), rms_distance=np.array(dist), margin=np.array(margin))
    print(f"{out}: {len(names)} inputs, min margin {margin:.3e}, f32-vs-f64 rms distance {dist:.3e}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
