"""What the on-device bss_eval SDR costs -> profiles/sdr_probe.json: metrics.sdr at B = 64 clips of 4 s, K = 512,
timed with HIP events (median of 10 calls after 3 warm-up calls), beside metrics.si_sdr and metrics.stoi on the same tensors in the same
run.  The time is a record, not a bar.
usage: python tools/sdr_probe.py [--batch 64] [--seconds 4] [--filter-len 512] [--out profiles/sdr_probe.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed_ms(fn, warm=3, n=10):
    """median and minimum of n event-timed calls, milliseconds"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--filter-len", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdr_probe.json"))
    args = ap.parse_args()
    from cruse_amd import metrics
    from cruse_amd.data import synth_batch
    dev = torch.device("cuda", 0)
    B, L, K = args.batch, int(round(args.seconds * 16000)), args.filter_len
    noisy, clean = synth_batch(B, L, dev, 3)
    res = {"B": B, "L": L, "filter_len": K, "device": torch.cuda.get_device_name(0), "warmup": 3, "calls": 10}
    for name, fn in (("sdr", lambda: metrics.sdr(clean, noisy, filter_len=K)), ("si_sdr", lambda: metrics.si_sdr(clean, noisy)),
                     ("stoi", lambda: metrics.stoi(clean, noisy))):
        med, lo = timed_ms(fn)
        res[name] = {"median_ms": med, "min_ms": lo}
    score = metrics.sdr(clean, noisy, filter_len=K)
    res["sdr"]["mean_db"] = float(score.double().mean())
    res["sdr"]["finite"] = bool(torch.isfinite(score).all())
    res["sdr"]["clips_per_s"] = B / (res["sdr"]["median_ms"] * 1e-3)
    # the multiply-adds of the definition: 2 K n for the correlations, K (n + K - 1) for the projection, per clip
    res["sdr"]["gfma_per_s"] = B * (2.0 * K * L + K * (L + K - 1.0)) / (res["sdr"]["median_ms"] * 1e-3) / 1e9
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
