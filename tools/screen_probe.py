"""What the file screening costs -> profiles/screen_probe.json: ops.screen_clips on a pool of synthetic utterances
(default 1 GiB of f32: 4 s to 12 s each at odd offsets) and ops.rt60 on 1000 responses of 8000 samples, timed with HIP events (median of
10 calls after 3 warm-up calls, plans and outputs made beforehand), beside a plain torch composition of peak and rms over the same pool
(a zero-padded [n, max_len] batch: amax |x| and sqrt(sum x^2 / len)) in the same run.  Bytes per second are the pool's bytes over the
median time; the card's HBM figure stands beside them.  The times are a record, not a bar.
usage: python tools/screen_probe.py [--gib 1.0] [--responses 1000] [--response-len 8000] [--out profiles/screen_probe.json]"""
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

from tools.sdr_probe import timed_ms  # noqa: E402

HBM_PEAK_GBPS = 8000.0        # MI355X: 8 TB/s HBM3E (data sheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--responses", type=int, default=1000)
    ap.add_argument("--response-len", type=int, default=8000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_probe.json"))
    args = ap.parse_args()
    from cruse_amd import ops
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    total = int(args.gib * (1 << 28))                         # f32 samples
    lens, pos, start = [], 0, []
    while pos < total:
        n = int(rng.integers(4 * 16000, 12 * 16000)) | 1      # odd lengths: every alignment of the first sample occurs
        n = min(n, total - pos)
        start.append(pos)
        lens.append(n)
        pos += n
    start, lens = np.asarray(start, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    pool = torch.empty(total, device=dev, dtype=torch.float32).normal_(0.0, 0.05)
    plan = ops.ragged_plan(pool, start, lens)
    out = torch.empty(len(lens), 6, device=dev, dtype=torch.float64)
    res = {"device": torch.cuda.get_device_name(0), "warmup": 3, "calls": 10, "hbm_peak_gbps": HBM_PEAK_GBPS,
           "pool_bytes": 4 * total, "utterances": int(len(lens)), "windows": int(plan.windows(800)[1])}
    med, lo = timed_ms(lambda: ops.screen_clips(pool, plan=plan, out=out))
    res["screen_clips"] = {"median_ms": med, "min_ms": lo, "gbps": 4 * total / (med * 1e-3) / 1e9,
                           "of_hbm_peak": 4 * total / (med * 1e-3) / 1e9 / HBM_PEAK_GBPS}
    # the yardstick: peak and rms by torch over a zero-padded batch gathered from the same pool (the gather is not timed)
    maxlen = int(lens.max())
    idx = torch.from_numpy(start).to(dev)[:, None] + torch.arange(maxlen, device=dev)[None, :]
    mask = torch.arange(maxlen, device=dev)[None, :] < torch.from_numpy(lens).to(dev)[:, None]
    padded = torch.where(mask, pool[idx.clamp_(max=total - 1)], torch.zeros((), device=dev))
    del idx, mask
    ln = torch.from_numpy(lens).to(dev).double()

    def torch_peak_rms():
        return padded.abs().amax(dim=1), (padded.double().square().sum(dim=1) / ln).sqrt()
    med, lo = timed_ms(torch_peak_rms)
    res["torch_peak_rms_padded"] = {"median_ms": med, "min_ms": lo, "padded_bytes": 4 * padded.numel(),
                                    "gbps_of_pool": 4 * total / (med * 1e-3) / 1e9}
    pk, rms = torch_peak_rms()
    res["agreement"] = {"peak_equal": bool(torch.equal(pk.double(), out[:, 0])),
                        "rms_max_rel": float(((rms - out[:, 2]).abs() / out[:, 2]).max())}
    del padded
    # rt60: exponential decays under noise
    R, n = args.response_len, args.responses
    t = torch.arange(R, device=dev, dtype=torch.float64)
    T = torch.linspace(0.1, 0.4, n, device=dev, dtype=torch.float64)[:, None]
    h = (torch.exp(-6.908 * t[None, :] / (T * 16000.0)) * torch.randn(n, R, device=dev, dtype=torch.float64)).float().reshape(-1)
    rplan = ops.ragged_plan(h, np.arange(n, dtype=np.int64) * R, np.full(n, R, dtype=np.int64))
    rout = torch.empty(n, 3, device=dev, dtype=torch.float64)
    med, lo = timed_ms(lambda: ops.rt60(h, plan=rplan, out=rout))
    res["rt60"] = {"responses": n, "len": R, "median_ms": med, "min_ms": lo, "gbps": 4 * n * R / (med * 1e-3) / 1e9,
                   "finite": int(torch.isfinite(rout[:, 0]).sum()),
                   "max_rel_dev_from_T": float(((rout[:, 0] - T[:, 0]).abs() / T[:, 0]).max())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
