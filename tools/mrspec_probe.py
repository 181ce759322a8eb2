#!/usr/bin/env python3
"""Timings of the multi-resolution spectral loss -> profiles/mrspec_probe.json.

    python tools/mrspec_probe.py [--out profiles/mrspec_probe.json] [--calls 30] [--skip-engine]

  op       cruse_mrspec_loss alone at B = 64, L = 64000, n_ffts (128, 256, 512): forward only and with the gradient
  torch    the same loss through torch autograd of tests/mrspec_ref.py on the device (torch.stft on the device's FFT library): the yardstick
  engine   one TrainEngine step (bf16, B = 64 x 4 s) with loss = "mrspec" against loss = "si_snr" on the same build
Every figure is the median of --calls timed calls (HIP events around each call) after 5 warm-up calls."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, calls, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrspec_probe.json"))
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--skip-engine", action="store_true")
    args = ap.parse_args()
    from cruse_amd import ops
    import mrspec_ref as R
    B, L, n_ffts, gamma, factor, fc = 64, 64000, (128, 256, 512), 0.3, 1.0, 1.0
    g = torch.Generator().manual_seed(0)
    ref = (0.1 * torch.randn(B, L, generator=g)).cuda()
    est = (ref + 0.05 * torch.randn(B, L, generator=g).cuda()).contiguous()
    res = {"shape": {"B": B, "L": L, "n_ffts": list(n_ffts), "gamma": gamma}, "device": torch.cuda.get_device_name(0),
           "ws_bytes": ops.mrspec_ws_bytes(B, L, n_ffts), "launches": {"forward": len(n_ffts) + 1, "with_gradient": len(n_ffts) + 2}}
    res["op_forward"] = timed(lambda: ops.mrspec_loss(est, ref, n_ffts, gamma, factor, fc, want_grad=False), args.calls)
    res["op_with_gradient"] = timed(lambda: ops.mrspec_loss(est, ref, n_ffts, gamma, factor, fc), args.calls)

    def torch_fwd():
        with torch.no_grad():
            return R.mrspec_loss(est, ref, n_ffts, gamma, factor, fc)

    def torch_bwd():
        x = est.detach().requires_grad_(True)
        R.mrspec_loss(x, ref, n_ffts, gamma, factor, fc).backward()
        return x.grad

    res["torch_forward"] = timed(torch_fwd, args.calls)
    res["torch_with_gradient"] = timed(torch_bwd, args.calls)
    lo, dx = ops.mrspec_loss(est, ref, n_ffts, gamma, factor, fc)
    res["op_vs_torch_device"] = {"loss_rel": abs(float(lo) - float(torch_fwd())) / float(lo), "grad_rel_l2": R.rel_l2(dx.cpu(), torch_bwd().cpu())}
    if not args.skip_engine:
        from cruse_amd.data import synth_batch
        from cruse_amd.engine import TrainEngine
        from cruse_amd.model.cruse_net import unet_2
        noisy, clean = synth_batch(64, 64000, "cuda", 1)
        for loss in ("si_snr", "mrspec"):
            torch.manual_seed(0)
            eng = TrainEngine(unet_2(rnn_groups=1, precision="bf16").cuda(), lr=1e-3, use_graph=True, loss=loss, mrs_f_complex=1.0)
            res["engine_step_" + loss] = timed(lambda: eng.step(noisy, clean), args.calls)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
