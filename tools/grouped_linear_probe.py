#!/usr/bin/env python3
"""Times one SqueezedGRU(640, 256, 640, linear_groups=8) forward + backward at B x T = 64 x 401, twice: with the single-launch grouped
linears (cruse_grouped_linear_*) and with the per-group ops.gemm loop they replace (G launches forward, 2 G backward, per linear).
The loop lives here only, as the yardstick.  The GRU between the two linears is the same code in both runs.

    python tools/grouped_linear_probe.py [--iters 10] [--out FILE.json]

HIP events around forward + backward, median and minimum over --iters after 3 warm-up runs; also the two grouped linears alone
(forward + backward without the GRU).  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from cruse_amd import ops  # noqa: E402
from cruse_amd.model.based_model import cust_conv as C  # noqa: E402

LAUNCHES = {"n": 0}


class _LoopFn(torch.autograd.Function):
    """GroupedLinearEinsum as G ops.gemm calls forward and 2 G backward (exact-f32 MFMA as well)"""

    @staticmethod
    def forward(ctx, x, w):
        G, Ig, Hg = w.shape
        rows = x.shape[0]
        y = torch.empty(rows, G * Hg, device=x.device)
        for g in range(G):
            ops.gemm(False, False, rows, Hg, Ig, x, g * Ig, G * Ig, w, g * Ig * Hg, Hg, y, g * Hg, G * Hg, prec="f32")
        LAUNCHES["n"] += G
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        G, Ig, Hg = w.shape
        rows = x.shape[0]
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dw = torch.zeros_like(w)
        sk = max(1, min(8, rows // 512))
        for g in range(G):
            ops.gemm(False, True, rows, Ig, Hg, dy, g * Hg, G * Hg, w, g * Ig * Hg, Hg, dx, g * Ig, G * Ig, prec="f32")
            ops.gemm(True, False, Ig, Hg, rows, x, g * Ig, G * Ig, dy, g * Hg, G * Hg, dw, g * Ig * Hg, Hg, accumulate=True, splitk=sk,
                     prec="f32")
        LAUNCHES["n"] += 2 * G + 1                                   # (+ the fill of dw)
        return dx, dw


def _loop_run(self, x, relu):
    b, t, i = x.shape
    y = _LoopFn.apply(x.reshape(b * t, i).contiguous(), self.weight)
    return (torch.relu(y) if relu else y).view(b, t, self.hidden_size)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 3), "min_ms": round(ms[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    B, T = 64, 401
    m = C.SqueezedGRU(640, 256, 640, linear_groups=8).cuda()
    x = torch.randn(B, T, 640, device="cuda", requires_grad=True)
    lin_in, lin_out = m.linear_in[0], m.linear_out[0]
    z = torch.randn(B, T, 256, device="cuda", requires_grad=True)

    def block():
        m.zero_grad(set_to_none=True)
        x.grad = None
        y, h = m(x)
        y.backward(y.detach())

    def linears():
        m.zero_grad(set_to_none=True)
        x.grad = z.grad = None
        a, b = lin_in(x), lin_out(z)
        torch.autograd.backward((a, b), (a.detach(), b.detach()))

    res = {"shape": {"B": B, "T": T, "input": 640, "hidden": 256, "output": 640, "groups": 8}, "iters": args.iters}
    original = C.GroupedLinearEinsum._run
    res["kernels"] = {"block": timed(block, args.iters), "linears": timed(linears, args.iters),
                      "launches_per_linear": {"fwd": 1, "bwd": 2 + (1 if ops.lib.cruse_grouped_linear_dw_ws_bytes(B * T, 8, 80, 32) else 0)}}
    C.GroupedLinearEinsum._run = _loop_run
    try:
        res["gemm_loop"] = {"block": timed(block, args.iters), "linears": timed(linears, args.iters)}
        LAUNCHES["n"] = 0
        linears()
        res["gemm_loop"]["launches_two_linears_fwd_bwd"] = LAUNCHES["n"]
    finally:
        C.GroupedLinearEinsum._run = original
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
