"""What the fused DeepFilter head costs beside the two launches it replaces -> profiles/df_head_probe.json.

  new: cruse_df_head_apply(mask, nre, nim)                                       3 planes read, 2 written
  old: cruse_mask_apply(mask, ones, zeros) -> hr; cruse_deepfilter_fwd(nre, nim, hr, zeros)      7 planes read, 4 written
       (engine._deepfilter_loss's forward composition)

at B = 64, T = 401, Fs = 161 (Fn = 160), half-widths (1, 5).  Each variant is captured once as a graph of `--sets` calls, one per
input / output set, so that no host launch time is inside the window and the working set (sets x 5 planes of 16.5 MB) does not stay
in the 256 MB last-level cache; the two graphs are replayed ALTERNATELY, `--rounds` times each, between HIP events, in one process.
Reported: the median, minimum and quartiles of the per-call time of each variant, the byte counts from the shapes, and whether the
two variants' outputs are the same bits at this shape.  The time is a record, not a bar.
usage: python tools/df_head_probe.py [--batch 64] [--frames 401] [--sets 6] [--rounds 30] [--out profiles/df_head_probe.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=401)
    ap.add_argument("--bins", type=int, default=161)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "df_head_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("df_head_probe: needs a HIP device (a time taken elsewhere says nothing)")
    from cruse_amd import ops
    dev = torch.device("cuda", 0)
    B, T, Fs, td, fd = args.batch, args.frames, args.bins, 1, 5
    Fn, rows = Fs // 2 * 2, B * T
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(args.sets):
        s = dict(mask=torch.sigmoid(torch.randn(rows, Fn, device=dev, generator=g)), nre=torch.randn(B, T, Fs, device=dev, generator=g),
                 nim=torch.randn(B, T, Fs, device=dev, generator=g))
        for name in ("new_re", "new_im", "old_re", "old_im"):
            s[name] = torch.empty(B, T, Fs, device=dev)
        sets.append(s)
    ones, zeros = torch.ones(rows, Fs, device=dev), torch.zeros(rows, Fs, device=dev)      # (the engine keeps one pair per shape)

    def new(s):
        ops.df_head_apply(s["mask"], s["nre"], s["nim"], td, fd, out=(s["new_re"], s["new_im"]))

    def old(s):
        hr, _ = ops.mask_apply(s["mask"], ones, zeros, rows, Fn, Fs)
        ops.deepfilter_fwd(s["nre"], s["nim"], hr.view(B, T, Fs), zeros.view(B, T, Fs), td, fd, out=(s["old_re"], s["old_im"]))

    graphs = {}
    for name, fn in (("new", new), ("old", old)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for s in sets:                                               # warm-up: every set, outside the capture
                fn(s)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for s in sets:
                fn(s)
    same = all(torch.equal(s["new_re"].view(torch.int32), s["old_re"].view(torch.int32))
               and torch.equal(s["new_im"].view(torch.int32), s["old_im"].view(torch.int32)) for s in sets)
    for name in ("new", "old", "new", "old"):                            # warm replays
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {"new": [], "old": []}
    for _ in range(args.rounds):
        for name in ("old", "new"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[name].replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.sets)      # microseconds per call
    plane = rows * Fs * 4
    res = {"B": B, "T": T, "Fs": Fs, "Fn": Fn, "t_dim": td, "f_dim": fd, "device": torch.cuda.get_device_name(0), "sets": args.sets,
           "rounds": args.rounds, "timing": "HIP events around one graph replay of `sets` calls, old and new alternating; microseconds per call",
           "same_bits_at_this_shape": bool(same), "plane_bytes": plane}
    for name, planes in (("new", 5), ("old", 11)):
        t = np.asarray(times[name])
        res[name] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "q25_us": float(np.percentile(t, 25)),
                     "q75_us": float(np.percentile(t, 75)), "max_us": float(t.max()),
                     "planes_moved": planes - (1.0 - Fn / Fs)}             # (the mask has Fn of the Fs bins)
        res[name]["bytes"] = int(round(res[name]["planes_moved"] * plane))
        res[name]["tb_per_s_at_median"] = res[name]["bytes"] / (res[name]["median_us"] * 1e-6) / 1e12
    res["old_over_new_median"] = res["old"]["median_us"] / res["new"]["median_us"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
