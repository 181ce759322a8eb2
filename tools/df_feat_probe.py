"""What DeepFilterNet's two input features cost on the fused kernel beside the torch composition they replace
-> profiles/df_feat_probe.json.

  kernel: ops.df_feat(re, im, starts, nb_df, alpha, erb_state, unit_state)                  one launch
  torch:  the reference module's loop on the device (ExponentialUnitNorm.forward, test/test_norm.py:52-61, restated here operation for
          operation), and for the ERB feature erb_apply of the band power, log10 and the same loop over the mean (test_erb.py:97-106 with
          the repair): a handful of small launches per frame
  frame:  the kernel on one frame, T = 1, with the state carried (the streaming call)

at B = 64, T = 401, F = 161, nb_erb = 32, nb_df = 96.  The kernel and the one-frame call are captured as graphs of `--sets` calls, one
per input set, and replayed between HIP events; the torch composition is timed eagerly between HIP events (its cost IS its launches),
after a warm-up, `--torch-rounds` times.  All three in one process.  Reported: median, minimum and quartiles per call, the kernel's
register and LDS figures (tools/kernel_resources.py), and the largest difference between the two results.  The times are a record, with
one condition that the tool checks: the kernel must not be slower than the torch composition.
usage: python tools/df_feat_probe.py [--batch 64] [--frames 401] [--sets 4] [--rounds 30] [--torch-rounds 5] [--out profiles/df_feat_probe.json]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def torch_composition(re, im, widths, nb_df, alpha, erb_state, unit_state):
    """-> feat_erb [B,T,nb_erb], feat_spec [B,T,nb_df,2]; the loops of the reference's scripts, on the device"""
    from cruse_amd.model.based_model.cust_conv import erb_apply
    T = re.shape[1]
    e = 10.0 * torch.log10(erb_apply(re.square() + im.square(), widths, True) + 1e-10)
    m, out = erb_state, []
    for t in range(T):
        m = e[:, t] * (1 - alpha) + alpha * m
        out.append((e[:, t] - m) / 40.0)
    feat_erb = torch.stack(out, 1)
    x = torch.stack([re[..., :nb_df], im[..., :nb_df]], dim=-1)
    x_abs = x.square().sum(dim=-1, keepdim=True).clamp_min(1e-14).sqrt()
    state, out_state = unit_state.unsqueeze(-1), []
    for t in range(T):
        state = x_abs[:, t] * (1 - alpha) + state * alpha
        out_state.append(state)
    return feat_erb, x / torch.stack(out_state, 1).sqrt()


def stats(t):
    t = np.asarray(t)
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "q25_us": float(np.percentile(t, 25)),
            "q75_us": float(np.percentile(t, 75)), "max_us": float(t.max())}


def resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, "cruse_amd", "csrc", "df_feat.hip"),
                          "df_feat_kernel"], capture_output=True, text=True).stdout.strip().splitlines()
    if len(out) < 2:
        return None
    v = out[-1].split()[-7:]
    return dict(zip(("vgpr", "agpr", "sgpr", "vgpr_spill", "scratch_bytes", "occupancy_waves_per_simd", "lds_bytes"), (int(x) for x in v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=401)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--torch-rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "df_feat_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("df_feat_probe: needs a HIP device (a time taken elsewhere says nothing)")
    from cruse_amd import ops
    from cruse_amd.acoustics import DfFeatures
    from cruse_amd.model.based_model.cust_conv import _band_table
    dev = torch.device("cuda", 0)
    B, T = args.batch, args.frames
    feat = DfFeatures()
    F, nb_erb, nb_df, alpha = feat.freq_bins, feat.nb_erb, feat.nb_df, feat.alpha
    starts = _band_table(feat.widths, dev)[0]
    g = torch.Generator(device=dev).manual_seed(5)
    sets = []
    for _ in range(args.sets):
        s = dict(re=0.3 * torch.randn(B, T, F, device=dev, generator=g), im=0.3 * torch.randn(B, T, F, device=dev, generator=g),
                 fe=torch.empty(B, T, nb_erb, device=dev), fs=torch.empty(B, T, nb_df, 2, device=dev),
                 fe1=torch.empty(B, 1, nb_erb, device=dev), fs1=torch.empty(B, 1, nb_df, 2, device=dev))
        s["state"] = feat.init_state(B, dev)
        sets.append(s)

    def kernel(s):
        ops.df_feat(s["re"], s["im"], starts, nb_df, alpha, erb_state=s["state"][0], unit_state=s["state"][1], out=(s["fe"], s["fs"]))

    def frame(s):
        ops.df_feat(s["re"][:, :1], s["im"][:, :1], starts, nb_df, alpha, erb_state=s["state"][0], unit_state=s["state"][1], out=(s["fe1"], s["fs1"]))

    graphs = {}
    for name, fn in (("kernel", kernel), ("frame", frame)):
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
    times = {"kernel": [], "frame": [], "torch": []}
    for name in ("kernel", "frame"):
        graphs[name].replay()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name in ("frame", "kernel"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[name].replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.sets)      # microseconds per call
    # the torch composition, eagerly: from the default states, as the kernel's accuracy comparison below
    s = sets[0]
    d_erb, d_unit = feat.init_state(B, dev)
    want = torch_composition(s["re"], s["im"], feat.widths, nb_df, alpha, d_erb, d_unit)      # warm-up
    torch.cuda.synchronize()
    for _ in range(args.torch_rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch_composition(s["re"], s["im"], feat.widths, nb_df, alpha, d_erb, d_unit)
        b.record()
        b.synchronize()
        times["torch"].append(a.elapsed_time(b) * 1e3)
    st = feat.init_state(B, dev)
    got = ops.df_feat(s["re"], s["im"], starts, nb_df, alpha, erb_state=st[0], unit_state=st[1])
    res = {"B": B, "T": T, "F": F, "nb_erb": nb_erb, "nb_df": nb_df, "alpha": alpha, "device": torch.cuda.get_device_name(0), "sets": args.sets,
           "rounds": args.rounds, "torch_rounds": args.torch_rounds,
           "timing": "kernel, frame: HIP events around one graph replay of `sets` calls, alternating; torch: HIP events around one eager "
                     "composition; microseconds per call",
           "kernel": stats(times["kernel"]), "frame_T1": stats(times["frame"]), "torch": stats(times["torch"]),
           "two_launch_variant": "not built: one launch only",
           "max_abs_diff_feat_erb_vs_torch": float((got[0] - want[0]).abs().max()),
           "max_rel_diff_feat_spec_vs_torch": float((got[1] - want[1]).abs().max() / want[1].abs().max()),
           "bytes_moved": 4 * B * T * (2 * F + nb_erb + 2 * nb_df), "kernel_resources": resources()}
    res["torch_over_kernel_median"] = res["torch"]["median_us"] / res["kernel"]["median_us"]
    res["gb_per_s_at_median"] = res["bytes_moved"] / (res["kernel"]["median_us"] * 1e-6) / 1e9
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if res["kernel"]["median_us"] > res["torch"]["median_us"]:
        raise SystemExit("df_feat_probe: the fused kernel is SLOWER than the torch composition at this shape: a defect")


if __name__ == "__main__":
    main()
