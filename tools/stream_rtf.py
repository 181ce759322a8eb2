"""Real-time factor of frame-by-frame streaming inference (cruse_amd.inferencer.StreamingInferencer) on one GPU.

For each n_slots: host wall time of one push (160 new samples for every slot) measured around a device synchronise after warm-up,
over >= `--seconds` of pushes (mean / p50 / p99), device time per hop from events around the push, and RTF = push time / 10 ms
(one hop at 16 kHz).  Prints one JSON object.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/stream_rtf.py`.

With --hops (e.g. 1,2,4,8) every (n_slots, hops) cell is measured: wall time per call and per hop (call / hops), device time per
hop and RTF = call time / (hops * 10 ms).  The hops = 1 row goes through the unchanged push, hops > 1 through push_packet on an
instance built with max_hops = hops; --out writes the JSON to a file as well (profiles/stream_packet_rtf.json).

With --precision f32,f16 every cell is measured for both modes of StreamingInferencer in the same process, f32 first; every row then
carries "precision", and f16 rows "vs_f32" = their wall time per hop over the f32 row's of the same cell (profiles/stream_f16_rtf.json).
The default, f32 alone, prints what it always printed.

With --pcm the instances are built with pcm_in = pcm_out = True and fed int16 blocks; with --atten-lim DB they are built with
atten_lim = True and every slot limited to DB dB.  Either adds "io" to the result; without them nothing changes (DESIGN 12c,
profiles/stream_io_rtf.json).

With --io-rate 16000,48000,... every cell is measured once per rate (StreamingInferencer(io_rate=...): blocks of rate / 100 samples
through the rate-conversion kernels; a hop is still 10 ms) and every row carries "io_rate"; without it nothing changes (DESIGN 12d,
profiles/stream_rs_rtf.json).

With --head mask,df every (n_slots, hops) cell is measured for both heads of StreamingInferencer in one run: one instance
each, in alternating slices of the measuring time; every row carries "head", the df row "vs_mask" (p50 wall time per hop over the mask
row's) and "device_vs_mask" (profiles/stream_df_rtf.json).

With --post-filter none,iam every (n_slots, hops) cell is measured with and without the perceptual post-filter in one
run, in the style of --head: one instance each (the filtered one with every slot's tau = --pf-tau, default 0.02), alternating slices;
every row carries "post_filter", the filtered rows "vs_none" and "device_vs_none".

With --model unet_2,cruse4 every (n_slots, hops) cell is measured for both decoders in one run, in the style of --head: unet_2 (ConvTranspose
levels, decoder="transposed") and CRUSE4MagAddSkipUpsample with the same channels and groups (FreqUpsample + Conv2d levels,
decoder="upsample"), one instance each, alternating slices; every row carries "model", the cruse4 row "vs_unet_2" and
"device_vs_unet_2" (profiles/stream_up_rtf.json).  --model cruse4 alone measures that model through every other option.

With --meters off,on every (n_slots, hops) cell is measured without and with the level meters and voice-activity detector (meters=True:
one more kernel per chain) in one run, in the style of --head: one instance each, alternating slices; every row carries
"meters", the "on" row "vs_off" and "device_vs_off" (profiles/stream_meter_rtf.json).

    python tools/stream_rtf.py [--slots 1,16,64,256,1024] [--seconds 2] [--groups 4] [--hops 1,2,4,8] [--precision f32,f16] [--pcm]
                               [--atten-lim DB] [--io-rate 16000,8000,48000] [--head mask,df]
                               [--post-filter none,iam] [--pf-tau 0.02] [--model unet_2,cruse4] [--meters off,on] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def closed_form(model):
    """deterministic weights (the oracle's closed_form_init formula) without importing the test oracle"""
    import math
    with torch.no_grad():
        for i, (name, p) in enumerate(model.named_parameters()):
            j = torch.arange(p.numel(), dtype=torch.float64)
            s = torch.sin(0.37 * j + 1.3 * i + 0.1)
            is_norm = ".ln" in name or "bn" in name or ".norm." in name or (name.startswith("enc") and ".2." in name)
            if is_norm:
                v = 1.0 + 0.1 * s if name.endswith("weight") else 0.05 * s
            else:
                v = s / math.sqrt(max(p[0].numel() if p.dim() > 1 else p.numel(), 1))
            p.copy_(v.reshape(p.shape).to(p.dtype))


IO = {"pcm": False, "atten_lim": None, "io_rate": None}      # --pcm / --atten-lim / --io-rate: the I/O mode of every instance measured
MODELS = {"unet_2": "transposed", "cruse4": "upsample"}      # --model: the StreamingInferencer decoder each name runs on


def build_model(name: str, groups: int):
    """the product module of --model `name` with deterministic weights, on the device"""
    if name == "cruse4":
        from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
        m = CRUSE4MagAddSkipUpsample(rnn_groups=groups, precision="f32")
    else:
        from cruse_amd.model.cruse_net import unet_2
        m = unet_2(rnn_groups=groups, precision="f32")
    closed_form(m)
    return m.cuda().eval()


def _inferencer(model, S: int, precision: str, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    if type(model).__name__ == "CRUSE4MagAddSkipUpsample":
        kw.update(decoder="upsample")
    if IO["pcm"]:
        kw.update(pcm_in=True, pcm_out=True)
    if IO["atten_lim"] is not None:
        kw.update(atten_lim=True)
    if IO["io_rate"] is not None:
        kw.update(io_rate=IO["io_rate"])
    inf = StreamingInferencer(model, S, **kw) if precision == "f32" else StreamingInferencer(model, S, precision=precision, **kw)
    if IO["atten_lim"] is not None:
        inf.set_atten_lim(IO["atten_lim"])
    return inf


def _blocks(*shape):
    """0.1 * randn blocks (`shape` ends in 160: a block, io_rate / 100 samples with --io-rate), as int16 PCM with --pcm"""
    if IO["io_rate"] is not None:
        shape = shape[:-1] + (IO["io_rate"] // 100,)
    x = 0.1 * torch.randn(*shape, device="cuda")
    return (x * 32768.0).round().clamp(-32768, 32767).to(torch.int16) if IO["pcm"] else x


def measure(model, S: int, seconds: float, precision: str = "f32"):
    inf = _inferencer(model, S, precision)
    blocks = _blocks(S, 160)
    for _ in range(50):
        inf.push(blocks)
    torch.cuda.synchronize()
    walls, devs = [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(walls) < 200:
        t0 = time.perf_counter()
        ev0.record()
        inf.push(blocks)
        ev1.record()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        devs.append(ev0.elapsed_time(ev1) * 1e-3)
    w, d = np.array(walls) * 1e6, np.array(devs) * 1e6
    return {"n_slots": S, "pushes": len(walls), "push_wall_us": {"mean": round(float(w.mean()), 2), "p50": round(float(np.median(w)), 2),
            "p99": round(float(np.percentile(w, 99)), 2)}, "device_us_per_hop": round(float(d.mean()), 2),
            "rtf": round(float(w.mean()) / 10000.0, 5), "rtf_per_stream": round(float(w.mean()) / 10000.0 / S, 8)}


def measure_packets(model, S: int, hops: int, seconds: float, precision: str = "f32"):
    """one (n_slots, hops) cell; hops = 1 is the single-hop push chain"""
    inf = _inferencer(model, S, precision, max_hops=hops)
    blocks = _blocks(S, hops, 160)
    call = (lambda: inf.push(blocks[:, 0])) if hops == 1 else (lambda: inf.push_packet(blocks))
    for _ in range(50):
        call()
    torch.cuda.synchronize()
    walls, devs = [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(walls) < 200:
        t0 = time.perf_counter()
        ev0.record()
        call()
        ev1.record()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        devs.append(ev0.elapsed_time(ev1) * 1e-3)
    w, d = np.array(walls) * 1e6, np.array(devs) * 1e6
    r = lambda v: round(float(v), 2)
    return {"n_slots": S, "hops": hops, "path": "push" if hops == 1 else "push_packet", "calls": len(walls),
            "call_wall_us": {"mean": r(w.mean()), "p50": r(np.median(w)), "p99": r(np.percentile(w, 99))},
            "wall_us_per_hop": {"mean": r(w.mean() / hops), "p50": r(np.median(w) / hops), "p99": r(np.percentile(w, 99) / hops)},
            "device_us_per_hop": r(d.mean() / hops), "rtf": round(float(w.mean()) / (10000.0 * hops), 5)}


def _variant(model, S, precision, hops, key, h, pf_tau):
    """the instance of one side-by-side variant: a head, or a post-filter setting ("none": the plain server)"""
    if key == "head":
        return _inferencer(model, S, precision, max_hops=hops, head=h)
    if key == "model":
        return _inferencer(model[h], S, precision, max_hops=hops)
    if key == "meters":
        return _inferencer(model, S, precision, max_hops=hops, **({"meters": True} if h == "on" else {}))
    inf = _inferencer(model, S, precision, max_hops=hops, post_filter=None if h == "none" else h)
    if h != "none":
        inf.set_post_filter(pf_tau)
    return inf


def measure_heads(model, S: int, hops: int, seconds: float, heads, precision: str = "f32", rounds: int = 8, key: str = "head",
                  base_name: str = "mask", pf_tau: float = 0.02):
    """one (n_slots, hops) cell for every head in `heads`, side by side: one instance per head, measured in `rounds` alternating slices of
    seconds / rounds each, so that clock and machine drift hit both alike.  Rows as measure_packets, plus "head" and, on the "df" row,
    "vs_mask" = its wall time per hop over the mask row's.  key = "post_filter", base_name = "none": the same for the post-filter settings."""
    infs = {h: _variant(model, S, precision, hops, key, h, pf_tau) for h in heads}
    blocks = _blocks(S, hops, 160)
    calls = {h: ((lambda i=i: i.push(blocks[:, 0])) if hops == 1 else (lambda i=i: i.push_packet(blocks))) for h, i in infs.items()}
    for call in calls.values():
        for _ in range(50):
            call()
    torch.cuda.synchronize()
    walls, devs = {h: [] for h in heads}, {h: [] for h in heads}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for h in heads:
            t_end = time.perf_counter() + seconds / rounds
            n0 = len(walls[h])
            while time.perf_counter() < t_end or len(walls[h]) - n0 < 50:
                t0 = time.perf_counter()
                ev0.record()
                calls[h]()
                ev1.record()
                torch.cuda.synchronize()
                walls[h].append(time.perf_counter() - t0)
                devs[h].append(ev0.elapsed_time(ev1) * 1e-3)
    r = lambda v: round(float(v), 2)
    rows = []
    for h in heads:
        w, d = np.array(walls[h]) * 1e6, np.array(devs[h]) * 1e6
        rows.append({"n_slots": S, "hops": hops, key: h, "path": "push" if hops == 1 else "push_packet", "calls": len(w),
                     "wall_us_per_hop": {"mean": r(w.mean() / hops), "p50": r(np.median(w) / hops), "p99": r(np.percentile(w, 99) / hops)},
                     "device_us_per_hop": r(d.mean() / hops), "rtf": round(float(w.mean()) / (10000.0 * hops), 5)})
    base = {row[key]: row for row in rows}.get(base_name)
    for row in rows:
        if base is not None and row[key] != base_name:
            row[f"vs_{base_name}"] = round(row["wall_us_per_hop"]["p50"] / base["wall_us_per_hop"]["p50"], 3)
            row[f"device_vs_{base_name}"] = round(row["device_us_per_hop"] / base["device_us_per_hop"], 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,16,64,256,1024")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--hops", default=None, help="comma-separated packet sizes, e.g. 1,2,4,8: measure every (slots, hops) cell")
    ap.add_argument("--precision", default="f32", help="f32 (default), f16 or f32,f16: the StreamingInferencer modes to measure")
    ap.add_argument("--pcm", action="store_true", help="int16 PCM blocks in and out (pcm_in = pcm_out = True)")
    ap.add_argument("--atten-lim", type=float, default=None, metavar="DB", help="every slot limited to DB dB of attenuation (atten_lim = True)")
    ap.add_argument("--io-rate", default=None, help="comma-separated I/O sample rates (8000, 16000, 32000, 48000): measure every cell at each")
    ap.add_argument("--head", default=None, help="mask, df or mask,df: the heads to measure side by side, alternating, in every cell")
    ap.add_argument("--post-filter", default=None, help="none, iam, envelope or a list (none,iam): measured side by side like --head")
    ap.add_argument("--pf-tau", type=float, default=0.02, help="tau of every slot of the post-filter instances")
    ap.add_argument("--model", default="unet_2", help="unet_2 (default), cruse4, or unet_2,cruse4: the two decoders side by side like --head")
    ap.add_argument("--meters", default=None, help="off, on or off,on: without / with the level meters, side by side like --head")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    IO.update(pcm=a.pcm, atten_lim=a.atten_lim)
    rates = [None] if a.io_rate is None else [int(r) for r in a.io_rate.split(",")]
    names = a.model.split(",")
    if any(n not in MODELS for n in names) or len(set(names)) != len(names):
        ap.error(f"--model takes unet_2, cruse4 or unet_2,cruse4, got {a.model}")
    torch.manual_seed(0)
    built = {n: build_model(n, a.groups) for n in names}
    m = built[names[0]]
    precs = a.precision.split(",")
    if any(p not in ("f32", "f16") for p in precs):
        ap.error(f"--precision takes f32, f16 or f32,f16, got {a.precision}")
    rows = []
    heads = None if a.head is None else a.head.split(",")
    side = dict(key="head", base_name="mask")
    if a.post_filter is not None:
        if heads is not None:
            ap.error("--head and --post-filter are measured in runs of their own")
        heads = a.post_filter.split(",")
        if any(h not in ("none", "iam", "envelope") for h in heads):
            ap.error(f"--post-filter takes none, iam, envelope or a list of them, got {a.post_filter}")
        side = dict(key="post_filter", base_name="none", pf_tau=a.pf_tau)
    elif heads is not None and any(h not in ("mask", "df") for h in heads):
        ap.error(f"--head takes mask, df or mask,df, got {a.head}")
    if a.meters is not None:
        if heads is not None:
            ap.error("--meters is measured in a run of its own (no --head / --post-filter)")
        heads = a.meters.split(",")
        if any(h not in ("off", "on") for h in heads):
            ap.error(f"--meters takes off, on or off,on, got {a.meters}")
        side = dict(key="meters", base_name="off")
    if len(names) > 1:
        if heads is not None:
            ap.error("--model with two models is measured in a run of its own (no --head / --post-filter / --meters)")
        heads, side, m = names, dict(key="model", base_name="unet_2"), built
    if heads is not None:
        for prec in precs:
            for s in a.slots.split(","):
                for h in (a.hops or "1").split(","):
                    part = measure_heads(m, int(s), int(h), a.seconds, heads, prec, **side)
                    for r in part:
                        if precs != ["f32"]:
                            r["precision"] = prec
                    rows += part
        rates = []
    for rate in rates:
        IO.update(io_rate=rate)
        for prec in precs:
            if a.hops is None:
                part = [measure(m, int(s), a.seconds, prec) for s in a.slots.split(",")]
            else:
                part = [measure_packets(m, int(s), int(h), a.seconds, prec) for s in a.slots.split(",") for h in a.hops.split(",")]
                base = {r["n_slots"]: r["wall_us_per_hop"]["mean"] for r in part if r["hops"] == 1}
                for r in part:                                      # per hop against the push path of the same mode and run
                    if r["n_slots"] in base:
                        r["per_hop_vs_push"] = round(r["wall_us_per_hop"]["mean"] / base[r["n_slots"]], 3)
            for r in part:
                if precs != ["f32"]:
                    r["precision"] = prec
                if rate is not None:
                    r["io_rate"] = rate
            rows += part
    if "f32" in precs and "f16" in precs:
        per_hop = lambda r: r["wall_us_per_hop"]["mean"] if "wall_us_per_hop" in r else r["push_wall_us"]["mean"]
        cell = lambda r: (r["n_slots"], r.get("hops", 1), r.get("io_rate"))
        f32 = {cell(r): per_hop(r) for r in rows if r["precision"] == "f32"}
        for r in rows:
            if r["precision"] == "f16":
                r["vs_f32"] = round(per_hop(r) / f32[cell(r)], 3)
    res = {"model": f"{'+'.join(names)} ch={built[names[0]].ch} rnn_groups={a.groups}", "device": torch.cuda.get_device_name(0), "rows": rows}
    if a.pcm or a.atten_lim is not None:
        res["io"] = {"pcm": a.pcm, "atten_lim_db": a.atten_lim}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
