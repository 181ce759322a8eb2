"""What the on-device EQ augmentation costs -> profiles/aug_probe.json:
  kernel        cruse_biquad_cascade alone, HIP events, B = 64, L = 64000, S = 4: microseconds and 2 B L 4 bytes over that time
  device_batch  one DevicePairs.device_batch (gather + [filters] + snr_mix) with and without the augmentation
  epoch         Trainer._train_epoch as bench.py's trainer_path row drives it, on the [train_dataset] sections of
                configs/cruse_augment.toml and configs/cruse_device_dataset.toml in one process: frames/s (the better of epochs 2-3) and
                the ratio augmented / plain
usage: python tools/aug_probe.py [--batches 120] [--out profiles/aug_probe.json]
With --reverb the same three rows for the reverberation -> profiles/aug_probe_reverb.json:
  kernel        cruse_fftconv_apply (with and without y_early) and cruse_fftconv_prepare at B = 64, L = 64000, R = 8000, with a bank of 32
                filters behind an index and with a filter per clip, and cruse_fir_causal on the same tensors in the same run
  device_batch  plain, reverb only, reverb + EQ
  epoch         configs/cruse_reverb.toml against configs/cruse_device_dataset.toml
With --files DIR the file-list dataset -> profiles/aug_probe_files.json: a small synthetic corpus of WAVs at mixed
rates is written into DIR, then
  kernel        cruse_resample_poly alone, 64 clips x 10 s of int16 mono from 44.1 kHz and from 48 kHz
  preload       DeviceFilePairs' first _ensure: wall time, and per (rate, channels) group the seconds of file reading and of device work
  device_batch  DeviceFilePairs.device_batch beside DevicePairs.device_batch at the same B x length (64 x 4 s), in windows interleaved
                P, N, P, N
Each row is its own process under its own time limit (--row kernel | device_batch | epoch, merged into --out); without --row the
rows run as child processes, one after the other, and the first that fails ends the run."""
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


def timed_us(fn, warm=5, n=50):
    """median and minimum of n event-timed calls, microseconds"""
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
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(min(ts))


def kernel_row(dev, B=64, L=64000, S=4):
    from cruse_amd import ops
    from cruse_amd.acoustics import audio_aug as A
    from cruse_amd.data import synth_batch
    rng = np.random.default_rng(0)
    coef = torch.from_numpy(np.concatenate([A.draw_sec_filters(B, S - 1, rng=rng), A.draw_hp_filters(B, 1, rng=rng)], axis=1)).to(dev)
    _, x = synth_batch(B, L, dev, 3)
    y = torch.empty_like(x)
    out = {"B": B, "L": L, "S": S, "bytes": 2 * B * L * 4}
    for clamp in (False, True):
        med, best = timed_us(lambda: ops.biquad_cascade(x, coef, clamp=clamp, out=y))
        out["clamp" if clamp else "no_clamp"] = {"median_us": round(med, 2), "min_us": round(best, 2), "GB_per_s": round(out["bytes"] / med / 1e3, 1)}
    return out


def reverb_kernel_row(dev, B=64, L=64000, R=8000, NR=32):
    from cruse_amd import ops
    from cruse_amd.data import fir_causal, rir_early_len, synth_batch, synth_rirs
    g = torch.Generator(device=dev).manual_seed(1)
    _, x = synth_batch(B, L, dev, 3)
    y, ye = torch.empty_like(x), torch.empty_like(x)
    out = {"B": B, "L": L, "R": R, "partition": ops.FFTCONV_PART}
    row = lambda t: {"median_us": round(t[0], 1), "min_us": round(t[1], 1)}
    for name, n in (("pool_indexed", NR), ("per_clip", B)):
        h = synth_rirs(n, R, 0.2, 0.8, 16000, dev, g)
        early = rir_early_len(h)
        idx = (torch.arange(B, device=dev) % n).to(torch.int32) if n != B else None
        bank = ops.fft_conv_prepare(h, early)
        spec = bank.spec
        r = {"NR": n, "prepare_with_early": row(timed_us(lambda: ops.fft_conv_prepare(h, early, spec=spec), n=20)),
             "apply": row(timed_us(lambda: ops.fft_conv_apply(x, bank, h_index=idx, out=y), n=30)),
             "apply_with_early": row(timed_us(lambda: ops.fft_conv_apply(x, bank, h_index=idx, want_early=True, out=y, out_early=ye), n=30))}
        hb = h if n == B else h.index_select(0, idx.long()).contiguous()
        r["fir_causal"] = row(timed_us(lambda: fir_causal(x, hb), warm=2, n=8))
        r["fir_over_fft"] = round(r["fir_causal"]["median_us"] / r["apply"]["median_us"], 1)
        r["rel_l2_fft_vs_fir"] = float((y - fir_causal(x, hb)).double().norm() / fir_causal(x, hb).double().norm())
        out[name] = r
    return out


def reverb_device_batch_row(dev, args, B):
    from cruse_amd.data import DevicePairs
    rev = {k: args[k] for k in ("reverb_proportion", "reverb_noise_proportion", "reverb_target")}
    base = {k: v for k, v in args.items() if k not in rev}
    out = {}
    for name, extra in (("plain", {}), ("reverb", rev), ("reverb_eq", dict(rev, eq_prob=0.5, eq_filters=3, hp_prob=0.5))):
        ds = DevicePairs(**base, **extra)
        idx = torch.arange(B)
        med, best = timed_us(lambda: ds.device_batch(idx, dev), warm=8, n=40)
        out[name] = {"median_us": round(med, 1), "min_us": round(best, 1)}
    return out


def device_batch_row(dev, args, B):
    from cruse_amd.data import DevicePairs
    out = {}
    for name, extra in (("plain", {}), ("augmented", {k: args[k] for k in ("eq_prob", "eq_filters", "hp_prob")})):
        ds = DevicePairs(**{k: v for k, v in args.items() if k not in ("eq_prob", "eq_filters", "hp_prob")}, **extra)
        idx = torch.arange(B)
        med, best = timed_us(lambda: ds.device_batch(idx, dev), warm=8, n=40)
        out[name] = {"median_us": round(med, 1), "min_us": round(best, 1)}
    return out


def epoch_row(dev, conf, nb, save_dir):
    import contextlib
    import io
    from torch.utils.data import DataLoader, DistributedSampler
    import train_base.loss as L
    from cruse_amd.data import DevicePairs
    from cruse_amd.model.cruse_net import unet_2
    from cruse_amd.train.trainer_casual import Trainer
    B = conf["train_dataset"]["dataloader"]["batch_size"]
    ds = DevicePairs(**dict(conf["train_dataset"]["args"], num=nb * B))
    torch.manual_seed(0)
    m = unet_2(**conf["model"]["args"])
    cfg = {"acoustics": conf["acoustics"], "trainer": {"train": {"epochs": 3, "clip_grad_norm_value": conf["trainer"]["train"]["clip_grad_norm_value"]}},
           "meta": {"save_dir": save_dir, "precision": conf["meta"]["precision"], "hip_graph": "auto"}}
    loader = DataLoader(dataset=ds, sampler=DistributedSampler(dataset=ds, num_replicas=1, rank=0, shuffle=True), shuffle=False, batch_size=B,
                        drop_last=True, num_workers=0)
    tr = Trainer(dist=None, rank=0, config=cfg, resume=False, only_validation=False, model=m, loss_function=L.wo_male_loss(**conf["loss_function"]["args"]),
                 optimizer=torch.optim.Adam(m.parameters(), lr=conf["optimizer"]["lr"]), train_dataloader=loader, validation_dataloader=None)
    fps, losses = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        for ep in (1, 2, 3):
            losses.append(float(tr._train_epoch(ep)))
            fps.append(tr.last_epoch_frames_per_s)
    return {"frames_per_s": round(max(fps[1:]), 1), "epochs_frames_per_s": [round(f, 1) for f in fps], "epoch_losses": [round(v, 6) for v in losses],
            "batches_per_epoch": nb, "skipped_steps": int(tr.engine.skipped_steps()), "timeout_steps": int(tr.engine.timeout_steps()),
            "nonfinite_steps": int(tr.engine.nonfinite_steps())}


def write_probe_corpus(root, seed=0):
    """48 speech-like, 16 noise and 4 RIR files of 16-bit PCM at mixed rates (one group stereo) -> the three list files"""
    import wave
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    lists = {}
    for name, n, (lo, hi) in (("clean", 48, (2.0, 6.0)), ("noise", 16, (3.0, 8.0)), ("rir", 4, (0.4, 0.5))):
        paths = []
        for k in range(n):
            rate, ch = ((16000, 1), (8000, 1), (44100, 1), (48000, 2), (22050, 1))[k % 5]
            m = int(rng.uniform(lo, hi) * rate)
            t = np.arange(m) / rate
            if name == "rir":
                x = 0.2 * rng.standard_normal(m) * np.exp(-t / 0.08)
                x[0] = 0.9
            else:
                f0 = rng.uniform(90, 280)
                x = sum(np.sin(2 * np.pi * f0 * (j + 1) * t + rng.uniform(0, 6.28)) / (j + 1) for j in range(8)) * (name == "clean") + 0.3 * rng.standard_normal(m)
            pcm = np.clip(np.rint(0.8 * x / np.abs(x).max() * 32767), -32768, 32767).astype(np.int16)
            path = os.path.join(root, f"{name}_{k:03d}.wav")
            with wave.open(path, "wb") as w:
                w.setnchannels(ch)
                w.setsampwidth(2)
                w.setframerate(rate)
                w.writeframes(np.repeat(pcm, ch).tobytes())
            paths.append(path)
        lists[name] = os.path.join(root, name + ".lst")
        with open(lists[name], "w") as f:
            f.write("\n".join(paths) + "\n")
    return lists


def files_main(a):
    import time
    from cruse_amd import ops
    from cruse_amd import resample_design as D
    from cruse_amd.data import DevicePairs
    from cruse_amd.filepairs import DeviceFilePairs
    assert torch.cuda.is_available(), "aug_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = a.out if a.out != os.path.join(ROOT, "profiles", "aug_probe.json") else os.path.join(ROOT, "profiles", "aug_probe_files.json")
    res = {"device": torch.cuda.get_device_name(0)}
    kern = {}
    for rate in (44100, 48000):                    # 64 clips x 10 s
        up, down = D.ratio(16000, rate)
        B, L = 64, 10 * rate
        src = torch.randint(-20000, 20000, (B * L,), device=dev, dtype=torch.int16)
        off_in = np.arange(B + 1, dtype=np.int64) * L
        off_out = np.arange(B + 1, dtype=np.int64) * D.out_len(L, up, down)
        y = torch.empty(int(off_out[-1]), device=dev)
        di, do = torch.from_numpy(off_in).to(dev), torch.from_numpy(off_out).to(dev)
        med, best = timed_us(lambda: ops.resample_poly(src, off_in, off_out, up, down, y, off_in_dev=di, off_out_dev=do), n=30)
        T = D.taps_per_phase(up, down)
        kern[str(rate)] = {"B": B, "seconds_per_clip": 10, "up": up, "down": down, "taps_per_output": T, "median_us": round(med, 1), "min_us": round(best, 1),
                           "outputs": int(off_out[-1]), "GFMA_per_s": round(int(off_out[-1]) * T / med / 1e3, 1),
                           "bytes": int(B * L * 2 + off_out[-1] * 4), "GB_per_s": round((B * L * 2 + int(off_out[-1]) * 4) / med / 1e3, 1)}
    res["kernel"] = kern
    print(json.dumps({"kernel": kern}), flush=True)
    lists = write_probe_corpus(a.files)
    B, sec = 64, 4.0
    ds = DeviceFilePairs(clean_dataset=lists["clean"], noise_dataset=lists["noise"], rir_dataset=lists["rir"], snr_range=[0, 20], silence_length=0.2,
                         sub_sample_length=sec, dataset_length=2048, seed=1)
    t0 = time.perf_counter()
    ds._ensure(dev)
    torch.cuda.synchronize()
    res["preload"] = {"wall_s": round(time.perf_counter() - t0, 4),
                      "groups": [dict(r, read_s=round(r["read_s"], 5), device_s=round(r["device_s"], 5)) for r in ds.preload_stats]}
    print(json.dumps({"preload": res["preload"]}), flush=True)
    parent = DevicePairs(num=2048, length=int(sec * 16000), seed=1, pool=128)
    idx = torch.arange(B)

    def window(d, k=30):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for j in range(k):
            d.device_batch((idx + j * B) % 2048, dev)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / k * 1e6

    for d in (parent, ds):
        window(d, 8)                               # warm: pools, pinned slots, code objects
    wins = {"P": [], "N": []}
    for _ in range(4):                             # P, N, P, N ...
        wins["P"].append(window(parent))
        wins["N"].append(window(ds))
    res["device_batch"] = {"B": B, "length": int(sec * 16000), "parent_us": [round(v, 1) for v in wins["P"]], "files_us": [round(v, 1) for v in wins["N"]],
                           "parent_median_us": round(float(np.median(wins["P"])), 1), "files_median_us": round(float(np.median(wins["N"])), 1),
                           "segments_last_batch": [int(ds.last_plan[0].shape[0]), int(ds.last_plan[2].shape[0])]}
    print(json.dumps({"device_batch": res["device_batch"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_probe.json"))
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--reverb", action="store_true")
    ap.add_argument("--row", choices=("kernel", "device_batch", "epoch"))
    ap.add_argument("--files", metavar="DIR", help="probe the file-list dataset on a synthetic corpus written into DIR")
    a = ap.parse_args()
    if a.files:
        return files_main(a)
    if a.reverb:
        return reverb_main(a)
    from tools.train_stand import load_toml
    assert torch.cuda.is_available(), "aug_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    aug = load_toml(os.path.join(ROOT, "configs", "cruse_augment.toml"))
    plain = load_toml(os.path.join(ROOT, "configs", "cruse_device_dataset.toml"))
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_row(dev)}
    print(json.dumps({"kernel": res["kernel"]}), flush=True)
    res["device_batch"] = device_batch_row(dev, aug["train_dataset"]["args"], aug["train_dataset"]["dataloader"]["batch_size"])
    print(json.dumps({"device_batch": res["device_batch"]}), flush=True)
    if not a.skip_epoch:
        import tempfile
        with tempfile.TemporaryDirectory(prefix="cruse_aug_probe_") as tmp:
            ep = {"plain": epoch_row(dev, plain, a.batches, tmp), "augmented": epoch_row(dev, aug, a.batches, tmp)}
        ep["ratio_augmented_to_plain"] = round(ep["augmented"]["frames_per_s"] / ep["plain"]["frames_per_s"], 4)
        res["epoch"] = ep
        print(json.dumps({"epoch": ep}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


ROW_LIMIT_S = {"kernel": 240, "device_batch": 180, "epoch": 900}


def reverb_main(a):
    out = a.out if a.out != os.path.join(ROOT, "profiles", "aug_probe.json") else os.path.join(ROOT, "profiles", "aug_probe_reverb.json")
    if a.row is None:                             # every row a fresh process under its own limit; a failure ends the run
        import subprocess
        rows = ("kernel", "device_batch") + (() if a.skip_epoch else ("epoch",))
        for row in rows:
            cmd = ["timeout", "-k", "10", str(ROW_LIMIT_S[row]), sys.executable, os.path.abspath(__file__), "--reverb", "--row", row, "--batches",
                   str(a.batches), "--out", out]
            rc = subprocess.call(cmd)
            if rc != 0:
                sys.exit(f"aug_probe --reverb: row {row} ended with status {rc}; nothing more is started")
        return
    from tools.train_stand import load_toml
    assert torch.cuda.is_available(), "aug_probe needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rev = load_toml(os.path.join(ROOT, "configs", "cruse_reverb.toml"))
    plain = load_toml(os.path.join(ROOT, "configs", "cruse_device_dataset.toml"))
    if a.row == "kernel":
        val = reverb_kernel_row(dev)
    elif a.row == "device_batch":
        val = reverb_device_batch_row(dev, rev["train_dataset"]["args"], rev["train_dataset"]["dataloader"]["batch_size"])
    else:
        import tempfile
        with tempfile.TemporaryDirectory(prefix="cruse_aug_probe_") as tmp:
            val = {"plain": epoch_row(dev, plain, a.batches, tmp), "reverb": epoch_row(dev, rev, a.batches, tmp)}
        val["ratio_reverb_to_plain"] = round(val["reverb"]["frames_per_s"] / val["plain"]["frames_per_s"], 4)
    print(json.dumps({a.row: val}), flush=True)
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    res[a.row] = val
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
