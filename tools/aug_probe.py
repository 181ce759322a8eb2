"""What the on-device EQ augmentation costs -> profiles/aug_probe.json:
  kernel        cruse_biquad_cascade alone, HIP events, B = 64, L = 64000, S = 4: microseconds and 2 B L 4 bytes over that time
  device_batch  one DevicePairs.device_batch (gather + [filters] + snr_mix) with and without the augmentation
  epoch         Trainer._train_epoch as bench.py's trainer_path row drives it, on the [train_dataset] sections of
                configs/cruse_augment.toml and configs/cruse_device_dataset.toml in one process: frames/s (the better of epochs 2-3) and
                the ratio augmented / plain
usage: python tools/aug_probe.py [--batches 120] [--out profiles/aug_probe.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_probe.json"))
    ap.add_argument("--skip-epoch", action="store_true")
    a = ap.parse_args()
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


if __name__ == "__main__":
    main()
