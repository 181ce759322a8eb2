"""Score a checkpoint on a list of paired WAV files (cruse_amd.evaluate.evaluate_files):

    python tools/evaluate.py --config cfg.toml --checkpoint runs/cfg/checkpoints/best_model.tar \\
        --clean-list clean.txt --noisy-list noisy.txt [--batch-size 16] [--metrics SI_SDR STOI ESTOI SDR] [--head df] [--post-filter iam] [--pf-tau 0.02]
        [--csv scores.csv]

The model is built from the config's [model] section as tools/train_stand.py builds it; the checkpoint is a *.tar of the trainer
(its "model" entry) or a bare state dict (model_NNNN.pth).  Prints one line per metric with the Noisy and Enhanced means."""
import argparse
import csv
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from train_base.utils import initialize_module  # noqa: E402
from tools.train_stand import load_toml  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(description="CRUSE on MI355X: metric scores of a checkpoint on paired files")
    parser.add_argument("--config", required=True, help="Configuration (*.toml): [model] and [acoustics] are read.")
    parser.add_argument("--checkpoint", required=True, help="best_model.tar / latest_model.tar / model_NNNN.pth")
    parser.add_argument("--clean-list", required=True, help="List file: one clean WAV path per line.")
    parser.add_argument("--noisy-list", required=True, help="List file: the noisy WAV of the same line.")
    parser.add_argument("--batch-size", type=int, default=16)
    parser.add_argument("--metrics", nargs="+", default=["SI_SDR", "STOI", "ESTOI"])
    parser.add_argument("--head", choices=["mask", "df"], default="mask",
                        help="How the network output is applied: mask (magnitude mask) or df (DeepFilter(1, 5) head: a model trained "
                             "with wo_male_df_loss, configs/cruse_deepfilter.toml).")
    parser.add_argument("--post-filter", choices=["iam", "envelope"], default=None,
                        help="The reference's perceptual post-filter on the mask (postfiltering / envelope_postfiltering); off by default.")
    parser.add_argument("--pf-tau", type=float, default=0.02, help="The post-filter's tau (the reference's default 0.02).")
    parser.add_argument("--csv", help="Write the per-file table here.")
    args = parser.parse_args(argv)
    from cruse_amd.evaluate import evaluate_files
    config = load_toml(args.config)
    model = initialize_module(config["model"]["path"], args=config["model"]["args"])
    ck = torch.load(os.path.abspath(os.path.expanduser(args.checkpoint)), map_location="cpu", weights_only=False)
    model.load_state_dict(ck["model"] if "model" in ck else ck)
    res = evaluate_files(model, args.clean_list, args.noisy_list, metrics=args.metrics, batch_size=args.batch_size,
                         acoustics=config.get("acoustics"), head=args.head, post_filter=args.post_filter, pf_tau=args.pf_tau)
    for name, m in res["mean"].items():
        print(f"{name}: Noisy {m['Noisy']!r}  Enhanced {m['Enhanced']!r}")
    if args.csv:
        with open(args.csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["name", "length"] + [f"{name}_{side}" for name in res["scores"] for side in ("Noisy", "Enhanced")])
            for i, name in enumerate(res["names"]):
                w.writerow([name, int(res["lengths"][i])] + [repr(float(res["scores"][m][side][i])) for m in res["scores"]
                                                             for side in ("Noisy", "Enhanced")])
    return res


if __name__ == "__main__":
    main()
