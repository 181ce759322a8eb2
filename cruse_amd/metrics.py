"""Validation metrics on the device: the two closed-form entries of the reference's train_base/metrics.py.

    si_sdr(ref, est)            SI_SDR (:60-82), dB
    stoi(ref, est, sr=16000)    STOI (:85-86): the classic, non-extended measure as DESIGN.md section 13 defines it

Inputs are device tensors [B, L] or [L] (f32, 16 kHz for stoi); the result is a device tensor [B] (a 0-d tensor for [L]) and
nothing is read back, so a call can be captured into a HIP graph once its tables and workspace exist (they are made on the first call
for a device and shape, and kept).  A cached workspace is shared by every call of that shape: calls on different streams must be
ordered by the caller.

Deviations from the reference, recorded here and in DESIGN.md section 13:
  * WB_PESQ / NB_PESQ (an ITU reference program behind the `pesq` / `pypesq` packages) are not built; looking them up raises.
  * The reference's best-epoch score is (STOI + (WB_PESQ + 0.5) / 5) / 2 (base_trainer.py:370-376), which needs PESQ; the trainer
    here scores an epoch by the enhanced mean of ONE metric, [trainer.validation] score_metric.
  * pystoi is not installed where this was written: agreement with it is not claimed, only with the stated definition.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import ops

STOI_RATE = 16000
_TABLES: Dict[torch.device, torch.Tensor] = {}
_WORKSPACES: Dict[Tuple[torch.device, int, int], torch.Tensor] = {}


def _pair(ref: torch.Tensor, est: torch.Tensor, name: str):
    if not (isinstance(ref, torch.Tensor) and isinstance(est, torch.Tensor)):
        raise TypeError(f"{name}: expected two tensors")
    if ref.shape != est.shape:
        raise ValueError(f"{name}: ref {tuple(ref.shape)} and est {tuple(est.shape)} differ in shape")
    if ref.dim() not in (1, 2):
        raise ValueError(f"{name}: expected [B, L] or [L] waveforms, got {tuple(ref.shape)}")
    if ref.numel() == 0:
        raise ValueError(f"{name}: empty input {tuple(ref.shape)}")
    single = ref.dim() == 1
    ref2 = ref.reshape(1, -1) if single else ref
    est2 = est.reshape(1, -1) if single else est
    return ref2.float().contiguous(), est2.float().contiguous(), single


def si_sdr(ref: torch.Tensor, est: torch.Tensor) -> torch.Tensor:
    r, e, single = _pair(ref, est, "si_sdr")
    out = ops.si_sdr(r, e)
    return out[0] if single else out


def stoi(ref: torch.Tensor, est: torch.Tensor, sr: int = STOI_RATE) -> torch.Tensor:
    if sr != STOI_RATE:
        raise ValueError(f"stoi: sr must be {STOI_RATE} (the only rate built), got {sr!r}")
    r, e, single = _pair(ref, est, "stoi")
    dev = r.device
    tab = _TABLES.get(dev)
    if tab is None:
        tab = _TABLES[dev] = ops.stoi_tables(dev)
    key = (dev, r.shape[0], r.shape[1])
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = ops.stoi_workspace(r.shape[0], r.shape[1], dev)
    out = ops.stoi(r, e, tab, ws)
    return out[0] if single else out


class _Registry(dict):
    """REGISTERED_METRICS of train_base/metrics.py:129-135, less the PESQ entries, which say why they are missing"""

    def __missing__(self, name):
        if name in ("WB_PESQ", "NB_PESQ"):
            raise KeyError(f"{name}: PESQ is not built on this path (it is an ITU reference program, not closed-form signal processing); "
                           f"registered metrics: {sorted(self)}")
        raise KeyError(f"{name!r} is not a registered metric; registered metrics: {sorted(self)}")


REGISTERED_METRICS = _Registry({"SI_SDR": si_sdr, "STOI": stoi})
# the reference's spellings (train_base/metrics.py:60,85)
SI_SDR, STOI = si_sdr, stoi
