"""Validation metrics on the device: the closed-form entries of the reference's train_base/metrics.py.

    si_sdr(ref, est)            SI_SDR (:60-82), dB
    stoi(ref, est, sr=16000)    STOI (:85-86): the classic, non-extended measure as DESIGN.md section 13 defines it
    estoi(ref, est, sr=16000)   extended STOI (Jensen & Taal 2016; pystoi's extended=True), DESIGN.md section 13f: an EXTENSION metric,
                                not in the reference's registry
    sdr(ref, est, sr=16000, filter_len=512)
                                SDR (:55-57): bss_eval_sources for one source as DESIGN.md section 13g defines it, dB; the reference
                                defines it without registering it (UNREGISTERED_REFERENCE_METRICS)

Every one takes lengths=: clip b of a zero-padded (or anyhow padded) batch is its first lengths[b] samples and scores bit for bit what
it scores alone; nothing beyond is read.  lengths is a device int tensor [B] (used as it is, never read back: a captured graph
replays with the lengths the tensor then holds), or a host sequence / numpy array / CPU tensor (checked for 0 <= len <= L, copied
once).  Without the keyword the calls launch what they always did.

Inputs are device tensors [B, L] or [L] (f32, 16 kHz for stoi); the result is a device tensor [B] (a 0-d tensor for [L]) and
nothing is read back, so a call can be captured into a HIP graph once its tables and workspace exist (they are made on the first call
for a device and shape, and kept).  A cached workspace is shared by every call of that shape: calls on different streams must be
ordered by the caller.

Deviations from the reference, recorded here and in DESIGN.md section 13:
  * WB_PESQ / NB_PESQ (an ITU reference program behind the `pesq` / `pypesq` packages) are not built; looking them up raises.
  * The reference's best-epoch score is (STOI + (WB_PESQ + 0.5) / 5) / 2 (base_trainer.py:370-376), which needs PESQ; the trainer
    here scores an epoch by the enhanced mean of ONE metric, [trainer.validation] score_metric.
  * pystoi is not installed where this was written: agreement with it is not claimed, only with the stated definition.
  * mir_eval is not installed either: the same holds for sdr.  Where mir_eval raises or falls back to lstsq (an empty clip, an all-zero
    reference, a Toeplitz system that is not positive definite in floating point) sdr returns NaN.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops

STOI_RATE = 16000
_TABLES: Dict[torch.device, torch.Tensor] = {}
_WORKSPACES: Dict[Tuple[torch.device, int, int], torch.Tensor] = {}
_FULL_LENGTHS: Dict[Tuple[torch.device, int, int], torch.Tensor] = {}
SDR_FILTER_LEN = 512                                                      # bss_eval_sources' flen
_SDR_WORKSPACES: Dict[Tuple[torch.device, int, int, int], torch.Tensor] = {}


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


def _lengths(lengths, B: int, L: int, single: bool, device, name: str) -> Optional[torch.Tensor]:
    """lengths= of the metrics -> int32 [B] on `device` (None stays None).  A device tensor is taken on trust (the kernels clamp to
    [0, L]); anything on the host is judged here, before the device is touched."""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor) and lengths.device.type != "cpu":
        if lengths.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool):
            raise TypeError(f"{name}: lengths must be an integer tensor, got {lengths.dtype}")
        t = lengths.reshape(1) if single and lengths.numel() == 1 else lengths
        if t.shape != (B,):
            raise ValueError(f"{name}: lengths {tuple(lengths.shape)} for {B} clip(s): expected [{B}]")
        return t.to(device=device, dtype=torch.int32).contiguous()
    import numpy as np
    a = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name}: lengths must be integers, got {a.dtype}")
    if single and a.size == 1:
        a = a.reshape(1)
    if a.shape != (B,):
        raise ValueError(f"{name}: lengths of shape {a.shape} for {B} clip(s): expected [{B}]" + (" or one value" if single else ""))
    if a.min() < 0 or a.max() > L:
        raise ValueError(f"{name}: lengths must lie in 0 .. L = {L}, got {int(a.min())} .. {int(a.max())}")
    return torch.from_numpy(a.astype(np.int32)).to(device)


def si_sdr(ref: torch.Tensor, est: torch.Tensor, lengths=None) -> torch.Tensor:
    r, e, single = _pair(ref, est, "si_sdr")
    out = ops.si_sdr(r, e, _lengths(lengths, r.shape[0], r.shape[1], single, r.device, "si_sdr"))
    return out[0] if single else out


def stoi(ref: torch.Tensor, est: torch.Tensor, sr: int = STOI_RATE, extended: bool = False, lengths=None) -> torch.Tensor:
    name = "estoi" if extended else "stoi"
    if sr != STOI_RATE:
        raise ValueError(f"{name}: sr must be {STOI_RATE} (the only rate built), got {sr!r}")
    r, e, single = _pair(ref, est, name)
    dev = r.device
    B, L = r.shape
    lens = _lengths(lengths, B, L, single, dev, name)
    tab = _TABLES.get(dev)
    if tab is None:
        tab = _TABLES[dev] = ops.stoi_tables(dev)
    key = (dev, B, L)
    ws = _WORKSPACES.get(key)
    if ws is None:
        ws = _WORKSPACES[key] = ops.stoi_workspace(B, L, dev)
    if extended and lens is None:                                        # the C entry point of ESTOI takes lengths: the whole rows
        lens = _FULL_LENGTHS.get(key)
        if lens is None:
            lens = _FULL_LENGTHS[key] = torch.full((B,), L, device=dev, dtype=torch.int32)
    out = ops.stoi(r, e, tab, ws, lengths=lens, extended=bool(extended))
    return out[0] if single else out


def estoi(ref: torch.Tensor, est: torch.Tensor, sr: int = STOI_RATE, lengths=None) -> torch.Tensor:
    return stoi(ref, est, sr=sr, extended=True, lengths=lengths)


def sdr(ref: torch.Tensor, est: torch.Tensor, sr: int = STOI_RATE, filter_len: int = SDR_FILTER_LEN, lengths=None) -> torch.Tensor:
    """bss_eval SDR of one source: est may be any filter_len-tap filtering of ref before anything counts as error"""
    if sr != STOI_RATE:
        raise ValueError(f"sdr: sr must be {STOI_RATE} (the only rate built), got {sr!r}")
    if isinstance(filter_len, bool) or not isinstance(filter_len, int) or not 1 <= filter_len <= ops.SDR_MAX_TAPS:
        raise ValueError(f"sdr: filter_len must be an integer in 1 .. {ops.SDR_MAX_TAPS}, got {filter_len!r}")
    r, e, single = _pair(ref, est, "sdr")
    dev = r.device
    B, L = r.shape
    lens = _lengths(lengths, B, L, single, dev, "sdr")
    key = (dev, B, L, filter_len)
    ws = _SDR_WORKSPACES.get(key)
    if ws is None:
        ws = _SDR_WORKSPACES[key] = ops.sdr_workspace(B, L, filter_len, dev)
    out = ops.sdr(r, e, ws, filter_len, lengths=lens)
    return out[0] if single else out


class _Registry(dict):
    """REGISTERED_METRICS of train_base/metrics.py:129-135, less the PESQ entries, which say why they are missing.  A name of
    EXTENSION_METRICS, then of UNREGISTERED_REFERENCE_METRICS, is found by lookup without being listed: the registry's keys stay the
    reference's."""

    def __missing__(self, name):
        if name in EXTENSION_METRICS:
            return EXTENSION_METRICS[name]
        if name in UNREGISTERED_REFERENCE_METRICS:
            return UNREGISTERED_REFERENCE_METRICS[name]
        if name in ("WB_PESQ", "NB_PESQ"):
            raise KeyError(f"{name}: PESQ is not built on this path (it is an ITU reference program, not closed-form signal processing); "
                           f"registered metrics: {sorted(self)}")
        raise KeyError(f"{name!r} is not a registered metric; registered metrics: {sorted(self)}; extension metrics: "
                       f"{sorted(EXTENSION_METRICS)}; reference metrics outside its registry: {sorted(UNREGISTERED_REFERENCE_METRICS)}")


REGISTERED_METRICS = _Registry({"SI_SDR": si_sdr, "STOI": stoi})
# metrics beyond the reference's registry, looked up through REGISTERED_METRICS by name ([trainer.validation] metrics = ["ESTOI", ...])
EXTENSION_METRICS = {"ESTOI": estoi}
# metrics that the reference's file defines but does not register (train_base/metrics.py:55-57), looked up the same way
UNREGISTERED_REFERENCE_METRICS = {"SDR": sdr}
# the reference's spellings (train_base/metrics.py:55,60,85)
SI_SDR, STOI, ESTOI, SDR = si_sdr, stoi, estoi, sdr
