"""Scoring a model on a list of paired files: pre-mixed noisy / clean WAV pairs of any lengths, such as the
VoiceBank-DEMAND test set, through wavio.read_pcm16 -> cruse_resample_poly -> cruse_assemble_clips -> Inferencer.mag_mask_to_wave ->
the ragged metric kernels (cruse_amd.metrics with lengths=).

Stated semantics.  Pairs are ordered by length and scored in batches of batch_size consecutive pairs, each zero-padded to its longest
clip.  A clip's enhanced signal is the first `len` samples of what the model produces for the padded clip; the model is causal and in
eval mode, so that differs from enhancing the clip alone only within the last STFT window, which sees the zero padding where the lone
clip sees its end (batch_size = 1 has no padding and is the clip alone).  The noisy-side scores do not depend on the batching."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import wavio

SR = 16000


def _paths(lst: Union[str, Sequence[str]]) -> List[str]:
    return wavio.read_list(lst) if isinstance(lst, (str, os.PathLike)) else [os.fspath(p) for p in lst]


def read_pairs(clean_list, noisy_list):
    """-> (clean paths, noisy paths, what wavio.read_pcm16 gave for the clean files, for the noisy files).  Line i of one list pairs
    with line i of the other; unequal counts, and a pair that differs in sample rate or frame count, raise ValueError (naming the pair)."""
    clean, noisy = _paths(clean_list), _paths(noisy_list)
    if len(clean) != len(noisy):
        raise ValueError(f"evaluate_files: {len(clean)} clean files but {len(noisy)} noisy files: the lists pair line by line")
    if not clean:
        raise ValueError("evaluate_files: the lists name no file")
    fc, fn = [wavio.read_pcm16(p) for p in clean], [wavio.read_pcm16(p) for p in noisy]
    for i, ((pc, cc, rc), (pn, cn, rn)) in enumerate(zip(fc, fn)):
        if rc != rn or pc.shape[0] // cc != pn.shape[0] // cn:
            raise ValueError(f"evaluate_files: pair {i} ({clean[i]}, {noisy[i]}) differs: {pc.shape[0] // cc} frames at {rc} Hz against "
                             f"{pn.shape[0] // cn} frames at {rn} Hz")
    return clean, noisy, fc, fn


@torch.no_grad()
def evaluate_files(model, clean_list, noisy_list, metrics: Sequence[str] = ("SI_SDR", "STOI", "ESTOI"), batch_size: int = 16,
                   device="cuda", atten_lim_db=None, acoustics: Optional[dict] = None, head: str = "mask",
                   df_dims=(1, 5), post_filter=None, pf_tau: float = 0.02) -> Dict[str, object]:
    """Score `model` on the pairs (clean_list[i], noisy_list[i]); each list a list file (one WAV path per line, wavio.read_list) or a
    Python list of paths; 16-bit PCM at any rate, channel 0 of multi-channel files.  acoustics: the [acoustics] table of a config
    (n_fft, hop_length, win_length), the Inferencer's defaults without it.  head / df_dims: the Inferencer's ("df" for a model trained
    with the DeepFilter loss, BASELINE config 4).  post_filter / pf_tau: the Inferencer's ("iam" or "envelope": the perceptual post-filter
    on the mask).
    -> {"names": the clean files' base names, "lengths": int64 [n] samples at 16 kHz,
        "scores": {metric: {"Noisy": f32 [n], "Enhanced": f32 [n]}}, "mean": {metric: {"Noisy": float, "Enhanced": float}}}, in LIST order.
    One read-back per batch."""
    from . import ops
    from .filepairs import load_pool
    from .inferencer import Inferencer
    from .metrics import REGISTERED_METRICS
    names = tuple(metrics)
    fns = [REGISTERED_METRICS[m] for m in names]                         # KeyError names the registered metrics
    if int(batch_size) < 1:
        raise ValueError(f"evaluate_files: batch_size = {batch_size}")
    clean, noisy, fc, fn = read_pairs(clean_list, noisy_list)
    n = len(clean)
    device = torch.device(device)
    ac = acoustics or {}
    enhance = Inferencer(model, n_fft=ac.get("n_fft", 320), hop_length=ac.get("hop_length", 160),
                         win_length=ac.get("win_length", ac.get("n_fft", 320)), sr=SR, device=device, atten_lim_db=atten_lim_db,
                         head=head, df_dims=df_dims, post_filter=post_filter, pf_tau=pf_tau)
    with torch.cuda.device(device):
        # one flat pool for both sides: one ragged resampler launch per distinct (rate, channels), int16 read in the kernel
        pool, start, lens, _ = load_pool(clean + noisy, device, SR, files=fc + fn)
        assert np.array_equal(lens[:n], lens[n:])
        order = np.argsort(lens[:n], kind="stable")
        scores = np.zeros((len(names), 2, n), dtype=np.float32)
        for k in range(0, n, int(batch_size)):
            idx = order[k:k + int(batch_size)]
            B, L = idx.shape[0], int(lens[idx].max())
            first = np.arange(B + 1)
            seg = [np.stack([start[idx + o], np.zeros(B, dtype=np.int64), lens[idx]], axis=1) for o in (0, n)]
            c = ops.assemble_clips(pool, seg[0], first, L)
            x = ops.assemble_clips(pool, seg[1], first, L)
            ln = torch.from_numpy(lens[idx].astype(np.int32)).to(device)
            y = enhance.mag_mask_to_wave(x)
            rows = [torch.stack([f(c, x, lengths=ln), f(c, y, lengths=ln)]) for f in fns]
            scores[:, :, idx] = torch.stack(rows).cpu().numpy()           # the batch's one read-back
    return {"names": [os.path.basename(p) for p in clean], "lengths": lens[:n].copy(),
            "scores": {m: {"Noisy": scores[i, 0].copy(), "Enhanced": scores[i, 1].copy()} for i, m in enumerate(names)},
            "mean": {m: {"Noisy": float(scores[i, 0].astype(np.float64).mean()), "Enhanced": float(scores[i, 1].astype(np.float64).mean())}
                     for i, m in enumerate(names)}}
