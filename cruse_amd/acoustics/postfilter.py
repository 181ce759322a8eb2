"""The reference's perceptual post-filters of a mask, postfiltering and envelope_postfiltering (utils/utils.py:345-362), on the HIP
pointwise kernel cruse_mask_postfilter (ops.post_filter).  The signatures are the reference's, its spelling of tau included.

Both run the closed forms of DESIGN 12e (g the mask value in [0, 1], s = sin(pi g / 2)):
    postfiltering            g (1 + tao) s^2 / (s^2 + tao)            0 at g = 0, where the reference divides 0 by 0
    envelope_postfiltering   g s sqrt((1 + tao) s / (s^2 + tao))      the reference's eps term, its only use of `unproc`, is dropped
so `indata` and `unproc` do not enter the result; they are accepted, and `unproc`'s shape is checked.  Inference only.
"""
from __future__ import annotations

import torch

from .. import ops


def _mask(mask) -> torch.Tensor:
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise RuntimeError("post-filter: the mask must be a tensor on the HIP device (there is no CPU path)")
    return mask.to(torch.float32).contiguous()


def postfiltering(mask, indata=None, tao=0.02):
    """utils/utils.py:345-349: (1 + tao) mask / (1 + tao mask^2 / (mask sin(pi mask / 2))^2)"""
    return ops.post_filter(_mask(mask), tao, "iam")


def envelope_postfiltering(unproc, mask, tao=0.02):
    """utils/utils.py:352-362 (PercepNet's envelope post-filter; for a ratio mask in [0, 1])"""
    if torch.is_tensor(unproc) and torch.is_tensor(mask) and unproc.shape != mask.shape:
        torch.broadcast_shapes(unproc.shape, mask.shape)                  # raises where the reference's product would
    return ops.post_filter(_mask(mask), tao, "envelope")
