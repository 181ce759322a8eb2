"""What a training step of unet_2 decides before it launches anything, as pure functions of shapes, the precision and an EngineConfig: no
device, stream or tensor is touched (ops.gru_plan / bnin_eligible / mask_head_eligible are host-only).  The forward passes of cruse_net.py
compute a plan once and keep it in ctx; the backward passes read it there.  Two decisions need addresses and stay at their launches: whether
the per-group biases lie at one stride (LayerPlan.grouped: "one launch IF they do") and whether dW_hh follows dW_ih in memory."""
import functools
from dataclasses import dataclass
from typing import FrozenSet, Optional, Tuple

import torch

from .. import ops


@dataclass(frozen=True)
class LayerPlan:
    """One forward gate projection gi = x W_ih^T + b_ih.  form, the GEMM each group runs: f32 (ops.gemm) | bf16 | bf16x3 (W_ih hi + lo planes:
    x3) | bf16x3_splitx (x hi + lo as well: split_x) | f16 (one pass) | f16x2 (f16 x against W_ih hi + lo); grouped: the groups in ONE launch.
    The 2-byte operand is written by the kernel that produces the rows (fused_copy) or by a cast pass of its own (needs_cast_pass)."""
    form: str; operand_dtype: torch.dtype; gi_dtype: torch.dtype
    fused_copy: bool; needs_cast_pass: bool; grouped: bool
    x3: bool; split_x: bool


@dataclass(frozen=True)
class GgruPlan:
    """fast: bf16-operand GEMMs (K = Hg and K = 3*Hg are rounded up to whole 64-deep tiles, kp -- the weight operand is zero padded (K-tiled),
    the activation operand reads on into the next group / row (finite values, zero weights), `pad` zero elements behind a cast operand);
    fwd_T: the forward pass makes the time-major copies of the weight-gradient GEMMs (where a side stream runs); dx_atr: where dX is wanted."""
    fast: bool; fwd_T: bool; dx_atr: bool
    pad: int; kp: int
    layers: Tuple[LayerPlan, LayerPlan]


_chains_of_8 = functools.lru_cache(maxsize=None)(lambda B, Hg, prec: ops.gru_plan(B, 1, Hg, prec)["clips_per_chain"] == 8)


def ggru_plan(B: int, T: int, H: int, groups: int, prec, cfg, training: bool, save: bool, slot: int = 0) -> GgruPlan:
    """training: a training-mode BatchNorm in front writes layer 1's operand copy (unet2_forward; not the stand-alone GGRU, not eval).
    slot (the issue's signature; every caller runs slot 0): recurrences on other slots make no forward copies and read f32 gi rows."""
    g, Hg, code = groups, H // groups, ops.prec_code(prec)
    fast = code == ops.PREC_BF16 and Hg % 32 == 0
    # The forward projection corrects the bf16 rounding of W_ih (a second pass with its low plane): that rounding
    # dominates the forward error of the bf16 mode (enhanced spectrum 1.25e-3 -> 5.1e-4 rel-L2 on fixture G6;
    # correcting x too only reaches 4.8e-4).  CRUSE_GI_X3: bit 0 / 1 = layer 1 / 2 corrected, bit 2 = also split x.
    # Default: W_ih split on both layers; x split as well when Hg <= 320 (K is then short enough that the third pass
    # costs < 0.04 ms per step, and the grouped configurations need it for the 1e-3 bar at T = 401: DESIGN.md section 2)
    knob = int(cfg.gi_x3) if cfg.gi_x3 is not None else (7 if Hg <= 320 else 3)
    # The gate projections read ONE bf16 plane of their activation operand, unpadded: the producer (BatchNorm / LayerNorm
    # kernel) can then write that copy itself instead of a separate cast pass.
    copy = fast and Hg % 64 == 0 and not (knob & 4)
    # Forward gate projections as ONE pass on IEEE-f16 operands (EngineConfig.gi_f16, cruse_gemm_f16_nt): 11 significant bits on x
    # and W_ih, where the split-bf16 form keeps x at 8 bits and spends a second (Hg <= 320: and a third) pass on low planes.  The
    # producers' operand copies are then f16 tensors (g = 1; with g > 1 the interleaving LayerNorm has no fused copy and a cast pass
    # makes it) and W_ih is K-tiled as f16.  The operands are BatchNorm + ReLU / LayerNorm outputs and |W_ih| ~ 1 / sqrt(Hg): inside
    # f16's range; a value past 65504 would surface as a non-finite loss and the guarded optimizer step skips (engine.step_health).
    # Not with the row-major TN weight gradients or the time-chunk pipeline, which read the bf16 copies.
    # Only where the split-bf16 form does NOT split x as well (Hg > 320 by default, i.e. g = 1 at H = 640): the three-pass form of the
    # grouped configurations carries ~16 bits on both operands and measured BETTER than f16 there (enhanced spectrum at T = 401, closed-form
    # init, g = 4: 3.1e-4 against 1.7e-3; g = 2: 9e-5 against 5.5e-4), so those keep it.
    f16_bits = (int(cfg.gi_f16) * 3 if isinstance(cfg.gi_f16, bool) else int(cfg.gi_f16 or 0)) if fast and not (knob & 4) else 0
    # gi rows: f32, or IEEE f16 where the recurrence reads them (EngineConfig.gi_store_f16: bf16 mode, one group of 640, chains of 8 clips
    # -- cruse_gru_seq_fwd_gi16): the largest tensor of the forward pass, written once and read once -- 197 -> 98 MB per layer at the bench shape
    gi16 = bool(cfg.gi_store_f16) and fast and g == 1 and Hg == 640 and slot == 0
    if gi16:
        # chains of 8 on the tag-free lean kernel?  A pure function of the shape (cached: two ctypes round trips per layer and step otherwise);
        # the three library options that select another kernel are A/B switches of probes and tests, looked up only when one is set
        lo = cfg.lib_options
        gi16 = _chains_of_8(B, Hg, code) and (lo.get("gru_tf", 1), lo.get("gru_wlo", 0), lo.get("gru_fwd_lean", 1)) == (1, 0, 1)
    layers = []
    for li in (0, 1):
        x3, f16 = bool(knob >> li & 1), bool(f16_bits >> li & 1)
        split_x = bool(knob & 4) and x3
        # layer 1's rows come from the BatchNorm of level L, layer 2's from the interleaving LayerNorm (no fused f16 copy with g > 1)
        fused = copy and (training if li == 0 else not (f16 and g > 1))
        dt = torch.float32 if not fast else torch.float16 if f16 else torch.bfloat16
        form = {torch.float32: "f32", torch.float16: "f16x2" if x3 and li == 0 else "f16",
                torch.bfloat16: "bf16x3_splitx" if split_x else "bf16x3" if x3 else "bf16"}[dt]
        layers.append(LayerPlan(form=form, operand_dtype=dt, fused_copy=fused, needs_cast_pass=fast and not fused, x3=x3, split_x=split_x,
                                gi_dtype=torch.float16 if gi16 else torch.float32, grouped=fast and g > 1 and dt == torch.bfloat16))
    return GgruPlan(fast=fast, fwd_T=bool(save) and fast and slot == 0, dx_atr=fast and bool(cfg.dx_atr) and Hg % 64 == 0 and g == 1,
                    pad=64 if Hg % 64 else 0, kp=(Hg + 63) // 64 * 64, layers=(layers[0], layers[1]))


@dataclass(frozen=True)
class LevelPlan:
    """Encoder level k: conv{k}; decoder level k: conv{k}_t, whose BatchNorm gives u_{k-1}.  conv_kind: bnin (the conv applies the BatchNorm of
    its VIRTUAL input while staging it) | bnstats (BatchNorm sums of its output in the epilogue) | plain.  virtual: the BatchNorm output behind
    this conv is never materialised in f32; head_deferred (decoder level 2): u_1 is left to unet2_mask_head."""
    conv_kind: str; virtual: bool; head_deferred: bool = False


@dataclass(frozen=True)
class UnetPlan:
    """enc[k], k = 1..L and dec[k], k = 2..L (None below); e_bf_dtype: the 2-byte copy of e_L the BatchNorm of level L writes for gate GEMM 1;
    backward: dprec of the data-gradient convs, bf16_levels whose du_k / de_k are stored as bf16."""
    enc: Tuple[Optional[LevelPlan], ...]; dec: Tuple[Optional[LevelPlan], ...]
    e_bf_dtype: Optional[torch.dtype]; ggru: GgruPlan
    dprec: object; all_mfma: bool
    dy_bf16: bool; fuse_bwd: bool; fuse_apply: bool
    bf16_levels: FrozenSet[int]; inline_mask: int


def unet_plan(ch, F0: int, groups: int, prec, cfg, training: bool, save: bool, update_running: bool, dec_mode: str, defer_head: bool,
              B: int, T: int) -> UnetPlan:
    """(update_running and T decide nothing today: they are the signature the plan was specified with)"""
    L = len(ch) - 1
    Fk = [F0 >> k for k in range(L + 1)]
    ups, bf16 = dec_mode == "upsample", ops.prec_code(prec) == ops.PREC_BF16
    # (the MFMA convs stage whole frame rows: up to 640 elements per row and level -- wider networks run the VALU kernels, unfused)
    rows_fit = all(ch[k] * Fk[k] <= 640 for k in range(1, L + 1))
    fz = bool(training and save and cfg.fuse_bn_fwd and cfg.fuse_bn_stats and rows_fit)        # EngineConfig.fuse_bn_fwd
    stats = "bnstats" if training and cfg.fuse_bn_stats else "plain"
    enc, dec, virt = [None], {}, False
    for k in range(1, L + 1):
        kind = "bnin" if virt else stats
        # e_k stays virtual when both of its forward consumers -- conv_{k+1} and skip_k -- take it fused (level L feeds the GGRU)
        virt = fz and k < L and ops.bnin_eligible(prec, ch[k], ch[k + 1]) and ops.bnin_eligible(prec, ch[k], ch[k])
        enc.append(LevelPlan(kind, virt))
    for k in range(L, 1, -1):
        kind = "bnin" if virt and not ups else stats
        # u_{k-1} stays virtual when its consumer conv{k-1}_t takes it fused (the last decoder layer, Cout = 1, is a VALU kernel)
        virt = fz and not ups and k - 1 >= 2 and ops.bnin_eligible(prec, ch[k - 1], ch[k - 2])
        dec[k] = LevelPlan(kind, virt, bool(defer_head and k == 2 and training and save and not ups and kind != "plain" and cfg.fuse_bn_bwd_stats
                                            and ops.mask_head_eligible(ch[1], Fk[1], Fk[0] + 1)))
    ggru = ggru_plan(B, T, ch[L] * Fk[L], groups, prec, cfg, training, save)
    e_bf_dtype = ggru.layers[0].operand_dtype if ggru.layers[0].fused_copy else None
    # backward-only tensors in bf16 (EngineConfig.bf16_dy): only where every consumer rounds them to bf16 operands anyway
    # ... and every consumer is an MFMA kernel (the VALU fallbacks of the convs and weight gradients take f32 only: channel counts
    # beyond 64 or not a power of two keep the f32 tensors -- ADVICE r4)
    all_mfma = all(8 <= c <= 64 and (c & (c - 1)) == 0 for c in ch[1:]) and rows_fit
    dy_bf16, fuse_bwd = bool(cfg.bf16_dy) and bf16 and all_mfma, bool(cfg.fuse_bn_bwd_stats)
    # ... and the data gradients of the levels between two MFMA kernels (EngineConfig.bf16_de): du_k / de_k for 2 <= k < L
    de_bf16 = dy_bf16 and bool(cfg.bf16_de) and fuse_bwd and not ups
    # dprec: data-gradient convolutions of the bf16 mode on plain bf16 operands (one MFMA, one conversion per element) like every
    # other backward contraction of that mode -- the split-bf16 x3 form is what the FORWARD convs need for the 1e-3 bar
    return UnetPlan(enc=tuple(enc), dec=(None, None) + tuple(dec[k] for k in range(2, L + 1)), e_bf_dtype=e_bf_dtype, ggru=ggru,
                    dprec=ops.PREC_BF16 if bf16 else prec, all_mfma=all_mfma, dy_bf16=dy_bf16, fuse_bwd=fuse_bwd,
                    fuse_apply=bool(cfg.fuse_bn_bwd_apply) and dy_bf16 and fuse_bwd and not ups,
                    bf16_levels=frozenset(range(2, L)) if de_bf16 else frozenset(), inline_mask=int(cfg.inline_mask))
