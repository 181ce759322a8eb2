"""The training step's plan (cruse_amd/model/step_plan.py) on the host: no device is needed.  The expected values are the decisions the
functional core of cruse_net.py took before the plan existed, read off that code and the EngineConfig docstrings, as literals; the
consistency properties run over the whole case matrix of the launch-trace test (tests/step_trace.py)."""
import pytest
import torch

from cruse_amd import ops
from cruse_amd.config import EngineConfig
from cruse_amd.model.step_plan import ggru_plan, unet_plan

from step_trace import B0, CASES, CH, F0, L0, _gi16_batch

T0 = L0 // 160 + 1


def plan(ch=CH, g=1, prec="bf16", training=True, save=True, dec_mode="transposed", defer_head=True, B=B0, **cfg):
    return unet_plan(ch, F0, g, prec, EngineConfig(**cfg), training, save, training, dec_mode, defer_head, B, T0)


def test_bench_configuration():
    p = plan()
    l1, l2 = p.ggru.layers
    assert p.ggru.fast and p.ggru.fwd_T and p.ggru.dx_atr
    assert (l1.form, l1.x3, l1.split_x, l1.operand_dtype, l1.fused_copy, l1.needs_cast_pass) == ("bf16x3", True, False, torch.bfloat16, True, False)
    assert (l2.form, l2.operand_dtype, l2.fused_copy, l2.needs_cast_pass) == ("f16", torch.float16, True, False)
    assert not l1.grouped and not l2.grouped
    assert (p.ggru.pad, p.ggru.kp) == (0, 640)
    assert l1.gi_dtype == torch.float32 and l2.gi_dtype == torch.float32
    assert p.e_bf_dtype == torch.bfloat16
    assert p.dprec == ops.PREC_BF16 and p.all_mfma and p.dy_bf16 and p.fuse_bwd and p.fuse_apply
    assert p.bf16_levels == {2, 3}
    assert p.inline_mask == 8
    assert [lv.conv_kind for lv in p.enc[1:]] == ["bnstats", "bnin", "bnin", "bnin"]
    assert [lv.virtual for lv in p.enc[1:]] == [True, True, True, False]
    assert [lv.conv_kind for lv in p.dec[2:]] == ["bnin", "bnin", "bnstats"]
    assert [lv.virtual for lv in p.dec[2:]] == [False, True, True]
    assert p.dec[2].head_deferred == ops.mask_head_eligible(8, 80, 161)
    assert not p.dec[3].head_deferred and not p.dec[4].head_deferred
    assert not plan(defer_head=False).dec[2].head_deferred


def test_four_groups():
    p = plan(g=4)
    for lp in p.ggru.layers:                 # knob 7: W_ih and x as hi + lo planes; ONE launch over the groups where the biases allow it
        assert (lp.form, lp.x3, lp.split_x, lp.grouped) == ("bf16x3_splitx", True, True, True)
        assert not lp.fused_copy and lp.needs_cast_pass and lp.operand_dtype == torch.bfloat16
    assert p.ggru.fast and (p.ggru.pad, p.ggru.kp) == (64, 192)
    assert not p.ggru.dx_atr
    assert p.e_bf_dtype is None


def test_two_groups_split_x_too():
    p = plan(g=2)
    assert [lp.form for lp in p.ggru.layers] == ["bf16x3_splitx"] * 2 and (p.ggru.pad, p.ggru.kp) == (0, 320)
    assert p.e_bf_dtype is None and not p.ggru.dx_atr


@pytest.mark.parametrize("g", [1, 4])
def test_f32(g):
    p = plan(g=g, prec="f32")
    assert not p.ggru.fast and not p.ggru.fwd_T and not p.ggru.dx_atr
    for lp in p.ggru.layers:
        assert (lp.form, lp.operand_dtype, lp.fused_copy, lp.needs_cast_pass, lp.grouped) == ("f32", torch.float32, False, False, False)
    assert p.e_bf_dtype is None and not p.dy_bf16 and not p.fuse_apply and p.bf16_levels == frozenset()
    assert p.dprec == "f32"
    assert not any(lv.virtual for lv in p.enc[1:] + p.dec[2:])


def test_gi_f16_on_both_layers():
    l1, l2 = plan(gi_f16=3).ggru.layers
    assert (l1.form, l1.operand_dtype, l1.fused_copy) == ("f16x2", torch.float16, True)
    assert (l2.form, l2.operand_dtype) == ("f16", torch.float16)
    assert plan(gi_f16=3).e_bf_dtype == torch.float16
    assert plan(g=4, gi_f16=3).ggru == plan(g=4).ggru            # knob bit 2 (x split as well) vetoes f16
    assert [lp.form for lp in plan(gi_f16=0).ggru.layers] == ["bf16x3", "bf16x3"]


def test_gi_x3_forms():
    assert [lp.form for lp in plan(gi_x3=0).ggru.layers] == ["bf16", "f16"]
    assert [lp.form for lp in plan(gi_x3=0, gi_f16=0).ggru.layers] == ["bf16", "bf16"]
    p = plan(gi_x3=7)
    assert [lp.form for lp in p.ggru.layers] == ["bf16x3_splitx"] * 2 and p.e_bf_dtype is None
    # g = 2 with x not split: the interleaving LayerNorm has no fused f16 copy -- a cast pass makes layer 2's operand, per-group launches
    l1, l2 = plan(g=2, gi_x3=3).ggru.layers
    assert (l1.form, l1.fused_copy, l1.grouped) == ("bf16x3", True, True)
    assert (l2.form, l2.fused_copy, l2.needs_cast_pass, l2.grouped) == ("f16", False, True, False)


def test_gi_store_f16():
    B = _gi16_batch()
    assert all(lp.gi_dtype == torch.float16 for lp in plan(B=B, gi_store_f16=True).ggru.layers)
    assert all(lp.gi_dtype == torch.float32 for lp in plan(B=B, g=2, gi_store_f16=True).ggru.layers)
    assert all(lp.gi_dtype == torch.float32 for lp in plan(B=B, gi_store_f16=True, lib_options={"gru_wlo": 1}).ggru.layers)
    assert all(lp.gi_dtype == torch.float32 for lp in ggru_plan(B, T0, 640, 1, "bf16", EngineConfig(gi_store_f16=True), True, True, slot=1).layers)


def test_stand_alone_ggru_and_eval_cast_their_operands():
    for p in (ggru_plan(B0, T0, 640, 1, "bf16", EngineConfig(), False, True), plan(training=False, save=False).ggru):
        assert (p.layers[0].form, p.layers[0].fused_copy, p.layers[0].needs_cast_pass) == ("bf16x3", False, True)
        assert (p.layers[1].form, p.layers[1].fused_copy) == ("f16", True)
    assert plan(training=False, save=False).e_bf_dtype is None and not plan(training=False, save=False).ggru.fwd_T


def test_backward_switches():
    assert not plan(bf16_dy=False).dy_bf16 and not plan(bf16_dy=False).fuse_apply and plan(bf16_dy=False).bf16_levels == frozenset()
    assert plan(bf16_de=False).dy_bf16 and plan(bf16_de=False).bf16_levels == frozenset() and plan(bf16_de=False).fuse_apply
    p = plan(fuse_bn_bwd_stats=False)
    assert not p.fuse_bwd and not p.fuse_apply and p.bf16_levels == frozenset() and not p.dec[2].head_deferred
    assert not plan(fuse_bn_bwd_apply=False).fuse_apply and plan(fuse_bn_bwd_apply=False).bf16_levels == {2, 3}
    p = plan(dec_mode="upsample")
    assert not p.fuse_apply and p.bf16_levels == frozenset() and p.dy_bf16
    assert [lv.conv_kind for lv in p.dec[2:]] == ["bnstats"] * 3 and not any(lv.virtual or lv.head_deferred for lv in p.dec[2:])
    p = plan()
    assert plan(inline_mask=31).inline_mask == 31
    assert not plan(dx_atr=False).ggru.dx_atr


def test_forward_switches():
    p = plan(fuse_bn_fwd=False)
    assert [lv.conv_kind for lv in p.enc[1:]] == ["bnstats"] * 4 and not any(lv.virtual for lv in p.enc[1:] + p.dec[2:])
    assert p.dec[2].head_deferred == ops.mask_head_eligible(8, 80, 161)
    p = plan(fuse_bn_stats=False)
    assert [lv.conv_kind for lv in p.enc[1:] + p.dec[2:]] == ["plain"] * 7 and not any(lv.virtual for lv in p.enc[1:] + p.dec[2:])
    assert not p.dec[2].head_deferred                                   # the head needs the sums of conv2_t's epilogue
    p = plan(ch=(1, 3, 5, 6, 8))
    assert not p.all_mfma and not p.dy_bf16 and not p.ggru.fast and [lp.form for lp in p.ggru.layers] == ["f32", "f32"]
    assert not any(lv.virtual for lv in p.enc[1:] + p.dec[2:])
    p = plan(ch=(1, 3, 5, 6, 16))
    assert p.ggru.fast and (p.ggru.pad, p.ggru.kp) == (64, 192) and not p.ggru.dx_atr and p.e_bf_dtype is None
    p = plan(ch=(1, 3, 5, 6, 32))
    assert p.ggru.fast and not p.all_mfma and not p.dy_bf16 and p.e_bf_dtype is None   # (Hg = 320: x is split as well)


def _case_plans():
    for name, spec in CASES.items():
        kind = spec.get("kind", "step")
        if kind == "ggru":
            continue
        training = kind != "eval"
        module = kind in ("module", "upsample")
        cfg = spec.get("cfg", {})
        defer_head = training and not module and spec.get("loss", "wo_male") == "wo_male" and cfg.get("fuse_mask_head", True)
        yield name, EngineConfig(**cfg), training, plan(ch=spec.get("ch", CH), g=spec.get("groups", 1), prec=spec.get("prec", "bf16"),
                                                        training=training, save=training, dec_mode="upsample" if kind == "upsample" else "transposed",
                                                        defer_head=defer_head, B=_gi16_batch() if spec.get("B") == "gi16" else B0, **cfg)


def test_consistency_over_the_trace_matrix():
    seen = 0
    for name, cfg, training, p in _case_plans():
        l1 = p.ggru.layers[0]
        assert p.e_bf_dtype == (l1.operand_dtype if l1.fused_copy else None), name
        for lp in p.ggru.layers:
            assert lp.fused_copy + lp.needs_cast_pass == (1 if p.ggru.fast else 0), name
            assert (lp.form == "f32") == (not p.ggru.fast) and (not lp.split_x or lp.x3), name
        for lv in p.enc[1:] + p.dec[2:]:
            if lv.virtual:
                assert cfg.fuse_bn_fwd and training, name                # (save == training in every case of the matrix)
            assert not (lv.virtual and lv.head_deferred), name
        for k in range(2, len(p.enc)):
            assert (p.enc[k].conv_kind == "bnin") == p.enc[k - 1].virtual, name
        for k in range(2, len(p.dec) - 1):
            assert (p.dec[k].conv_kind == "bnin") == p.dec[k + 1].virtual, name
        if p.fuse_apply:
            assert p.dy_bf16 and p.fuse_bwd, name
        if p.bf16_levels:
            assert p.dy_bf16 and p.fuse_bwd, name
        seen += 1
    assert seen == len(CASES) - 1
