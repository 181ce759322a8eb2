"""Host side of DESIGN section 17 (no device): the ERB width tables and matrices against the reference's own (fixture G24), the
state-dict surface of GroupedLinearEinsum / GroupedLinear / SqueezedGRU / SqueezedGRU_S, constructor refusals, and the C interface of
the new entry points before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from model.based_model.cust_conv import (GroupedLinear, GroupedLinearEinsum, SqueezedGRU, SqueezedGRU_S, erb2freq, erb_fb, erb_fb_use,
                                         freq2erb)

ERB_CONFIGS = ((16000, 320, 32, 2), (16000, 320, 24, 1), (48000, 960, 32, 2))


@pytest.fixture(scope="module")
def g24(golden):
    return golden("g24_squeezed.npz")


@pytest.mark.parametrize("i", range(3))
def test_erb_fb_widths(g24, i):
    width = erb_fb(*ERB_CONFIGS[i])
    assert width.dtype == torch.int16
    assert width.tolist() == g24[f"erb/{i}/width"].tolist()
    assert int(width.sum()) == ERB_CONFIGS[i][1] // 2 + 1 == (161, 161, 481)[i]


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("normalized", (True, False))
@pytest.mark.parametrize("inverse", (True, False))
def test_erb_fb_use_matrices(g24, i, normalized, inverse):
    width = g24[f"erb/{i}/width"].astype(int)
    fb = erb_fb_use(width, ERB_CONFIGS[i][0], normalized=normalized, inverse=inverse)
    want = g24[f"erb/{i}/fb_n{int(normalized)}_i{int(inverse)}"]
    assert tuple(fb.shape) == want.shape and fb.dtype == torch.float32
    assert np.array_equal(fb.numpy(), want)


def test_erb_scale_round_trip():
    f = torch.tensor([0.0, 100.0, 1000.0, 8000.0, 24000.0])
    assert torch.allclose(erb2freq(freq2erb(f)), f, rtol=1e-5, atol=1e-3)
    assert float(freq2erb(torch.tensor([0.0]))) == 0.0


def _keys(m):
    return [f"{k}:{','.join(str(d) for d in v.shape)}" for k, v in m.state_dict().items()]


def _build(name):
    if name == "gle":
        return GroupedLinearEinsum(96, 64, 8)
    if name == "gl_shuffle":
        return GroupedLinear(96, 40, 8, shuffle=True)
    if name == "gl_cat":
        return GroupedLinear(96, 40, 8, shuffle=False)
    if name == "sq2":
        return SqueezedGRU(96, 64, output_size=40, num_layers=2, linear_groups=8, gru_skip_op=nn.Identity, linear_act_layer=nn.ReLU)
    if name == "sqs":
        return SqueezedGRU_S(96, 64, output_size=96, num_layers=1, gru_skip_op=nn.Identity)
    if name == "sq_noout":
        return SqueezedGRU(96, 64, output_size=None)
    if name == "sq_tmajor":
        return SqueezedGRU(96, 64, output_size=40, num_layers=2, linear_groups=8, batch_first=False, gru_skip_op=nn.Identity,
                           linear_act_layer=nn.ReLU)
    if name == "sq_tanh":
        return SqueezedGRU(96, 64, output_size=40, gru_skip_op=nn.Identity, linear_act_layer=nn.Tanh)
    raise KeyError(name)


@pytest.mark.parametrize("name", ("gle", "gl_shuffle", "gl_cat", "sq2", "sqs", "sq_noout", "sq_tmajor", "sq_tanh"))
def test_state_dict_surface(g24, name):
    assert _keys(_build(name)) == g24[f"keys/{name}"].tolist()


def test_named_keys_and_children():
    sq = _build("sq2")
    keys = list(sq.state_dict())
    assert keys == ["linear_in.0.weight"] + [f"gru.{n}_l{k}" for k in (0, 1) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + [
        "linear_out.0.weight"]
    assert isinstance(sq.gru, nn.GRU) and sq.gru.num_layers == 2 and isinstance(sq.gru_skip, nn.Identity)
    assert isinstance(sq.linear_in[0], GroupedLinearEinsum) and isinstance(sq.linear_in[1], nn.ReLU)
    assert isinstance(_build("sq_noout").linear_out, nn.Identity) and _build("sq_noout").gru_skip is None
    gl = _build("gl_shuffle")
    assert list(gl.state_dict())[:2] == ["layers.0.weight", "layers.0.bias"] and len(gl.layers) == 8
    assert gl.shuffle is True and GroupedLinear(96, 40, 1, shuffle=True).shuffle is False
    assert "groups: 8" in repr(_build("gle"))


def test_default_initialisation():
    # kaiming_uniform_(a = sqrt(5)) on [G, Ig, Hg]: torch's fan_in of a 3-D tensor is size(1) * size(2) = Ig * Hg -> bound 1 / sqrt(Ig * Hg)
    torch.manual_seed(0)
    m = GroupedLinearEinsum(96, 64, 8)
    w = m.weight.detach()
    bound = 1.0 / (12 * 8) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound and m.weight.requires_grad


def test_constructor_refusals():
    with pytest.raises(AssertionError):
        GroupedLinearEinsum(96, 64, 7)
    with pytest.raises(AssertionError):
        GroupedLinearEinsum(96, 60, 8)
    with pytest.raises(AssertionError):
        GroupedLinear(96, 40, 7)
    with pytest.raises(AssertionError):
        GroupedLinear(96, 41, 8)
    with pytest.raises(AssertionError):
        SqueezedGRU(100, 64, linear_groups=8)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        SqueezedGRU(96, 48)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        SqueezedGRU_S(96, 48)


def test_c_interface_refuses_before_any_hip_call():
    from cruse_amd._lib import lib
    from cruse_amd import ops
    for name in ("cruse_grouped_linear_fwd", "cruse_grouped_linear_bwd_dx", "cruse_grouped_linear_bwd_dw", "cruse_grouped_linear_dw_ws_bytes",
                 "cruse_band_pool", "cruse_band_expand"):
        assert hasattr(lib, name)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fwd = lambda rows, G, Ig, Hg, sg=1, si=1, so=1, omap=0, x=p: lib.cruse_grouped_linear_fwd(x, p, sg, si, so, None, rows, G, Ig, Hg, 0, omap,
                                                                                              p, None)
    assert fwd(0, 1, 1, 1) == -1 and fwd(1, 0, 1, 1) == -1 and fwd(1, 1, 0, 1) == -1 and fwd(1, 1, 1, 0) == -1
    assert fwd(1, 1, 1, 1, so=0) == -1 and fwd(1, 1, 1, 1, omap=2) == -1 and fwd(1, 1, 1, 1, x=None) == -1
    assert fwd(1, 70000, 1, 1) == -1 and fwd(2 ** 30 + 1, 1, 1, 1) == -1
    assert b"grouped_linear_fwd" in lib.cruse_last_error()
    assert lib.cruse_grouped_linear_bwd_dx(p, None, p, 1, 1, 1, 1, 1, 1, 1, 1, 0, p, None) == -1          # ReLU mask without y
    assert lib.cruse_grouped_linear_bwd_dw(p, None, p, 1, 1, 1, 1, 1, 0, p, 1, 1, 1, None, None, 0, None) == -1
    # the row split is a function of the shape alone: none below 512 rows, slabs of [G][Ig * Hg + Hg] floats above
    assert lib.cruse_grouped_linear_dw_ws_bytes(21, 8, 12, 5) == 0 and lib.cruse_grouped_linear_dw_ws_bytes(0, 8, 12, 5) == 0
    assert lib.cruse_grouped_linear_dw_ws_bytes(1100, 1, 96, 80) == 5 * (96 * 80 + 80) * 4
    assert lib.cruse_grouped_linear_bwd_dw(p, None, p, 1100, 1, 96, 80, 0, 0, p, 7680, 80, 1, None, None, 0, None) == -1   # no workspace
    tab = (ctypes.c_int * 3)(0, 1, 2)
    t = ctypes.addressof(tab)
    for fn in (lib.cruse_band_pool, lib.cruse_band_expand):
        assert fn(p, t, 0, 2, 2, 1, p, None) == -1 and fn(p, t, 1, 0, 1, 1, p, None) == -1 and fn(p, t, 1, 2, 3, 1, p, None) == -1
        assert fn(p, t, 1, ops.BAND_MAX_F + 1, 2, 1, p, None) == -1 and fn(None, t, 1, 2, 2, 1, p, None) == -1
        assert fn(p, None, 1, 2, 2, 1, p, None) == -1
