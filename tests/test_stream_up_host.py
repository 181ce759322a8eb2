"""CPU: streaming inference of CRUSE4MagAddSkipUpsample (the upsample decoder) -- everything that needs no GPU.

The per-frame restatement (tests/stream_up_ref.py) reproduces the oracle model run offline, so that tests/test_gpu_stream_up.py can hold
the kernels to its per-frame intermediates; the polyphase form the kernel's header states is the conv on the upsampled row; the header,
the ctypes table and the library agree on the two new entry points; the host packer writes the [Cout][Cin][3] decoder weights with
BatchNorm folded."""
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import cruse_oracle as O
from oracle import cruse_oracle_ext as X
from tests.stream_up_ref import as_double, channels, nontrivial_bn, polyphase_upconv, stream_clip
from tests.util import rel_l2

CONFIGS = [dict(ch=(1, 4, 8, 16, 32), rnn_groups=2), dict(ch=(1, 3, 5, 6, 8), rnn_groups=1), dict(rnn_groups=4)]
IDS = ["small_g2", "odd_g1", "g4"]


def oracle_model(cfg):
    m = X.CRUSE4MagAddSkipUpsample(**cfg)
    O.closed_form_init(m)
    nontrivial_bn(m)
    return m.eval()


def offline(m, x):
    with torch.no_grad():
        _, est, _ = O.enhanced_spectrum(m, x.view(1, -1))
        return O.istft(torch.complex(est[..., 0], est[..., 1]).transpose(1, 2), 320, 160, 320, length=x.numel()).view(-1)


def offline64(m, x):
    """offline() with float64 as the default dtype, so that the Hann windows the oracle's stft / istft build are float64 as well (they are
    torch.hann_window(n_fft) without a dtype; a float32 window under float64 data would put its 6e-8 rounding into the comparison)"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return offline(m, x)
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_per_frame_restatement_equals_offline_f64(cfg):
    """float64 on both sides: the restatement and the offline model differ by rounding alone, so 1e-10 is a bar on the block contract
    (frame 0 reflected, the end frame end-reflected, one previous row per encoder level, overlap-add over the window envelope)"""
    m = as_double(oracle_model(cfg))
    x = O.synth_pair(1, 160 * 40, seed=11)[0].view(-1).double()
    got, frames = stream_clip(m, x, dtype=torch.float64)
    ref = offline64(m, x)
    assert got.dtype == ref.dtype == torch.float64 and got.shape == ref.shape and len(frames) == 41
    err = rel_l2(got, ref)
    print(f"{cfg}: streaming restatement vs offline, float64: rel-L2 {err:.2e}")
    assert err <= 1e-10


def test_per_frame_restatement_f32_and_shortest_clip():
    m = oracle_model(CONFIGS[0])
    for n in (2, 30):
        x = O.synth_pair(1, 160 * n, seed=4)[0].view(-1)
        got, frames = stream_clip(m, x)
        assert got.dtype == torch.float32 and len(frames) == n + 1
        assert rel_l2(got, offline(m, x)) <= 1e-6
    with pytest.raises(ValueError, match="as_double"):
        stream_clip(m, torch.zeros(320), dtype=torch.float64)


@pytest.mark.parametrize("Fin,Cin,Cout", list(itertools.product((1, 2, 10), (1, 3), (1, 3))))
def test_polyphase_identity(Fin, Cin, Cout):
    """even fo = 2j: W0 in[j-1] + (W1 + W2) in[j]; odd fo = 2j+1: (W0 + W1) in[j] + W2 in[j+1]; the out-of-range terms absent --
    against F.conv2d(F.interpolate(...)) in float64, every column including 0 and 2*Fin - 1 (Fin = 1: both edges in one input column)"""
    gen = torch.Generator().manual_seed(100 * Fin + 10 * Cin + Cout)
    x = torch.randn(Cin, Fin, generator=gen, dtype=torch.float64)
    W = torch.randn(Cout, Cin, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(Cout, generator=gen, dtype=torch.float64)
    up = F.interpolate(x.view(1, Cin, 1, Fin), scale_factor=(1.0, 2.0), mode="nearest")
    ref = F.conv2d(up, W.view(Cout, Cin, 1, 3), b, padding=(0, 1)).view(Cout, 2 * Fin)
    got = polyphase_upconv(x, W, b)
    assert got.shape == ref.shape
    scale = float(ref.abs().max())
    for name, cols in (("all", slice(None)), ("column 0", slice(0, 1)), ("column 2*Fin-1", slice(2 * Fin - 1, 2 * Fin))):
        err = float((got[:, cols] - ref[:, cols]).abs().max())
        assert err <= 1e-13 * max(scale, 1.0), (name, err)
    # the oracle's own block is that conv: convkxf(mode="upsample") without norm, identity activation
    blk = X.convkxf(Cin, Cout, k=1, f=3, fstride=2, batch_norm=False, act=torch.nn.Identity(), mode="upsample", depthwise=False).double()
    with torch.no_grad():
        blk.sconv.weight.copy_(W.view(Cout, Cin, 1, 3))
        blk.sconv.bias.copy_(b)
        assert float((blk(x.view(1, Cin, 1, Fin)).view(Cout, -1) - got).abs().max()) <= 1e-13 * max(scale, 1.0)


def test_abi_declares_and_binds_the_up_entry_points():
    from cruse_amd import _lib
    from cruse_amd._abi_check import parse_header
    hdr = parse_header()
    for name, sibling in (("cruse_stream_decode_up", "cruse_stream_decode_pf"), ("cruse_stream_decode_n_up", "cruse_stream_decode_n_pf")):
        assert name in hdr, f"{name} is not declared in include/cruse_hip.h"
        assert hdr[name] == hdr[sibling]                                   # the full _pf argument list
        assert _lib.SIGNATURES[name] == hdr[name]
        fn = getattr(_lib.lib, name)                                       # the built library exports it
        assert len(fn.argtypes) == len(hdr[name][0])
    assert _lib.ABI_VERSION == 15 and _lib.lib.cruse_abi_version() == 15   # additive: the version stays
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "cruse_hip.h")).read()
    assert "#define CRUSE_ABI_VERSION 15\n" in src
    assert "cust_conv.py:163-166,177-184" in src


def _fold(bn):
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.double() * s


@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=IDS[:2])
def test_host_packer_layout_and_batchnorm_fold(cfg):
    """pack_weights(decoder="upsample") from the product model's own children: decW{k} is [Cout][Cin][3] with the BatchNorm scale on the
    OUTPUT channel, decB{k} the folded shift (dec2..4 have no conv bias), dec1 its own weight and bias; the encoder and skip entries as
    for unet_2.  The expected values are folded here from the oracle's modules, independently of the packer."""
    from cruse_amd import ops
    from cruse_amd.inferencer.streaming import pack_weights
    from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
    o = oracle_model(cfg)
    m = CRUSE4MagAddSkipUpsample(precision="f32", **cfg)
    m.load_state_dict(o.state_dict(), strict=True)
    ch = channels(o)
    lay = ops.stream_layout(ch)
    w = pack_weights(m.eval(), lay, "upsample")
    assert w.dtype == torch.float64 and w.numel() == lay["wtotal"]
    take = lambda name, n: w[lay[name]:lay[name] + n]
    used = torch.zeros(lay["wtotal"], dtype=torch.bool)

    def expect(name, t):
        t = t.detach().double().reshape(-1)
        assert torch.allclose(take(name, t.numel()), t, rtol=1e-14, atol=0), name
        used[lay[name]:lay[name] + t.numel()] = True

    for k in range(1, 5):
        enc, dec = getattr(o, f"enc{k}"), getattr(o, f"dec{k}")
        s, sh = _fold(enc[2])
        expect(f"encW{k}", enc[1].weight.double() * s.view(-1, 1, 1, 1))
        expect(f"encB{k}", enc[1].bias.double() * s + sh)
        expect(f"skW{k}", getattr(o, f"skip_connect_{k}").weight)
        Wd = dec.sconv.weight.detach().double()                            # [Cout, Cin, 1, 3]
        assert tuple(Wd.shape) == (ch[k - 1], ch[k], 1, 3)
        if k > 1:
            assert dec.sconv.bias is None
            s, sh = _fold(dec.norm)
            assert float((s - 1).abs().max()) > 1e-2 and float(sh.abs().max()) > 1e-2     # the statistics are not trivial
            got = take(f"decW{k}", Wd.numel()).view(ch[k - 1], ch[k], 3)
            for co in range(ch[k - 1]):                                    # element [co][ci][kw] at (co * Cin + ci) * 3 + kw
                for ci in range(ch[k]):
                    assert torch.allclose(got[co, ci], Wd[co, ci, 0] * s[co], rtol=1e-14, atol=0), (k, co, ci)
            expect(f"decW{k}", Wd * s.view(-1, 1, 1, 1))
            expect(f"decB{k}", sh)
        else:
            expect("decW1", Wd)
            expect("decB1", dec.sconv.bias)
    for n in ("ln1g", "ln1b", "ln2g", "ln2b"):
        ln = getattr(o.gru, n[:3])
        expect(n, ln.weight if n.endswith("g") else ln.bias)
    assert float(w[~used].abs().max() if (~used).any() else 0.0) == 0.0    # the padding between the fields stays zero
    # a packed decoder level evaluates to the oracle's block (eval mode) on a random row
    k = 3
    x = torch.randn(ch[k], 160 >> k, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    Wp = take(f"decW{k}", ch[k - 1] * ch[k] * 3).view(ch[k - 1], ch[k], 3)
    got = torch.relu(polyphase_upconv(x, Wp, take(f"decB{k}", ch[k - 1])))
    ref = as_double(o).dec3(x.view(1, ch[k], 1, -1)).view(ch[k - 1], -1)
    assert rel_l2(got, ref) <= 1e-12
    with pytest.raises(ValueError, match="decoder"):
        pack_weights(m, lay, "bogus")


def test_host_packer_transposed_is_unchanged():
    """the unet_2 path through the same function keeps ConvTranspose2d's [Cin][Cout][3] and the scale on dim 1"""
    from cruse_amd import ops
    from cruse_amd.inferencer.streaming import pack_weights
    from cruse_amd.model.cruse_net import unet_2
    cfg = dict(ch=(1, 3, 5, 6, 8), rnn_groups=1)
    o = O.unet_2(**cfg)
    O.closed_form_init(o)
    nontrivial_bn(o)
    m = unet_2(precision="f32", **cfg)
    m.load_state_dict(o.state_dict())
    lay = ops.stream_layout(cfg["ch"])
    w = pack_weights(m.eval(), lay)
    s, sh = _fold(o.bn3_t)
    t = (o.conv3_t.weight.detach().double() * s.view(1, -1, 1, 1)).reshape(-1)
    assert torch.allclose(w[lay["decW3"]:lay["decW3"] + t.numel()], t, rtol=1e-14, atol=0)
    b = o.conv3_t.bias.detach().double() * s + sh
    assert torch.allclose(w[lay["decB3"]:lay["decB3"] + b.numel()], b, rtol=1e-14, atol=0)
