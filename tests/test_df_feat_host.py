"""CPU: DeepFilterNet's input features off the device -- the C entry point (declaration, signature table, library,
build scripts), get_norm_alpha and ExponentialUnitNorm's buffer against the fixture made by the reference's own code, the float64
restatement against that fixture's outputs, every refusal of cruse_df_feat (host pointers: a refused call dereferences nothing) and of
ops.df_feat (CPU tensors: every argument is judged before the device is asked for), DfFeatures' widths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import df_feat_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ALPHA_ARGS = ((48000, 480, 1), (16000, 160, 1), (16000, 160, 0.1), (16000, 160, 100))


def test_header_signatures_and_library_agree():
    from cruse_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert _lib.ABI_VERSION == 15 and "#define CRUSE_ABI_VERSION 15" in hdr and _lib.lib.cruse_abi_version() == 15
    m = re.search(r"int\s+cruse_df_feat\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 19 == len(_lib.SIGNATURES["cruse_df_feat"][0])
    assert _lib.SIGNATURES["cruse_df_feat"] == ("ppqqiiipiidfffppppp", "i")
    doc = hdr[hdr.index("DeepFilterNet's normalised input features"):hdr.index("cruse_df_feat(")]
    assert "test/test_norm.py:52-61" in doc and "test/test_erb.py:104" in doc and "fma(alpha, s, a * oma)" in doc
    assert re.search(r"int nb_df, double alpha, float log_eps", m.group(1))        # a double: (float)(1 - alpha) is torch's scalar
    assert f"#define CRUSE_DF_FEAT_TC {ops.DF_FEAT_TC}\n" in hdr
    assert getattr(_lib.lib, "cruse_df_feat") is not None
    for script in ("build.sh", "relink.sh"):
        assert " df_feat" in open(os.path.join(ROOT, "cruse_amd", "csrc", script)).read()


def test_get_norm_alpha_equals_the_reference(golden, capsys):
    from cruse_amd.acoustics import get_norm_alpha
    from cruse_amd.acoustics.df_features import _calculate_norm_alpha
    g = golden("dfeat.npz")
    assert [tuple(r) for r in g["alpha/args"]] == [tuple(float(v) for v in a) for a in ALPHA_ARGS]
    for (sr, hop, tau), want, raw in zip(ALPHA_ARGS, g["alpha/value"], g["alpha/raw"]):
        assert get_norm_alpha(sr=sr, hop_size=hop, tau=tau, log=False) == float(want)
        assert _calculate_norm_alpha(sr=sr, hop_size=hop, tau=tau) == float(raw)
    assert float(g["alpha/value"][3]) == 0.9999                                       # the rounding loop ran: round(., 3) is 1.0
    assert capsys.readouterr().out == ""
    assert get_norm_alpha() == 0.99 and "alpha = '0.99'" in capsys.readouterr().out   # log=True prints, as the reference does


@pytest.mark.parametrize("F", [1, 96])
def test_unit_norm_buffer_and_keys_equal_the_reference(golden, F):
    from cruse_amd.acoustics import ExponentialUnitNorm
    g = golden("dfeat.npz")
    m = ExponentialUnitNorm(0.8, F)
    keys = [f"{k}:{','.join(str(d) for d in v.shape)}" for k, v in m.state_dict().items()]
    assert keys == list(g[f"keys/{F}"]) == [f"init_state:1,1,{F},1"]
    assert np.array_equal(m.init_state.numpy(), g[f"init_state/{F}"])
    assert m.alpha == 0.8 and m.eps == 1e-14


@pytest.mark.parametrize("F", [1, 96])
@pytest.mark.parametrize("alpha", [0.8, 0.99])
def test_restatement_agrees_with_the_reference_outputs(golden, F, alpha):
    """the reference's f32 loop against the float64 restatement: a few f32 roundings per frame, relative to the largest output"""
    g = golden("dfeat.npz")
    x, y = g[f"x/{F}"], g[f"y/{F}/{alpha}"]
    assert x.shape == (2, 1, 37, F, 2) and y.shape == x.shape and y.dtype == np.float32
    _, spec, _, _ = R.df_feat(x[:, 0, ..., 0], x[:, 0, ..., 1], None, F, alpha)
    err = np.abs(spec - y[:, 0]).max() / np.abs(spec).max()
    assert err <= 8 * 2.0 ** -24, err


def test_restatement_states_and_erb_repair():
    """one step by hand: m = e (1 - a) + a m0, out = (e - m) / 40 (the repair: not -m / 40); the final states are the last m and s"""
    re, im = np.full((1, 1, 4), 3.0), np.full((1, 1, 4), 4.0)
    erb, spec, m, s = R.df_feat(re, im, np.array([0, 1, 4]), 2, 0.5, erb_state=[[-10.0, -20.0]], unit_state=[[1.0, 9.0]])
    e = 10 * np.log10(25.0 + 1e-10)
    assert np.allclose(m, [[(e - 10) / 2, (e - 20) / 2]]) and np.allclose(erb[0, 0], (e - m[0]) / 40.0)
    assert np.allclose(s, [[3.0, 7.0]]) and np.allclose(spec[0, 0], [[3 / np.sqrt(3.0), 4 / np.sqrt(3.0)], [3 / np.sqrt(7.0), 4 / np.sqrt(7.0)]])
    d_erb, d_unit = R.default_states(2, 32, 96)
    assert d_erb[1, 0] == -60 and d_erb[1, -1] == -90 and d_unit[0, 0] == 0.001 and abs(d_unit[0, -1] - 0.0001) < 1e-18


def test_every_c_refusal_names_its_argument():
    from cruse_amd._lib import lib
    buf = ctypes.create_string_buffer(64)                       # host memory: nothing below may dereference it
    P = ctypes.addressof(buf)

    def call(re=P, im=P, es=1, fs=161, B=2, T=5, F=161, starts=P, nb_erb=32, nb_df=96, alpha=0.99, log_eps=1e-10, scale=40.0, unit_eps=1e-14,
             erb_state=P, unit_state=P, feat_erb=P, feat_spec=P):
        rc = lib.cruse_df_feat(re, im, es, fs, B, T, F, starts, nb_erb, nb_df, alpha, log_eps, scale, unit_eps, erb_state, unit_state, feat_erb,
                               feat_spec, None)
        return rc, (lib.cruse_last_error() or b"").decode()

    for kw, rc_want, words in [
            (dict(re=None), -1, ("null spectrum",)), (dict(im=None), -1, ("null spectrum",)),
            (dict(starts=None), -1, ("nb_erb = 32 needs starts",)), (dict(erb_state=None), -1, ("erb_state",)), (dict(feat_erb=None), -1, ("feat_erb",)),
            (dict(unit_state=None), -1, ("nb_df = 96 needs unit_state",)), (dict(feat_spec=None), -1, ("feat_spec",)),
            (dict(nb_df=162), -1, ("nb_df = 162", "F = 161")), (dict(nb_df=-1), -1, ("nb_df = -1",)),
            (dict(nb_erb=162), -1, ("nb_erb = 162",)), (dict(nb_erb=0, nb_df=0), -1, ("no output is requested",)),
            (dict(alpha=1.0), -1, ("alpha = 1 ",)), (dict(alpha=-0.1), -1, ("alpha = -0.1",)), (dict(alpha=float("nan")), -1, ("alpha = nan",)),
            (dict(es=0), -1, ("bin_stride = 0",)), (dict(fs=160), -1, ("frame_stride = 160", "at least 161")),
            (dict(es=2, fs=320), -1, ("frame_stride = 320", "at least 321")),
            (dict(B=0), -1, ("B = 0",)), (dict(T=-1), -1, ("T = -1",)), (dict(F=0, nb_erb=0, nb_df=0), -1, ("F = 0",)), (dict(F=4096), -1, ("F = 4096",)),
            (dict(unit_eps=-1.0), -1, ("unit_eps = -1",)), (dict(scale=0.0), -1, ("erb_scale = 0",)),
            (dict(feat_spec=P + 4), -2, ("8-byte",))]:
        rc, msg = call(**kw)
        assert rc == rc_want and msg.startswith("df_feat:") and all(w in msg for w in words), (kw, rc, msg)
    # T = 0 is no refusal: nothing is launched or dereferenced; a skipped feature's pointers may be null
    assert call(T=0)[0] == 0
    assert call(T=0, nb_erb=0, starts=None, erb_state=None, feat_erb=None)[0] == 0
    assert call(T=0, nb_df=0, unit_state=None, feat_spec=None)[0] == 0


def test_every_ops_refusal_raises_with_its_message():
    from cruse_amd import ops
    re, im = torch.zeros(2, 5, 161), torch.zeros(2, 5, 161)
    starts = torch.tensor(R.starts_of([5] * 31 + [6]), dtype=torch.int32)

    def bad(match, re=re, im=im, starts=starts, nb_df=96, alpha=0.99, **kw):
        with pytest.raises(RuntimeError, match=match):
            ops.df_feat(re, im, starts, nb_df, alpha, **kw)

    bad("inference-only", re=re.clone().requires_grad_())
    bad("inference-only", im=im.clone().requires_grad_())
    bad(r"float32 \[B,T,F\]", re=re[0])
    bad(r"float32 \[B,T,F\]", im=im[:, :4])
    bad(r"float32 \[B,T,F\]", re=re.double())
    bad("nb_df = 162 outside", nb_df=162)
    bad("nb_df = -1 outside", nb_df=-1)
    bad("band table", starts=starts.long())
    bad("band table", starts=starts[:1])
    bad("nb_erb = 3 bands over F = 2", re=re[..., :2], im=im[..., :2], starts=starts[:4], nb_df=1)
    bad("no output is requested", starts=None, nb_df=0)
    for a in (1.0, -0.01, float("nan"), 1.5):
        bad("alpha = .* outside", alpha=a)
    bad(r"erb_state must be contiguous float32 \[2, 32\]", erb_state=torch.zeros(2, 31))
    bad(r"unit_state must be contiguous float32 \[2, 96\]", unit_state=torch.zeros(2, 96, dtype=torch.float64))
    bad(r"out feat_erb must be contiguous float32 \[2, 5, 32\]", out=(torch.zeros(2, 5, 31), None))
    bad(r"out feat_spec must be contiguous float32 \[2, 5, 96, 2\]", out=(None, torch.zeros(2, 5, 96)))
    bad("HIP device", re=re, im=im)                                                   # every argument stands: only the device is missing


def test_plane_layouts_are_read_in_place():
    """planar planes and the views of an interleaved tensor go to the kernel as they are; anything else is copied to planar"""
    from cruse_amd.ops import _df_planes
    x = torch.zeros(3, 7, 11, 2)
    re, im, es, fs = _df_planes(x[..., 0], x[..., 1])
    assert (es, fs) == (2, 22) and re.data_ptr() == x.data_ptr() and im.data_ptr() == x.data_ptr() + 4
    p, q = torch.zeros(3, 7, 11), torch.zeros(3, 7, 11)
    re, im, es, fs = _df_planes(p, q)
    assert (es, fs) == (1, 11) and re.data_ptr() == p.data_ptr() and im.data_ptr() == q.data_ptr()
    x1 = torch.zeros(3, 7, 1, 2)                                                       # F = 1 and T = 1: the strides that matter are taken
    assert _df_planes(x1[..., 0], x1[..., 1])[2:] == (1, 2)
    xt = torch.zeros(3, 1, 11, 2)
    assert _df_planes(xt[..., 0], xt[..., 1])[2:] == (2, 22)
    re, im, es, fs = _df_planes(p.transpose(1, 2).contiguous().transpose(1, 2), q)     # bins not the fastest axis: copied
    assert (es, fs) == (1, 11) and re.is_contiguous()
    re, im, es, fs = _df_planes(p[:, ::2], q[:, ::2])                                  # a frame stride that the clip stride does not follow
    assert (es, fs) == (1, 11) and re.is_contiguous() and re.shape == (3, 4, 11)


@pytest.mark.parametrize("cfg", [(16000, 320, 160, 32, 96, 2), (16000, 320, 160, 24, 161, 1), (48000, 960, 480, 32, 96, 2)])
def test_df_features_widths_are_erb_fb(cfg):
    from cruse_amd.acoustics import DfFeatures, get_norm_alpha
    from cruse_amd.model.based_model.cust_conv import erb_fb
    sr, n_fft, hop, nb_erb, nb_df, mnf = cfg
    m = DfFeatures(sr=sr, fft_size=n_fft, hop_size=hop, nb_erb=nb_erb, nb_df=nb_df, min_nb_freqs=mnf)
    assert m.widths == [int(w) for w in erb_fb(sr, n_fft, nb_erb, mnf)] and sum(m.widths) == n_fft // 2 + 1 == m.freq_bins
    assert m.alpha == get_norm_alpha(sr=sr, hop_size=hop, tau=1.0, log=False) == 0.99
    assert len(list(m.state_dict())) == 0
    with pytest.raises(ValueError, match="nb_df"):
        DfFeatures(nb_df=162)
