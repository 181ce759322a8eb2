"""CPU: the multi-resolution spectral loss off the device -- the float64 restatement against the fixture made by the
reference's own code, the two C entry points (declaration, signature table, library), the workspace layout, every refusal of
cruse_mrspec_loss (host pointers: a refused call dereferences nothing), the factory tag, the Python surface's ValueErrors, the TOML."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mrspec_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_restatement_equals_the_reference_fixture(golden):
    g = golden("mrspec.npz")
    assert tuple(g["n_ffts"]) == (128, 256) and g["est"].shape == (2, 700) and g["est"].dtype == np.float32
    loss, grad = R.mrspec_loss_and_grad(torch.from_numpy(g["est"]), torch.from_numpy(g["ref"]), (128, 256), float(g["gamma"]),
                                        float(g["factor"]), float(g["f_complex"]))
    assert abs(float(loss) - float(g["loss"])) <= 1e-12 * abs(float(g["loss"]))
    assert R.rel_l2(grad, torch.from_numpy(g["grad"])) <= 1e-12
    # callable in f32 too, and close to f64 there
    l32, g32 = R.mrspec_loss_and_grad(torch.from_numpy(g["est"]), torch.from_numpy(g["ref"]), (128, 256), 0.3, 1000.0, 1000.0, dtype=torch.float32)
    assert l32.dtype == torch.float32 and abs(float(l32) - float(loss)) <= 1e-5 * float(loss)


def test_header_signatures_and_library_agree():
    from cruse_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert _lib.ABI_VERSION == 15 and "#define CRUSE_ABI_VERSION 15" in hdr and _lib.lib.cruse_abi_version() == 15
    assert re.search(r"size_t\s+cruse_mrspec_ws_bytes\(int B, int L, const int\* n_ffts, int R\);", hdr)
    m = re.search(r"int\s+cruse_mrspec_loss\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == 15 == len(_lib.SIGNATURES["cruse_mrspec_loss"][0])
    assert _lib.SIGNATURES["cruse_mrspec_ws_bytes"] == ("iipi", "z") and _lib.SIGNATURES["cruse_mrspec_loss"] == ("ppiipiffppzppfp", "i")
    assert "test/test_loss.py:193-229" in hdr[hdr.index("multi-resolution spectral loss"):hdr.index("cruse_mrspec_loss(")]
    for name in ("cruse_mrspec_ws_bytes", "cruse_mrspec_loss"):
        assert getattr(_lib.lib, name) is not None
    for script in ("build.sh", "relink.sh"):
        assert " mrspec" in open(os.path.join(ROOT, "cruse_amd", "csrc", script)).read()


HOPS = {128: 29, 256: 13, 512: 13, 1024: 9, 2048: 8}


def layout_bytes(B, L, n_ffts):
    """| f64 partial sums, B * runs_r per resolution | to 256 | f32 [B, L + N_r] per resolution, each to 256 |"""
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    parts = sum(B * -(-(L + n) // (HOPS[n] * n // 4)) for n in n_ffts)
    return up(8 * parts) + sum(up(4 * B * (L + n)) for n in n_ffts)


@pytest.mark.parametrize("B,L,n_ffts", [(2, 700, (128, 256)), (3, 2049, (128, 256, 512, 1024)), (1, 1025, (2048,)), (64, 64000, (128, 256, 512)),
                                        (1, 65, (128,)), (5, 12345, (2048, 128, 2048))])
def test_ws_bytes_follows_the_stated_layout(B, L, n_ffts):
    from cruse_amd import ops
    assert ops.mrspec_ws_bytes(B, L, n_ffts) == layout_bytes(B, L, n_ffts)


def test_ws_bytes_is_zero_for_refused_shapes():
    from cruse_amd import ops
    for B, L, n in [(0, 700, (128,)), (2, 64, (128,)), (2, 1024, (2048,)), (2, 700, (100,)), (2, 700, (64,)), (2, 9000, (4096,)), (2, 700, ()),
                    (2, 700, (128,) * 9), (70000, 700, (128,)), (2, (1 << 30) + 1, (128,)), (65535, 1 << 30, (128,))]:
        assert ops.mrspec_ws_bytes(B, L, n) == 0, (B, L, n)


def test_every_refusal_names_its_argument():
    from cruse_amd._lib import lib
    buf = ctypes.create_string_buffer(64)                       # host memory: nothing below may dereference it
    P = ctypes.addressof(buf)

    def call(est=P, ref=P, B=2, L=700, n_ffts=(128, 256), gamma=0.3, fc=None, ws=P, ws_bytes=1 << 40, loss=P, R=None):
        arr = (ctypes.c_int * max(len(n_ffts), 1))(*n_ffts)
        fca = (ctypes.c_float * len(fc))(*fc) if fc else None
        rc = lib.cruse_mrspec_loss(est, ref, B, L, ctypes.cast(arr, ctypes.c_void_p), len(n_ffts) if R is None else R, gamma, 1.0,
                                   ctypes.cast(fca, ctypes.c_void_p) if fca else None, ws, ws_bytes, loss, None, 1.0, None)
        return rc, (lib.cruse_last_error() or b"").decode()

    for kw, words in [(dict(est=None), ("est",)), (dict(ref=None), ("ref",)), (dict(ws=None), ("ws",)), (dict(loss=None), ("loss",)),
                      (dict(B=0), ("B=0",)), (dict(B=-3), ("B=-3",)), (dict(B=65536), ("B=65536",)),
                      (dict(R=0), ("R=0",)), (dict(n_ffts=(128,) * 9), ("R=9",)),
                      (dict(n_ffts=(128, 200)), ("n_ffts[1]=200",)), (dict(n_ffts=(64,)), ("n_ffts[0]=64",)), (dict(n_ffts=(4096,), L=9000), ("n_ffts[0]=4096",)),
                      (dict(L=128), ("L=128",)), (dict(L=1024, n_ffts=(128, 2048)), ("L=1024",)), (dict(L=(1 << 30) + 1), ("L=1073741825",)),
                      (dict(B=65535, L=1 << 30), ("B*L=",)),
                      (dict(gamma=0.0), ("gamma=0",)), (dict(gamma=-1.0), ("gamma=-1",)),
                      (dict(ws_bytes=layout_bytes(2, 700, (128, 256)) - 1), ("ws_bytes=",))]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("mrspec:") and all(w in msg for w in words), (kw, rc, msg)


def test_factory_tag_and_python_surface():
    import train_base.loss as TL
    from cruse_amd import ops
    from cruse_amd.engine import LOSSES, WAVE_LOSSES
    from cruse_amd.loss import MultiResSpecLoss, multi_res_spec_loss
    assert "mrspec" in LOSSES and "mrspec" in WAVE_LOSSES
    fn = TL.multi_res_spec_loss(n_ffts=[128, 256, 512], gamma=0.3, factor=1.0, f_complex=1.0)
    assert fn.cruse_loss == ("mrspec", dict(mrs_ffts=(128, 256, 512), mrs_gamma=0.3, mrs_factor=1.0, mrs_f_complex=(1.0, 1.0, 1.0)))
    assert TL.multi_res_spec_loss().cruse_loss == ("mrspec", dict(mrs_ffts=(128, 256, 512), mrs_gamma=0.3, mrs_factor=1.0, mrs_f_complex=None))
    assert TL.si_snr_loss().cruse_loss == ("si_snr", {})
    # the reference's constructor: None or 0 -> no complex term, a scalar -> every resolution, a list -> as given
    assert ops.mrspec_args((128, 256), 0.3, 1.0, 0)[3] is None and ops.mrspec_args((128, 256), 0.3, 1.0, 2)[3] == (2.0, 2.0)
    assert ops.mrspec_args([128, 256], 0.3, 1.0, [1, 3])[3] == (1.0, 3.0)
    m = MultiResSpecLoss([128, 256], 0.3, 1000.0, 1000.0)
    assert m.n_ffts == (128, 256) and m.gamma == 0.3 and m.f == 1000.0 and m.f_complex == (1000.0, 1000.0)
    for kw, word in [(dict(n_ffts=(100,)), "n_ffts"), (dict(n_ffts=(64,)), "n_ffts"), (dict(n_ffts=(4096,)), "n_ffts"), (dict(n_ffts=()), "n_ffts"),
                     (dict(n_ffts=(128,) * 9), "n_ffts"), (dict(n_ffts=128), "n_ffts"), (dict(gamma=0.0), "gamma"), (dict(gamma=-0.3), "gamma"),
                     (dict(n_ffts=(128, 256), f_complex=[1.0]), "f_complex")]:
        with pytest.raises(ValueError, match=word):
            multi_res_spec_loss(**kw)
        with pytest.raises(ValueError, match=word):
            MultiResSpecLoss(**dict(dict(n_ffts=(128,), gamma=0.3, factor=1.0), **kw))


def test_config_loads_and_names_the_loss():
    import importlib.util
    import train_base.loss as TL
    spec = importlib.util.spec_from_file_location("train_stand", os.path.join(ROOT, "tools", "train_stand.py"))
    ts = importlib.util.module_from_spec(spec); spec.loader.exec_module(ts)
    cfg = ts.load_toml(os.path.join(ROOT, "configs", "cruse_mrspec.toml"))
    lf = cfg["loss_function"]
    assert lf["name"] == "multi_res_spec_loss" and lf["args"] == dict(n_ffts=[128, 256, 512], gamma=0.3, factor=1.0, f_complex=1.0)
    tag = getattr(TL, lf["name"])(**lf["args"]).cruse_loss
    assert tag[0] == "mrspec" and tag[1]["mrs_ffts"] == (128, 256, 512) and tag[1]["mrs_f_complex"] == (1.0, 1.0, 1.0)
