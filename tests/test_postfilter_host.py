"""CPU: the perceptual post-filter -- what can be pinned without a GPU: the float64 restatement of the two closed forms against the outputs
of the reference's own postfiltering / envelope_postfiltering (tests/golden/postfilter.npz), the properties of the closed forms, the C
entry points, the Python keywords and the utils.utils shim."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import postfilter_ref as P
from tests import stream_io_ref as IO
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cruse_stream_decode_pf", "cruse_stream_decode_n_pf", "cruse_mask_postfilter")
EPS = np.finfo(np.float64).eps


def golden():
    path = os.path.join(ROOT, "tests", "golden", "postfilter.npz")
    assert os.path.getsize(path) <= 20 * 1024
    z = np.load(path)
    g, u, tau = z["g"], z["u"], z["tau"]
    assert g.shape == u.shape == (512,) and g.dtype == u.dtype == np.float64 and tau.tolist() == [0.02, 0.1]
    assert g.min() == 1e-3 and g.max() == 1.0 and u.min() == 1e-3 and u.max() == 10.0
    return g, u, tau, z["iam"], z["envelope"]


def test_iam_restatement_matches_the_reference():
    g, _, tau, iam, _ = golden()
    for j, t in enumerate(tau):
        err = float(np.abs(P.pf(g, t, "iam") / iam[j] - 1.0).max())
        print(f"iam, tau {t}: restatement vs the reference's postfiltering, worst relative {err:.2e}")
        assert err <= 1e-12


def test_envelope_restatement_matches_the_reference_up_to_its_eps_term():
    """The reference's tmp = g u / (g s u + eps) is (1 / s) (1 - d + O(d^2)), d = eps / (g s u), where the closed form has 1 / s.  With
    ln G = (ln tmp - ln(1 + tau tmp^2)) / 2 + const the returned value moves by the relative amount c d, c = (1 - tau / s^2) / (2 (1 + tau /
    s^2)), |c| <= 1 / 2.  So: the restatement with that first-order term restored matches to 1e-12 (d^2 < 2e-14), and without it the
    residual is at most d at the fixture's smallest g and smallest u, which is the bound asserted."""
    g, u, tau, _, env = golden()
    s = np.sin(0.5 * np.pi * g)
    d = EPS / (g * s * u)
    bound = EPS / (g.min() * np.sin(0.5 * np.pi * g.min()) * u.min())
    assert 1.4e-7 < bound < 1.5e-7 and d.max() <= bound
    for j, t in enumerate(tau):
        e = P.pf(g, t, "envelope")
        res = float(np.abs(e / env[j] - 1.0).max())
        c = (1.0 - t / s ** 2) / (2.0 * (1.0 + t / s ** 2))
        err = float(np.abs(e * (1.0 - c * d) / env[j] - 1.0).max())
        print(f"envelope, tau {t}: residual of the dropped eps term {res:.2e} (bound eps / (g s u) at the smallest inputs {bound:.2e}, largest "
              f"d of the fixture {d.max():.2e}); with the first-order term restored {err:.2e}")
        assert res <= bound
        assert err <= 1e-12


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("tau", [0.02, 0.1, 0.5, 1e-6, 10.0])
def test_properties_on_the_sweep(kind, tau):
    g = P.sweep(4097)
    for v in (0.0, 1e-30, 1e-4, 0.5, 1.0 - 2.0 ** -24, 1.0):
        assert v in g
    f = P.pf(g, tau, kind)
    assert f.shape == (4097,) and np.isfinite(f).all()
    assert f[0] == 0.0 and abs(f[-1] - 1.0) <= 4 * EPS
    assert (f <= g * (1.0 + 4 * EPS)).all()
    assert (np.diff(f) >= -4 * EPS).all()
    assert (f >= 0.0).all()


@pytest.mark.parametrize("kind", P.KINDS)
def test_tau_zero_is_the_identity(kind):
    g = P.sweep(4097)
    assert np.array_equal(P.pf(g, 0.0, kind), g)


def test_the_filter_separates_on_the_test_clips():
    """the GPU module asserts that slots with tau > 0 differ from the plain server by rel-L2 > 1e-3: the float64 reference says so first"""
    o = IO.oracle("hg20_g1")
    clips = IO.clips()
    for s, tau in ((0, 0.02), (2, 0.2)):
        fr = P.frames64(o, clips[s])
        plain = P.e64_pf(fr, 0.0, "iam")
        assert rel_l2(plain, IO.e64(o, clips[s])) < 1e-12             # tau 0: the unfiltered chain itself
        for kind in P.KINDS:
            d = rel_l2(P.e64_pf(fr, tau, kind), plain)
            print(f"slot {s} {kind} tau {tau}: filtered vs unfiltered float64 reference, rel-L2 {d:.2e}")
            assert d > 1e-3
    assert torch.equal(P.mix(clips[0], plain, 1.0), clips[0].double())


def test_entry_points_declared_and_bound():
    from cruse_amd import _lib
    from cruse_amd._abi_check import parse_header
    header = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    parsed = parse_header()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\bint {sym}\(", header), f"{sym} is not declared in include/cruse_hip.h"
        assert _lib.SIGNATURES[sym] == parsed[sym], (sym, _lib.SIGNATURES[sym], parsed[sym])
        assert getattr(_lib.lib, sym).argtypes is not None
    for sym in NEW_SYMBOLS[:2]:                                       # the _io sibling's arguments plus pf_kind and pf_tau
        sib = sym[:-3] + "_io"
        a, b = _lib.SIGNATURES[sym][0], _lib.SIGNATURES[sib][0]
        assert a == b[:-1] + "ip" + b[-1], (sym, a, b)
    assert header.count("utils/utils.py:345-362") >= 3
    assert re.search(r"^#define CRUSE_ABI_VERSION 15$", header, flags=re.M) and _lib.ABI_VERSION == 15 and _lib.lib.cruse_abi_version() == 15
    assert "postfilter" in open(os.path.join(ROOT, "cruse_amd", "csrc", "build.sh")).read()


def test_python_keywords_and_the_shim():
    from cruse_amd import ops
    from cruse_amd.evaluate import evaluate_files
    from cruse_amd.inferencer.base_inferencer import Inferencer
    from cruse_amd.inferencer.streaming import StreamingInferencer
    p = inspect.signature(StreamingInferencer.__init__).parameters
    assert p["post_filter"].default is None and hasattr(StreamingInferencer, "set_post_filter")
    q = inspect.signature(Inferencer.__init__).parameters
    assert q["post_filter"].default is None and q["pf_tau"].default == 0.02
    e = inspect.signature(evaluate_files).parameters
    assert e["post_filter"].default is None and e["pf_tau"].default == 0.02
    f = inspect.signature(ops.post_filter).parameters
    assert list(f)[:3] == ["mask", "tau", "kind"] and f["tau"].default == 0.02 and f["kind"].default == "iam"
    import utils.utils as shim
    from cruse_amd.acoustics import postfilter
    assert shim.postfiltering is postfilter.postfiltering and shim.envelope_postfiltering is postfilter.envelope_postfiltering
    assert list(inspect.signature(shim.postfiltering).parameters) == ["mask", "indata", "tao"]
    assert list(inspect.signature(shim.envelope_postfiltering).parameters) == ["unproc", "mask", "tao"]
    assert inspect.signature(shim.postfiltering).parameters["tao"].default == 0.02
    assert inspect.signature(shim.envelope_postfiltering).parameters["tao"].default == 0.02


def test_host_side_refusals():
    from cruse_amd import ops
    assert ops.post_filter_kind("iam") == 1 and ops.post_filter_kind("envelope") == 2
    for bad in ("IAM", "irm", 1, None):
        with pytest.raises(ValueError, match="kind"):
            ops.post_filter_kind(bad)
    assert ops.post_filter_tau(0) == 0.0 and ops.post_filter_tau(0.02) == 0.02
    for bad in (-1e-9, float("nan"), float("-inf"), float("inf")):
        with pytest.raises(ValueError, match="non-negative"):
            ops.post_filter_tau(bad)
    m = torch.zeros(4, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference-only"):
        ops.post_filter(m)
    with pytest.raises(ValueError, match="kind"):
        ops.post_filter(torch.zeros(4), kind="other")


def test_tools_take_the_option():
    for tool, words in (("evaluate.py", ("--post-filter", "--pf-tau")), ("stream_rtf.py", ("--post-filter", "--pf-tau"))):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        for w in words:
            assert f'"{w}"' in src, (tool, w)
