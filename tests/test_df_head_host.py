"""Host: the float64 restatement of the DeepFilter head (tests/df_head_ref.py) against the oracle's DeepFilter module fed
[pad(mask), 0] as oracle.cruse_oracle_ext.train_step_loss_df feeds it, and the host-side surface of the feature: the loss tag,
the Inferencer's head argument, the header."""
import os
import re

import numpy as np
import pytest
import torch

from tests import df_head_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _oracle(mask, nre, nim, t_dim, f_dim):
    """train_step_loss_df's head in float64: filters = [pad(mask, Fs bins), 0], inputs = [Re N, Im N] as [B,F,T] -> (ere, eim) [B,T,Fs]"""
    from oracle import cruse_oracle as O
    Bn, T, Fs = nre.shape
    m = torch.from_numpy(mask).double().view(Bn, T, -1)
    h_r = torch.nn.functional.pad(m, (0, Fs - m.shape[-1])).transpose(1, 2)
    x_r, x_i = (torch.from_numpy(p).double().transpose(1, 2) for p in (nre, nim))
    y = O.DeepFilter(t_dim, f_dim).double()([x_r, x_i], [h_r, torch.zeros_like(h_r)])
    return y[:, :Fs].transpose(1, 2).numpy(), y[:, Fs:].transpose(1, 2).numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def test_restatement_equals_the_oracle_head_on_random_data():
    rng = np.random.default_rng(3)
    mask = rng.uniform(0.0, 1.0, (2 * 7, 160)).astype(np.float32)
    nre, nim = (rng.standard_normal((2, 7, 161)).astype(np.float32) for _ in range(2))
    got, want = R.df_head(mask, nre, nim, 1, 5), _oracle(mask, nre, nim, 1, 5)
    for g, w in zip(got, want):
        assert g.shape == (2, 7, 161) and _rel(g, w) <= 1e-12, _rel(g, w)
    # the Nyquist bin of the product is zero (R8): bin 160 sums bins 155 .. 159 only, and the head is not the mask applied in place
    prod = mask.reshape(2, 7, 160).astype(np.float64) * nre[..., :160].astype(np.float64)
    assert np.allclose(got[0][:, 3, 160], prod[:, 2:5, 155:160].sum(axis=(1, 2)), rtol=1e-12, atol=0)
    assert _rel(got[0][..., :160], prod) > 0.5


@pytest.mark.parametrize("T,Fs,Fn,td,fd", R.DEGENERATE + [c for c in R.CASES if c not in R.DEGENERATE])
def test_restatement_equals_the_oracle_head_at_the_test_shapes(T, Fs, Fn, td, fd):
    mask, nre, nim = R.case_data(T, Fs, Fn)
    got, want = R.df_head(mask, nre, nim, td, fd), _oracle(mask, nre, nim, td, fd)
    for g, w in zip(got, want):
        assert g.shape == (R.B, T, Fs) and _rel(g, w) <= 1e-12, _rel(g, w)


def test_wo_male_df_loss_carries_the_engine_tag():
    import train_base.loss as L
    assert L.wo_male_df_loss(alpha=3.0).cruse_loss == ("wo_male_df", {"loss_alpha": 3.0, "loss_beta": 1.0})
    assert L.wo_male_df_loss().cruse_loss == ("wo_male_df", {"loss_alpha": 2.0, "loss_beta": 1.0})
    assert L.wo_male_loss().cruse_loss == ("wo_male", {"loss_alpha": 2.0, "loss_beta": 1.0})        # (its neighbour is untouched)


def test_inferencer_refuses_an_unknown_head_before_moving_the_model():
    from cruse_amd.inferencer import Inferencer

    class Model(torch.nn.Module):
        moved = False

        def to(self, *a, **k):
            Model.moved = True
            return self
    with pytest.raises(ValueError, match="head"):
        Inferencer(Model(), head="x", device="cpu")
    with pytest.raises(ValueError, match="df_dims"):
        Inferencer(Model(), head="df", df_dims=(9, 5), device="cpu")
    assert not Model.moved


def test_header_declares_the_entry_point_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert re.search(r"#define\s+CRUSE_ABI_VERSION\s+15\b", text)
    decl = re.search(r"int\s+cruse_df_head_apply\s*\(([^;]*)\)\s*;", text)
    assert decl, "include/cruse_hip.h does not declare cruse_df_head_apply"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 12 and args[0] == "const float* mask" and args[-1] == "void* stream"
    assert "df_head" in open(os.path.join(ROOT, "cruse_amd", "csrc", "build.sh")).read()
