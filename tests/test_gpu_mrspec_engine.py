"""GPU: the engine loss "mrspec"  -- one training step against the oracle chain enhanced spectrum -> iSTFT ->
tests/mrspec_ref.py, the captured step against the eager one, and a TOML run through tools/train_stand.py."""
import math

import pytest
import torch

import mrspec_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

N_FFTS, GAMMA, FACTOR, F_COMPLEX = (128, 256, 512), 0.3, 1000.0, 1000.0


def _oracle_and_product(grp):
    from cruse_amd.model import cruse_net as M
    from oracle import cruse_oracle as O
    o = O.unet_2(rnn_groups=grp); O.closed_form_init(o)
    m = M.unet_2(rnn_groups=grp, precision="f32")
    m.load_state_dict(o.state_dict(), strict=True)
    return o, m.cuda()


def _engine(m, use_graph, lr=1e-3):
    from cruse_amd.engine import TrainEngine
    return TrainEngine(m, lr=lr, use_graph=use_graph, loss="mrspec", mrs_ffts=N_FFTS, mrs_gamma=GAMMA, mrs_factor=FACTOR,
                       mrs_f_complex=F_COMPLEX)


def test_mrspec_training_step_vs_oracle():
    """waveform in -> waveform loss: STFT -> unet_2 -> mask -> iSTFT -> multi-resolution spectral loss and all gradients"""
    from oracle import cruse_oracle as O
    o, m = _oracle_and_product(1)
    eng = _engine(m, False)
    o.train()
    noisy, clean = O.synth_pair(2, 3200, seed=93)
    _, est, _ = O.enhanced_spectrum(o, noisy)
    spec = torch.view_as_complex(est.contiguous()).transpose(1, 2)          # [B,F,T]
    wave = O.istft(spec, 320, 160, 320, length=noisy.shape[1])
    loss = R.mrspec_loss(wave, clean, N_FFTS, GAMMA, FACTOR, F_COMPLEX)
    loss.backward()
    ls = eng.step(noisy.cuda(), clean.cuda())
    got, want = eng.loss_value(ls), float(loss.detach())
    print(f"[mrspec engine] loss {got:.7g} vs oracle {want:.7g}")
    assert abs(got - want) <= 1e-4 * abs(want)
    for n, po in o.named_parameters():
        if n in eng.flat.G and not (n.endswith(".bias") and n.startswith("conv") and n != "conv1_t.bias"):
            assert rel_l2(eng.flat.G[n], po.grad) <= 5e-3, n
    # validation: the same loss without gradients, finite
    assert math.isfinite(eng.eval_loss(noisy.cuda(), clean.cuda()))


def test_mrspec_graph_step_gives_the_eager_loss_bits():
    """Two steps on two different batches, launched eagerly and from the captured graph (the second graph step is a replay with new
    inputs): the same loss bits, step for step.
    The steps run with lr = 0.  The engine's forward and loss are bit-identical from run to run, its GRADIENTS are not (DESIGN section 2:
    the f64 atomics of the BatchNorm backward sums land in run-dependent order, ~2e-7), so the loss AFTER an update repeats only to ~1e-8
    between any two runs of any loss, eager or not.  Measured with lr = 1e-3, step 2 (step 1 has equal bits everywhere): "mrspec" eager
    207.38142174268432 / 207.3814213263904, graph 207.38142199155845 / 207.38142181525473; "si_snr" eager 8.272200068649969 /
    8.272199954995937, graph 8.272200110084656; "wo_male" eager 0.363540658194553 / 0.3635406618416133.  With the weights held, a difference in a step's loss bits can only come from
    what the graph replays: the forward, the iSTFT and the loss kernels of this file's subject."""
    from oracle import cruse_oracle as O
    batches = [O.synth_pair(2, 3200, seed=s) for s in (93, 94)]
    losses = {}
    for use_graph in (False, True):
        _, m = _oracle_and_product(1)
        eng = _engine(m, use_graph, lr=0.0)
        losses[use_graph] = [eng.loss_value(eng.step(noisy.cuda(), clean.cuda())) for noisy, clean in batches]
    print(f"[mrspec engine] eager {losses[False]} graph {losses[True]}")
    assert all(math.isfinite(v) for v in losses[True]) and losses[True][0] != losses[True][1]
    assert losses[True] == losses[False], losses


def test_train_stand_runs_the_mrspec_config(tmp_path):
    from test_gpu_trainer import _cli, _port, _write
    args = "[loss_function.args]\nn_ffts = [128, 256, 512]\ngamma = 0.3\nfactor = 1.0\nf_complex = 1.0"
    cfg = _write(tmp_path, "l_mrspec", loss="multi_res_spec_loss", loss_args=args, epochs=1, port=_port(29561))
    out = _cli(cfg, port=_port(29561))
    assert "[epoch 1] loss" in out and "validation loss" in out
    assert math.isfinite(float(out.split("[epoch 1] loss")[1].split()[0]))
    assert math.isfinite(float(out.split("validation loss")[1].split()[0]))
