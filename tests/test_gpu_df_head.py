"""GPU: the DeepFilter head at inference -- cruse_df_head_apply (csrc/df_head.hip, ops.df_head_apply) against the two launches it
replaces and against the float64 restatement, its guards, and the layers above it: loss.deepfilter_spectrum,
Inferencer(head="df"), evaluate_files(head="df") and the Trainer's validation of a wo_male_df run."""
import ctypes
import functools
import os
import wave

import numpy as np
import pytest
import torch

from tests import df_head_ref as R
from tests.util import bits, embed, embed_out, has_poison, poison_, rel_l2, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TILE_FRAMES = 16          # DH_TF of csrc/df_head.hip: R.CASES has T = 15, 16, 17 (below, at, above) and 33 (a third tile)
TILE_BINS = 192           # DH_FW: Fs = 200 takes two bin tiles
# the composition's deepfilter kernel takes a bin half-width of 8 at most (it sees the axes exchanged); this one reaches the head's own
# limits, asks for more than 48 KB of LDS, and is compared against the restatement only
REF_ONLY = [(3, 200, 199, 8, 16)]
COMPOSED = [c for c in R.CASES if c not in REF_ONLY]
assert {15, 16, 17} <= {c[0] for c in COMPOSED} and TILE_FRAMES == 16 and any(c[1] > TILE_BINS for c in COMPOSED)


def _dev(case):
    T, Fs, Fn, _, _ = case
    return tuple(torch.from_numpy(a).cuda() for a in R.case_data(T, Fs, Fn))


def _composition(mask, nre, nim, td, fd):
    """engine._deepfilter_loss's forward: the mask padded against a plane of ones and one of zeros, then the four-plane complex
    kernel on the [B,T,Fs] views with the roles of its two axes (and half-widths) exchanged"""
    from cruse_amd import ops
    Bn, T, Fs = nre.shape
    rows, Fn = Bn * T, mask.shape[-1]
    ones, zeros = torch.ones(rows, Fs, device="cuda"), torch.zeros(rows, Fs, device="cuda")
    hr, _ = ops.mask_apply(mask, ones, zeros, rows, Fn, Fs)
    return ops.deepfilter_fwd(nre, nim, hr.view(Bn, T, Fs), zeros.view(Bn, T, Fs), td, fd)


@functools.lru_cache(maxsize=None)
def kernel(case):
    """the kernel's result for one case, computed once and shared (never written to)"""
    from cruse_amd import ops
    mask, nre, nim = _dev(case)
    return ops.df_head_apply(mask, nre, nim, case[3], case[4])


@pytest.mark.parametrize("case", COMPOSED, ids=lambda c: "T%d_F%d_%d_d%d_%d" % c)
def test_kernel_has_the_bits_of_the_composition(case):
    mask, nre, nim = _dev(case)
    want = _composition(mask, nre, nim, case[3], case[4])
    got = kernel(case)
    for g, w, name in zip(got, want, ("real", "imag")):
        assert g.shape == w.shape == (R.B, case[0], case[1])
        diff = int((bits(g) != bits(w)).sum())
        print(f"{case} {name}: {diff} of {g.numel()} words differ")
        assert diff == 0, (case, name, diff)


@pytest.mark.parametrize("case", COMPOSED + REF_ONLY, ids=lambda c: "T%d_F%d_%d_d%d_%d" % c)
def test_kernel_against_the_float64_restatement(case):
    T, Fs, Fn, td, fd = case
    want = R.df_head(*R.case_data(T, Fs, Fn), td, fd)
    got = kernel(case)
    for g, w, name in zip(got, want, ("real", "imag")):
        err = rel_l2(g, torch.from_numpy(w))
        print(f"{case} {name}: rel-L2 {err:.3e}")
        assert err <= 1e-6, (case, name, err)
    if Fn < Fs and td == 0 and fd == 0:
        assert not bool(got[0][..., Fn:].any()) and not bool(got[1][..., Fn:].any())      # the bare product: a zero Nyquist bin (R8)


@pytest.mark.parametrize("case", [(17, 161, 160, 1, 5), (3, 200, 199, 2, 5), (2, 9, 8, 1, 5)], ids=lambda c: "T%d_F%d_%d_d%d_%d" % c)
def test_poisoned_outputs_are_written_in_full_and_nothing_around_them(case):
    from cruse_amd import ops
    T, Fs, Fn, td, fd = case
    mask, nre, nim = _dev(case)
    want = kernel(case)
    # outputs inside larger poisoned allocations, pre-filled with NaN
    ere, ck_r = embed_out((R.B, T, Fs))
    eim, ck_i = embed_out((R.B, T, Fs))
    ops.df_head_apply(mask, nre, nim, td, fd, out=(ere, eim))
    torch.cuda.synchronize()
    assert not has_poison(ere) and not has_poison(eim)
    assert same_bits(ere, want[0]) and same_bits(eim, want[1])
    ck_r("ere"); ck_i("eim")
    # operands at the very tail of their allocations (poison in front): the same bits, the operands untouched
    ops_in = [embed(x, lead=32, trail=0) for x in (mask, nre, nim)]
    got = ops.df_head_apply(*(v for v, _ in ops_in), td, fd)
    torch.cuda.synchronize()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    for (_, ck), name in zip(ops_in, ("mask", "nre", "nim")):
        ck(name)
    # the wrapper's own allocations hold NaN where the kernel does not write
    from tests.util import poisoned_empty
    with poisoned_empty():
        again = ops.df_head_apply(mask, nre, nim, td, fd)
    assert same_bits(again[0], want[0]) and same_bits(again[1], want[1])


def test_graph_replay_equals_the_eager_bits():
    from cruse_amd import ops
    case = (33, 161, 160, 1, 5)
    mask, nre, nim = _dev(case)
    want = kernel(case)
    ere, eim = poison_(torch.empty_like(nre)), poison_(torch.empty_like(nre))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.df_head_apply(mask, nre, nim, 1, 5, out=(ere, eim))          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.df_head_apply(mask, nre, nim, 1, 5, out=(ere, eim))
    for _ in range(2):
        poison_(ere); poison_(eim)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(ere, want[0]) and same_bits(eim, want[1])


def test_refusals_come_before_any_launch():
    from cruse_amd import ops
    from cruse_amd._lib import lib
    Bn, T, Fs, Fn = 2, 3, 161, 160
    mask, nre, nim = _dev((T, Fs, Fn, 1, 5))
    ere, eim = torch.full_like(nre, 7.0), torch.full_like(nre, 7.0)
    P = lambda x: ctypes.c_void_p(x.data_ptr())                           # noqa: E731
    ok = dict(mask=P(mask), nre=P(nre), nim=P(nim), B=Bn, T=T, Fn=Fn, Fs=Fs, t_dim=1, f_dim=5, ere=P(ere), eim=P(eim))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cruse_df_head_apply(a["mask"], a["nre"], a["nim"], a["B"], a["T"], a["Fn"], a["Fs"], a["t_dim"], a["f_dim"], a["ere"],
                                       a["eim"], None)
    bad = [dict(B=0), dict(B=-1), dict(T=0), dict(Fn=0), dict(Fs=0), dict(Fs=-3), dict(Fn=Fs + 1), dict(t_dim=9), dict(f_dim=17),
           dict(t_dim=-1), dict(f_dim=-1), dict(mask=None), dict(nre=None), dict(nim=None), dict(ere=None), dict(eim=None)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"df_head_apply" in lib.cruse_last_error(), kw
    with pytest.raises(RuntimeError, match="df_head_apply"):
        ops.df_head_apply(torch.zeros(Bn * T, Fs + 1, device="cuda"), nre, nim, out=(ere, eim))       # Fn > Fs through the wrapper
    with pytest.raises(RuntimeError, match="df_head_apply"):
        ops.df_head_apply(mask, nre, nim, t_dim=9, out=(ere, eim))
    with pytest.raises(RuntimeError, match="df_head_apply"):
        ops.df_head_apply(mask[:-1], nre, nim, out=(ere, eim))                                       # not B*T rows
    torch.cuda.synchronize()
    assert bool((ere == 7.0).all()) and bool((eim == 7.0).all())          # nothing was launched
    assert call() == 0                                                    # ... and the same arguments, unspoiled, are accepted
    torch.cuda.synchronize()
    want = kernel((T, Fs, Fn, 1, 5))
    assert same_bits(ere, want[0]) and same_bits(eim, want[1])


def test_deepfilter_spectrum_stacks_the_kernel_planes():
    from cruse_amd.loss import deepfilter_spectrum, enhanced_spectrum
    case = (17, 161, 160, 1, 5)
    mask, nre, nim = _dev(case)
    want = kernel(case)
    est = deepfilter_spectrum(mask.view(R.B, 1, 17, 160), nre, nim)
    assert est.shape == (R.B, 17, 161, 2) and same_bits(est[..., 0].contiguous(), want[0]) and same_bits(est[..., 1].contiguous(), want[1])
    # half-widths (0, 0) are the mask applied in place: enhanced_spectrum's planes
    plain = deepfilter_spectrum(mask.view(R.B, 1, 17, 160), nre.unsqueeze(1), nim.unsqueeze(1), 0, 0)
    assert torch.equal(plain, enhanced_spectrum(mask.view(R.B, 1, 17, 160), nre, nim))
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        deepfilter_spectrum(mask.view(R.B, 1, 17, 160), nre[:, :16], nim)


def test_wo_male_df_loss_stand_alone_gives_the_oracle_value():
    """the factory's callable outside the engine: WO-MALE of the oracle on the float64 head output.  Bar 1e-5 relative: the terms are
    f32 sqrt / exp / log10 expressions (a few 1e-7 each) of an estimate itself within 1e-6, summed in f64; test_gpu_extras gives
    the plain rmse loss value the same bar"""
    import train_base.loss as TL
    from oracle import cruse_oracle as O
    case = (17, 161, 160, 1, 5)
    mask, nre, nim = _dev(case)
    clean = torch.randn(R.B, 2, 17, 161, generator=torch.Generator().manual_seed(3))
    noisy = torch.stack([nre, nim], dim=1)                               # [B,2,T,Fs]
    got = float(TL.wo_male_df_loss(alpha=2.0, beta=1.0)(mask.view(R.B, 1, 17, 160), noisy, clean.cuda()))
    est = torch.stack([torch.from_numpy(p) for p in R.df_head(*R.case_data(17, 161, 160), 1, 5)], dim=1)
    want = float(O.wo_male(clean.double(), est, noisy.cpu().double(), 2.0, 1.0))
    print(f"wo_male_df_loss stand-alone {got!r}, oracle {want!r}")
    assert abs(got - want) <= 1e-5 * abs(want)


# ---- Inferencer ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_and_product(grp):
    from cruse_amd.model import cruse_net as M
    from oracle import cruse_oracle as O
    o = O.unet_2(rnn_groups=grp)
    O.closed_form_init(o)
    o.eval()
    m = M.unet_2(rnn_groups=grp, precision="f32")
    m.load_state_dict(o.state_dict(), strict=True)
    return o, m.cuda().eval()


@functools.lru_cache(maxsize=None)
def oracle_waves(grp, L):
    """the oracle on the CPU: pre_stft -> unet_2 -> train_step_loss_df's head (zero-padded mask, DeepFilter(1, 5)) -> istft, and the
    magnitude-mask waveform of the same mask -> (noisy [1,L], df waveform, mask waveform)"""
    from oracle import cruse_oracle as O
    o, _ = oracle_and_product(grp)
    noisy, _ = O.synth_pair(1, L, seed=123)
    with torch.no_grad():
        f = O.pre_stft(noisy, 320, 160, 320, f_net=160)
        mask = o(f["mag_net"])
        Fs = f["real"].shape[-1]
        h_r = torch.nn.functional.pad(mask, (0, Fs - 160)).squeeze(1).transpose(1, 2)              # [B,F,T]
        x_r, x_i = f["real"].squeeze(1).transpose(1, 2), f["imag"].squeeze(1).transpose(1, 2)
        y = O.DeepFilter(1, 5)([x_r, x_i], [h_r, torch.zeros_like(h_r)])
        df = O.istft(torch.complex(y[:, :Fs], y[:, Fs:]), 320, 160, 320, length=L)
        mk = O.istft(torch.complex(x_r * h_r, x_i * h_r), 320, 160, 320, length=L)
    return noisy, df, mk


@pytest.mark.parametrize("L", [3200, 4000])
@pytest.mark.parametrize("grp", [1, 4])
def test_inferencer_df_head_matches_the_oracle_waveform(grp, L):
    from cruse_amd.inferencer import Inferencer
    _, m = oracle_and_product(grp)
    noisy, want, want_mask = oracle_waves(grp, L)
    inf = Inferencer(m, head="df")
    assert inf.head == "df" and inf.df_dims == (1, 5)
    got = inf.mag_mask_to_wave(noisy.cuda())
    err = rel_l2(got, want)
    print(f"groups {grp} L {L}: head=df rel-L2 {err:.3e} against the oracle")
    assert got.shape == noisy.shape and err <= 1e-4
    # the head is really applied.  The oracle's own two waveforms are 1.47 .. 1.53 apart in rel-L2 (closed_form_init, seed 123:
    # 1.530 / 1.471 for groups 1, 1.530 / 1.473 for groups 4 at L = 3200 / 4000), far above 100 x the 1e-4 bar
    far = rel_l2(want, want_mask)
    assert far > 1e-2, far
    plain = Inferencer(m, head="mask").mag_mask_to_wave(noisy.cuda())
    assert rel_l2(got, plain) > 1e-2 and rel_l2(plain, want_mask) <= 1e-4
    assert same_bits(plain, Inferencer(m).mag_mask_to_wave(noisy.cuda()))                           # the default runs what it ran
    # atten_lim_db and __call__ work with this head
    lim = Inferencer(m, head="df", atten_lim_db=12.0)
    mixed = lim.mag_mask_to_wave(noisy.cuda())
    assert rel_l2(mixed, lim.lim * noisy + (1.0 - lim.lim) * want) <= 1e-4
    res = inf([(noisy, ["clip0"])], log=lambda *_: None)
    assert res[0][0] == "clip0" and 0 < res[0][1] < 10.0


def test_inferencer_refuses_an_unknown_head():
    from cruse_amd.inferencer import Inferencer
    _, m = oracle_and_product(1)
    with pytest.raises(ValueError, match="head"):
        Inferencer(m, head="deepfilter")


# ---- evaluate_files ------------------------------------------------------------------------------------------------------------
def _write_wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())


def test_evaluate_files_scores_the_df_head(tmp_path):
    from cruse_amd import metrics
    from cruse_amd.evaluate import evaluate_files
    from cruse_amd.filepairs import load_pool
    from cruse_amd.inferencer import Inferencer
    from oracle import cruse_oracle as O
    _, m = oracle_and_product(1)
    clean, noisy = [], []
    for k, L in enumerate((4000, 4800)):
        n, c = O.synth_pair(1, L, seed=40 + k)
        for side, x, lst in (("clean", c, clean), ("noisy", n, noisy)):
            lst.append(str(tmp_path / f"{side}{k}.wav"))
            _write_wav(lst[-1], x[0].numpy())
    res = evaluate_files(m, clean, noisy, metrics=["SI_SDR"], batch_size=1, head="df")
    res_mask = evaluate_files(m, clean, noisy, metrics=["SI_SDR"], batch_size=1, head="mask")
    assert res["lengths"].tolist() == [4000, 4800]
    inf = Inferencer(m, head="df")
    pool, start, lens, _ = load_pool(clean + noisy, "cuda")              # the clips as evaluate_files reads them
    for i in range(2):
        c, x = (pool[start[k]:start[k] + lens[k]].reshape(1, -1).contiguous() for k in (i, 2 + i))
        want = float(metrics.si_sdr(c, inf.mag_mask_to_wave(x))[0])
        got = float(res["scores"]["SI_SDR"]["Enhanced"][i])
        print(f"pair {i}: SI_SDR enhanced head=df {got!r} (by hand {want!r}), head=mask {float(res_mask['scores']['SI_SDR']['Enhanced'][i])!r}")
        assert got == want                                               # batch_size = 1: the clip alone, bit for bit
    assert np.array_equal(res["scores"]["SI_SDR"]["Noisy"], res_mask["scores"]["SI_SDR"]["Noisy"])
    assert (np.abs(res["scores"]["SI_SDR"]["Enhanced"] - res_mask["scores"]["SI_SDR"]["Enhanced"]) > 0.1).all()
    assert np.array_equal(res_mask["scores"]["SI_SDR"]["Enhanced"],
                          evaluate_files(m, clean, noisy, metrics=["SI_SDR"], batch_size=1)["scores"]["SI_SDR"]["Enhanced"])


# ---- Trainer -------------------------------------------------------------------------------------------------------------------
TOML = '''
[meta]
seed = 0
save_dir = "{save_dir}"
use_amp = false
precision = "f32"
hip_graph = false
[acoustics]
n_fft = 320
hop_length = 160
win_length = 320
sr = 16000
[train_dataset]
path = "cruse_amd.data.SyntheticPairs"
[train_dataset.args]
num = 4
length = 3200
seed = 1
[train_dataset.dataloader]
batch_size = 2
num_workers = 0
drop_last = true
[validation_dataset]
path = "cruse_amd.data.SyntheticPairs"
[validation_dataset.args]
num = 2
length = 3200
seed = 2
[model]
path = "model.cruse_net.unet_2"
[model.args]
in_feat = 161
rnn_groups = 2
[optimizer]
lr = 0.001
beta1 = 0.9
beta2 = 0.999
[loss_function]
name = "{loss}"
[loss_function.args]
alpha = 2.0
beta = 1.0
[trainer]
path = "train.trainer_casual.Trainer"
[trainer.train]
epochs = 1
save_checkpoint_interval = 1
clip_grad_norm_value = 10.0
[trainer.validation]
validation_interval = 1
metrics = ["SI_SDR"]
save_max_metric_score = true
'''


def _trainer_from_toml(tmp_path, loss, model=None, only_validation=False):
    """what tools/train_stand.py's entry() builds from the config, in this process and without a process group"""
    import train_base.loss as TL
    from torch.utils.data import DataLoader
    from tools.train_stand import load_toml
    from train_base.utils import initialize_module
    path = tmp_path / f"{loss}.toml"
    path.write_text(TOML.format(save_dir=str(tmp_path / "runs"), loss=loss))
    cfg = load_toml(str(path))
    cfg["meta"]["experiment_name"] = loss
    torch.manual_seed(cfg["meta"]["seed"])
    train = DataLoader(initialize_module(cfg["train_dataset"]["path"], args=cfg["train_dataset"]["args"]), shuffle=False,
                       **cfg["train_dataset"]["dataloader"])
    valid = DataLoader(initialize_module(cfg["validation_dataset"]["path"], args=cfg["validation_dataset"]["args"]), num_workers=0, batch_size=1)
    if model is None:
        model = initialize_module(cfg["model"]["path"], args=cfg["model"]["args"])
    opt = torch.optim.Adam(params=model.parameters(), lr=cfg["optimizer"]["lr"], betas=(cfg["optimizer"]["beta1"], cfg["optimizer"]["beta2"]))
    loss_fn = getattr(TL, cfg["loss_function"]["name"])(**cfg["loss_function"].get("args", {}))
    cls = initialize_module(cfg["trainer"]["path"], initialize=False)
    tr = cls(dist=None, rank=0, config=cfg, resume=False, only_validation=only_validation, model=model, loss_function=loss_fn, optimizer=opt,
             train_dataloader=train, validation_dataloader=valid)
    return tr, valid


def _mean_si_sdr(inf, loader):
    from cruse_amd import metrics
    per = []
    for noisy, clean in loader:
        noisy, clean = noisy.cuda().float().contiguous(), clean.cuda().float().contiguous()
        per += metrics.si_sdr(clean, inf.mag_mask_to_wave(noisy)).tolist()
    return float(np.mean(per)), len(per)


def test_trainer_trains_and_validates_a_deepfilter_run_from_toml(tmp_path, monkeypatch, capsys):
    import cruse_amd.inferencer as I
    built = []

    class Spy(I.Inferencer):
        def __init__(self, *a, **k):
            built.append(k.get("head", "mask"))
            super().__init__(*a, **k)
    monkeypatch.setattr(I, "Inferencer", Spy)
    tr, valid = _trainer_from_toml(tmp_path, "wo_male_df_loss")
    assert tr.engine.loss == "wo_male_df" and tr.engine.loss_alpha == 2.0 and tr.validation_head == "df"
    tr.train()                                                           # 2 steps, then one scored validation epoch
    out = capsys.readouterr().out
    assert "[epoch 1] loss" in out and "validation SI_SDR: Noisy" in out and "validation score (SI_SDR, enhanced)" in out
    assert built == ["df"]
    ck = torch.load(tmp_path / "runs" / "wo_male_df_loss" / "checkpoints" / "latest_model.tar", map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "best_score", "optimizer", "scaler", "model"}                        # the schema is unchanged
    assert float(ck["optimizer"]["state"][0]["step"]) == 2.0
    monkeypatch.undo()
    want, n = _mean_si_sdr(I.Inferencer(tr.model, head="df"), valid)
    got = tr.last_metric_means["SI_SDR"]["Enhanced"]
    plain, _ = _mean_si_sdr(I.Inferencer(tr.model), valid)
    print(f"validation SI_SDR enhanced: trainer {got!r}, Inferencer(head='df') {want!r}, Inferencer(head='mask') {plain!r}")
    assert n == 2 and abs(got - want) <= 1e-4 and abs(ck["best_score"] - got) <= 1e-9
    assert abs(got - plain) > 0.1                                        # ... and not the magnitude-mask audio
    # a wo_male run of the same model still scores the magnitude-mask audio
    monkeypatch.setattr(I, "Inferencer", Spy)
    del built[:]
    tr2, valid2 = _trainer_from_toml(tmp_path, "wo_male_loss", model=tr.model, only_validation=True)
    assert tr2.engine.loss == "wo_male" and tr2.validation_head == "mask"
    tr2.model.eval()
    tr2._validation_epoch(1)
    assert built == ["mask"]
    assert abs(tr2.last_metric_means["SI_SDR"]["Enhanced"] - plain) <= 1e-4
