"""GPU: filepairs.DeviceFilePairs on a corpus of WAVs written into a temporary directory: the preloaded pools against
the float64 resampling of every file, a batch against the restated reference driven by the same draws, the reverb + EQ chain against
the existing float64 twins, determinism, the untouched parent, and two trainer steps on a config shaped like cruse_file_dataset.toml."""
import math
import os

import numpy as np
import pytest
import torch

import biquad_ref as BQ
import fftconv_ref as F
import filepairs_ref as R
from cruse_amd import resample_design as D
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MIX_BAR = 2e-6                     # the bar of test_gpu_extras.test_snr_mix_vs_reference (rel-L2)
STAGE_BAR = 1e-5                   # the bar of test_gpu_reverb_dataset.py for the composition with reverberation and EQ
LENGTH, SEED = 4000, 5


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return R.write_corpus(tmp_path_factory.mktemp("corpus"))


@pytest.fixture(scope="module")
def ref(corpus):
    """the float64 pools, computed once and left unchanged"""
    return {name: R.pool64(files) for name, (_, files) in corpus.items()}


def make(corpus, **kw):
    from cruse_amd.filepairs import DeviceFilePairs
    args = dict(clean_dataset=corpus["clean"][0], noise_dataset=corpus["noise"][0], rir_dataset=corpus["rir"][0], snr_range=[0, 20],
                silence_length=0.02, sub_sample_length=LENGTH / 16000, sr=16000, dataset_length=8, seed=SEED)
    args.update(kw)
    return DeviceFilePairs(**args)


def test_the_pools_are_the_resampled_files(corpus, ref):
    ds = make(corpus)
    pools = ds._ensure(dev())
    torch.cuda.synchronize()
    assert ds._ensure(dev()) is pools                                      # once per device
    for name in ("clean", "noise"):
        files, pool = corpus[name][1], pools[name].cpu().numpy()
        start, lens = getattr(ds, name + "_utt_start"), getattr(ds, name + "_utt_len")
        want_len = [D.out_len(len(pcm) // ch, *D.ratio(16000, rate)) for pcm, ch, rate in files]
        assert lens.tolist() == want_len and pool.shape == (sum(want_len),)
        order = np.argsort(start)                                          # the utterances tile the pool, group by group
        assert start[order[0]] == 0 and np.array_equal(start[order][1:], np.cumsum(lens[order])[:-1])
        rates = [files[i][2] for i in order]
        assert rates == sorted(rates)
        for i, (pcm, ch, rate) in enumerate(files):
            got = pool[start[i]:start[i] + lens[i]]
            x32 = pcm.reshape(-1, ch)[:, 0].astype(np.float32) / np.float32(32768.0)
            if rate == 16000:
                assert np.array_equal(got, x32), (name, i)                 # the conversion alone: exact
                continue
            want, b2, bm = R.bars(x32, *D.ratio(16000, rate))
            assert np.array_equal(want, ref[name][i])
            e2, em = R.errors(got, want)
            print(f"{name} {i} ({rate} Hz, {ch} ch, {lens[i]} samples): rel-L2 {e2:.2e} / {b2:.2e}, max-abs {em:.2e} / {bm:.2e}")
            assert e2 <= b2 and em <= bm, (name, i)
    groups = {(r["pool"], r["rate"], r["channels"]) for r in ds.preload_stats}
    assert groups == {(n, rate, ch) for n in ("clean", "noise") for _, ch, rate in corpus[n][1]}


def reference_batch(ds, ref, items):
    """the restated SynDataset driven by the dataset's own stream of draws: -> (clean [B, L], noise [B, L], snr [B]) float64"""
    rng = np.random.default_rng(ds.seed * 100003 + 47)
    first = rng.integers(0, len(ref["clean"]), ds.num)                     # general_mix_dataset_list (:134)
    assert np.array_equal(first, ds.general_mix_dataset_list)
    c, n, snr = [], [], []
    for i in items:
        c.append(R.select_ref(int(first[i]), ref["clean"], ds.length, ds.silence, rng))
        n.append(R.select_ref(None, ref["noise"], ds.length, ds.silence, rng))
        snr.append(ds.snr_list[int(rng.integers(len(ds.snr_list)))])
    return np.stack(c), np.stack(n), np.asarray(snr, dtype=np.float64)


def test_a_plain_batch_equals_the_restated_reference(corpus, ref):
    from cruse_amd.data import snr_mix
    ds = make(corpus)
    idx = torch.tensor([0, 4, 5])                                          # items whose plans hold silence gaps in speech and noise
    noisy, clean = ds.device_batch(idx, dev())
    torch.cuda.synchronize()
    assert noisy.shape == clean.shape == (3, LENGTH) and noisy.dtype == torch.float32
    c, n, snr = reference_batch(ds, ref, [0, 4, 5])                        # the first batch of a fresh dataset: the same stream
    assert np.array_equal(snr.astype(np.float32), ds.last_snr)
    assert (c == 0).sum() >= 320 and (n == 0).sum() >= 320 and len(ds.last_plan[0]) > 4 and len(ds.last_plan[2]) > 4       # stitched, with gaps
    want_noisy, want_clean, _ = R.snr_mix64(c, n, snr)
    e_n, e_c = rel_l2(noisy.cpu().double(), torch.from_numpy(want_noisy)), rel_l2(clean.cpu().double(), torch.from_numpy(want_clean))
    print(f"plain batch vs the float64 pipeline: noisy rel-L2 {e_n:.2e}, clean rel-L2 {e_c:.2e}")
    assert e_n <= MIX_BAR and e_c <= MIX_BAR
    # ... and, as the dataset tests take it, against snr_mix of the reference clips
    gn, gc, _ = snr_mix(torch.from_numpy(c.astype(np.float32)).cuda(), torch.from_numpy(n.astype(np.float32)).cuda(),
                        torch.from_numpy(snr.astype(np.float32)).cuda(), return_parts=True)
    assert rel_l2(noisy, gn) <= MIX_BAR and rel_l2(clean, gc) <= MIX_BAR
    assert ds.reverb_index is None and ds.aug_coefs is None                # no reverberation, no EQ drawn


def test_reverb_and_eq_match_the_chain_of_reference_twins(corpus, ref):
    ds = make(corpus, rir_noise_dataset=corpus["rir_noise"][0], reverb_proportion=1.0, reverb_noise_proportion=1.0, eq_prob=1.0, eq_filters=3,
              hp_prob=1.0, rir_len=1000, predelay=10)
    idx = torch.tensor([0, 4, 5])
    noisy, clean = ds.device_batch(idx, dev())
    torch.cuda.synchronize()
    c, n, snr = reference_batch(ds, ref, [0, 4, 5])
    banks = []
    for name, got in (("rir", ds._ensure_rirs(dev())), ("rir_noise", ds._ensure_noise_rirs(dev()))):
        h = np.zeros((len(ref[name]), 1000))
        for i, u in enumerate(ref[name]):                                   # 800 samples each: zero-padded to rir_len
            assert len(u) == 800
            h[i, :800] = u
        g = got[0].cpu().numpy()
        assert g.shape == h.shape and not g[:, 800:].any() and R.errors(g, h)[0] <= R.CAP
        assert np.array_equal(got[1].cpu().numpy(), h.argmax(axis=1) + 160) and got[2].NR == len(ref[name]) and got[2].early
        banks.append(h)
    ic, inz = ds.reverb_index
    assert ic.min() >= 0 and ic.max() < 2 and not inz.any()                # the noise bank has one response
    full = np.stack([F.truth(c[b], banks[0][ic[b]])[0] for b in range(3)])
    noise = np.stack([F.truth(n[b], banks[1][inz[b]])[0] for b in range(3)])
    cc, nc = ds.aug_coefs
    full, noise = BQ.cascade_ref(full, cc, False), BQ.cascade_ref(noise, nc, False)
    want_noisy, want_clean, _ = R.snr_mix64(full, noise, snr)
    e_n, e_c = rel_l2(noisy.cpu().double(), torch.from_numpy(want_noisy)), rel_l2(clean.cpu().double(), torch.from_numpy(want_clean))
    print(f"reverb + EQ batch vs the float64 chain: noisy rel-L2 {e_n:.2e}, clean rel-L2 {e_c:.2e}")
    assert e_n <= STAGE_BAR and e_c <= STAGE_BAR
    plain = make(corpus).device_batch(idx, dev())
    assert rel_l2(clean, plain[1]) > 1e-2


def test_valid_mode_repeats_and_training_moves_on(corpus):
    kw = dict(reverb_proportion=0.5, reverb_noise_proportion=0.5, rir_len=600, predelay=10)
    v = make(corpus, valid_mode=True, **kw)
    idx = torch.tensor([4, 1, 7])
    a = v.device_batch(idx, dev())
    rows = [r.copy() for r in v.reverb_index]
    b = v.device_batch(idx, dev())                                          # the next epoch
    one = make(corpus, valid_mode=True, **kw).device_batch(torch.tensor([7]), dev())
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(rows[0], v.reverb_index[0]) and np.array_equal(rows[1], v.reverb_index[1])
    assert torch.equal(one[0][0], a[0][2]) and torch.equal(one[1][0], a[1][2])          # item 7 alone: a function of (seed, item)
    t = make(corpus, **kw)
    e1, e2 = t.device_batch(idx, dev()), t.device_batch(idx, dev())
    t2 = make(corpus, **kw).device_batch(idx, dev())
    torch.cuda.synchronize()
    assert not torch.equal(e1[0], e2[0]) and not torch.equal(e1[1], e2[1])
    assert torch.equal(e1[0], t2[0]) and torch.equal(e1[1], t2[1])          # one seed, one stream
    for k in range(6):                                                      # more batches than pinned slots
        n, c = t.device_batch(idx, dev())
        assert bool(torch.isfinite(n).all()) and float(c.abs().amax()) > 0.5
    assert t._plan_k == 8


def test_the_parent_is_unchanged():
    from cruse_amd.data import DevicePairs, snr_mix
    ds = DevicePairs(num=8, length=3200, pool=4, seed=5)
    for idx in (torch.tensor([3, 0, 7, 5]), torch.arange(8)):
        noisy, clean = ds.device_batch(idx, dev())
        clean_p, noise_p, snr = ds._ensure(dev())
        i = idx.to(dev())
        want_noisy, want_clean, _ = snr_mix(clean_p.index_select(0, i % ds.pool), noise_p.index_select(0, (i * 7 + 3) % ds.pool),
                                            snr.index_select(0, i % ds.num), return_parts=True)
        torch.cuda.synchronize()
        assert torch.equal(noisy, want_noisy) and torch.equal(clean, want_clean)


def test_two_trainer_steps_from_the_file_config(corpus, tmp_path):
    from torch.utils.data import DataLoader, DistributedSampler
    import train_base.loss as L
    from cruse_amd.filepairs import DeviceFilePairs
    from cruse_amd.model.cruse_net import unet_2
    from cruse_amd.train.trainer_casual import Trainer, _Prefetcher
    from tools.train_stand import load_toml
    conf = load_toml(os.path.join(ROOT, "configs", "cruse_file_dataset.toml"))
    assert conf["train_dataset"]["path"] == conf["validation_dataset"]["path"] == "cruse_amd.filepairs.DeviceFilePairs"
    assert conf["validation_dataset"]["args"]["valid_mode"] is True and conf["trainer"]["validation"]["score_metric"] == "STOI"
    # silence_length: the config's 0.2 s gaps are 40 % of these 0.5 s clips, and where a gap of the speech meets a gap of the noise the mixture
    # has exactly silent frames, on which WO-MALE divides by zero and the guarded optimizer step skips the batch; gaps
    # shorter than a frame (5 ms) keep every step of this short run applied, so that the loss below is the loss of two real steps
    args = dict(conf["train_dataset"]["args"], clean_dataset=corpus["clean"][0], noise_dataset=corpus["noise"][0], rir_dataset=corpus["rir"][0],
                rir_noise_dataset=corpus["rir_noise"][0], sub_sample_length=0.5, dataset_length=4, rir_len=1000, silence_length=0.005)
    ds = DeviceFilePairs(**args)
    assert ds.length == 8000 and len(ds) == 4 and ds.augments and ds.reverberates
    torch.manual_seed(0)
    m = unet_2(**conf["model"]["args"])
    cfg = {"acoustics": conf["acoustics"], "trainer": {"train": dict(conf["trainer"]["train"], epochs=1)}, "meta": dict(conf["meta"], save_dir=str(tmp_path))}
    loader = DataLoader(ds, sampler=DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True), batch_size=2, drop_last=True, num_workers=0)
    tr = Trainer(dist=None, rank=0, config=cfg, resume=False, only_validation=False, model=m, loss_function=L.wo_male_loss(**conf["loss_function"]["args"]),
                 optimizer=torch.optim.Adam(m.parameters(), lr=conf["optimizer"]["lr"]), train_dataloader=loader, validation_dataloader=None)
    assert _Prefetcher(loader, tr.device).resident
    loss = tr._train_epoch(1)
    assert math.isfinite(loss) and loss > 0, loss
    assert tr.engine.skipped_steps() == 0 and ds._plan_k == 2 and ds._rev_k == 2 and ds._aug_k == 2
    vds = DeviceFilePairs(**dict(conf["validation_dataset"]["args"], clean_dataset=corpus["clean"][0], noise_dataset=corpus["noise"][0],
                                 sub_sample_length=0.5, dataset_length=2))
    a, b = vds[1], vds[1]                                                   # what the validation DataLoader asks for
    assert a[0].shape == (8000,) and not a[0].is_cuda and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
