"""GPU: DevicePairs with the EQ augmentation switched on (eq_prob / eq_filters / hp_prob) against the float64 oracle of
tests/biquad_ref.py, the unchanged default path, and one trainer epoch on configs/cruse_augment.toml."""
import math
import os

import numpy as np
import pytest
import torch

import biquad_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STAGE_BAR = 1e-5                                                         # the project's stage bar (rel-L2)
SMALL = dict(num=8, length=3200, pool=4, seed=5)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def gathered(ds, idx):
    """what device_batch gathers before any filtering: (clean clips, noise clips, snr) as the dataset's own pools give them"""
    clean_p, noise_p, snr = ds._ensure(dev())
    idx = idx.to(dev())
    return clean_p.index_select(0, idx % ds.pool), noise_p.index_select(0, (idx * 7 + 3) % ds.pool), snr.index_select(0, idx % ds.num)


def test_defaults_are_bit_identical_to_the_plain_mix():
    from cruse_amd.data import DevicePairs, snr_mix
    ds = DevicePairs(**SMALL)
    idx = torch.arange(8)
    noisy, clean = ds.device_batch(idx, dev())
    c, n, snr = gathered(ds, idx)
    want_noisy, want_clean, _ = snr_mix(c, n, snr, return_parts=True)
    torch.cuda.synchronize()
    assert torch.equal(noisy, want_noisy) and torch.equal(clean, want_clean)
    assert ds.aug_coefs is None and not ds._pin                          # no draw, no staging buffer, no filter launch
    off = DevicePairs(eq_prob=0.0, eq_filters=3, hp_prob=0.0, **SMALL).device_batch(idx, dev())
    assert torch.equal(off[0], noisy) and torch.equal(off[1], clean)


def test_all_clips_augmented_equal_the_float64_oracle():
    from cruse_amd.data import DevicePairs, snr_mix
    ds = DevicePairs(eq_prob=1.0, eq_filters=3, hp_prob=1.0, **SMALL)
    idx = torch.tensor([3, 0, 7, 5, 1, 6])
    noisy, clean = ds.device_batch(idx, dev())
    torch.cuda.synchronize()
    cc, nc = ds.aug_coefs
    assert cc.shape == nc.shape == (6, 4, 6) and cc.dtype == np.float64 and not np.array_equal(cc, nc)
    assert not np.any(np.all(cc == np.array(R.IDENTITY), axis=2)) and not np.any(np.all(nc == np.array(R.IDENTITY), axis=2))
    c, n, snr = gathered(ds, idx)
    fc = R.cascade_ref(c.cpu().numpy(), cc, clamp=False)                  # the pools are not normalised: no clipping
    fn = R.cascade_ref(n.cpu().numpy(), nc, clamp=False)
    assert np.abs(fn).max() > 1.0
    want_clean = fc / (np.abs(fc).max(axis=1, keepdims=True) + 1e-7)      # snr_mix: clean / (max |clean| + eps)
    e = rel_l2(clean.cpu().double(), torch.from_numpy(want_clean))
    print(f"clean vs peak-normalised float64 oracle: rel-L2 {e:.2e}")
    assert e <= STAGE_BAR
    want_noisy = snr_mix(torch.from_numpy(fc.astype(np.float32)).cuda(), torch.from_numpy(fn.astype(np.float32)).cuda(), snr)
    e = rel_l2(noisy, want_noisy)
    print(f"noisy vs snr_mix of the oracle-filtered pair: rel-L2 {e:.2e}")
    assert e <= STAGE_BAR
    plain = DevicePairs(**SMALL).device_batch(idx, dev())
    assert rel_l2(clean, plain[1]) > 1e-2                                 # the target follows the augmentation


def test_half_the_clips_augmented():
    from cruse_amd.data import DevicePairs
    kw = dict(num=64, length=3200, pool=4, seed=5)
    ds = DevicePairs(eq_prob=0.5, eq_filters=3, hp_prob=0.5, **kw)
    idx = torch.arange(64)
    noisy, clean = ds.device_batch(idx, dev())
    plain_noisy, plain_clean = DevicePairs(**kw).device_batch(idx, dev())
    torch.cuda.synchronize()
    cc, nc = ds.aug_coefs
    ident = np.array(R.IDENTITY)
    c_off = np.all(cc == ident, axis=(1, 2))
    n_off = np.all(nc == ident, axis=(1, 2))
    assert 4 <= c_off.sum() <= 40 and 4 <= n_off.sum() <= 40              # P(untouched) = 1 / 4 per clip
    differs = 0
    for b in range(64):
        ec, en = rel_l2(clean[b], plain_clean[b]), rel_l2(noisy[b], plain_noisy[b])
        if c_off[b]:
            assert ec <= 1e-6, (b, ec)
            if n_off[b]:
                assert en <= 1e-6, (b, en)
        else:
            differs += ec > 1e-3
    assert differs >= 1 and differs == int((~c_off).sum())


def test_same_seed_same_batches():
    from cruse_amd.data import DevicePairs
    kw = dict(eq_prob=0.5, eq_filters=2, hp_prob=0.5, **SMALL)
    a, b, other = DevicePairs(**kw), DevicePairs(**kw), DevicePairs(**dict(kw, seed=6))
    for k in range(6):                                                   # more batches than pinned staging slots: they are reused
        idx = (torch.arange(4) + k) % 8
        na, ca = a.device_batch(idx, dev())
        nb, cb = b.device_batch(idx, dev())
        no, _ = other.device_batch(idx, dev())
        assert np.array_equal(a.aug_coefs[0], b.aug_coefs[0]) and np.array_equal(a.aug_coefs[1], b.aug_coefs[1])
        assert a.aug_coefs[0].shape == (4, 3, 6)
        torch.cuda.synchronize()
        assert torch.equal(na, nb) and torch.equal(ca, cb) and not torch.equal(na, no)
        # the staged coefficients of THIS batch are the ones the kernel read, although slots rotate
        c, n, _ = gathered(a, idx)
        want = R.cascade_ref(c.cpu().numpy(), a.aug_coefs[0], clamp=False)
        want /= np.abs(want).max(axis=1, keepdims=True) + 1e-7
        assert rel_l2(ca.cpu().double(), torch.from_numpy(want)) <= STAGE_BAR


def test_one_trainer_epoch_on_the_augment_config(tmp_path):
    from torch.utils.data import DataLoader, DistributedSampler
    import train_base.loss as L
    from cruse_amd.data import DevicePairs
    from cruse_amd.model.cruse_net import unet_2
    from cruse_amd.train.trainer_casual import Trainer
    from tools.train_stand import load_toml
    conf = load_toml(os.path.join(ROOT, "configs", "cruse_augment.toml"))
    assert conf["train_dataset"]["path"] == "cruse_amd.data.DevicePairs"
    args = dict(conf["train_dataset"]["args"], num=12, length=3200, pool=4)          # 3 steps of 4 clips
    ds = DevicePairs(**args)
    assert ds.augments and (ds.eq_prob, ds.eq_filters, ds.hp_prob) == (0.5, 3, 0.5)
    torch.manual_seed(0)
    m = unet_2(**conf["model"]["args"])
    cfg = {"acoustics": conf["acoustics"], "trainer": {"train": dict(conf["trainer"]["train"], epochs=1)},
           "meta": dict(conf["meta"], save_dir=str(tmp_path))}
    loader = DataLoader(ds, sampler=DistributedSampler(ds, num_replicas=1, rank=0, shuffle=True), batch_size=4, drop_last=True, num_workers=0)
    tr = Trainer(dist=None, rank=0, config=cfg, resume=False, only_validation=False, model=m, loss_function=L.wo_male_loss(**conf["loss_function"]["args"]),
                 optimizer=torch.optim.Adam(m.parameters(), lr=conf["optimizer"]["lr"]), train_dataloader=loader, validation_dataloader=None)
    loss = tr._train_epoch(1)
    assert math.isfinite(loss) and loss > 0, loss
    assert tr.engine.skipped_steps() == 0 and ds.aug_coefs is not None and ds._aug_k == 3
