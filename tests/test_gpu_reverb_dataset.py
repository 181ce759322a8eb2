"""GPU: DevicePairs with reverberation switched on (reverb_proportion / reverb_noise_proportion / reverb_target)
against a float64 oracle of the whole composition -- convolve, [EQ], peak-normalise, SNR-scale, mix -- and the unchanged default path."""
import numpy as np
import pytest
import torch

import biquad_ref as R
import fftconv_ref as F
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

STAGE_BAR = 1e-5                                                         # DESIGN 14e's bar for this composition (rel-L2)
SMALL = dict(num=8, length=4099, pool=4, seed=5)
# predelay 10 ms: with the default 50 ms, et = delay + 800 lies beyond a response of 600 taps and the early target would be the full one
REV = dict(reverb_proportion=1.0, reverb_noise_proportion=1.0, rir_pool=4, rir_len=600, predelay=10)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def gathered(ds, idx):
    clean_p, noise_p, snr = ds._ensure(dev())
    idx = idx.to(dev())
    return [t.cpu().numpy() for t in (clean_p.index_select(0, idx % ds.pool), noise_p.index_select(0, (idx * 7 + 3) % ds.pool), snr.index_select(0, idx % ds.num))]


def oracle(ds, idx, eps=1e-7):
    """float64: -> noisy, full clean, early clean (both at the full speech's scale), scaled noise"""
    c, n, snr = gathered(ds, idx)
    rirs, early_len, _ = ds._ensure_rirs(dev())
    rirs, early_len = rirs.cpu().numpy(), early_len.cpu().numpy()
    ic, inz = ds.reverb_index
    et = np.minimum(early_len, rirs.shape[1])
    cut = np.where(np.arange(rirs.shape[1])[None, :] < et[:, None], rirs, 0)
    pick = lambda x, h, i: np.stack([F.truth(x[b], h[i[b]])[0] if i[b] >= 0 else x[b].astype(np.float64) for b in range(len(i))])
    full, early, noise = pick(c, rirs, ic), pick(c, cut, ic), pick(n, rirs, inz)
    if ds.augments:
        cc, nc = ds.aug_coefs
        full, early, noise = R.cascade_ref(full, cc, False), R.cascade_ref(early, cc, False), R.cascade_ref(noise, nc, False)
    s = 1.0 / (np.abs(full).max(axis=1, keepdims=True) + eps)
    full, early = full * s, early * s
    noise = noise / (np.abs(noise).max(axis=1, keepdims=True) + eps)
    scalar = np.sqrt((full ** 2).mean(axis=1)) / 10 ** (snr.astype(np.float64) / 20) / (np.sqrt((noise ** 2).mean(axis=1)) + eps)
    noise = noise * scalar[:, None]
    return full + noise, full, early, noise


@pytest.mark.parametrize("eq", [False, True])
def test_defaults_are_bit_identical_to_a_dataset_built_without_the_arguments(eq):
    from cruse_amd.data import DevicePairs
    kw = dict(SMALL, **(dict(eq_prob=0.5, eq_filters=3, hp_prob=0.5) if eq else {}))
    a = DevicePairs(**kw)
    b = DevicePairs(reverb_proportion=0.0, reverb_noise_proportion=0.0, reverb_target="full", rir_pool=32, rir_len=8000, rt60_low=0.2, rt60_high=0.8,
                    predelay=50, **kw)
    for idx in (torch.arange(8), torch.tensor([3, 0, 7, 5])):
        na, ca = a.device_batch(idx, dev())
        nb, cb = b.device_batch(idx, dev())
        torch.cuda.synchronize()
        assert torch.equal(na, nb) and torch.equal(ca, cb)
    assert b.reverb_index is None and not b._rpin and not b._rirs and b._rev_k == 0      # no draw, no pool, no staging, no launch


@pytest.mark.parametrize("eq", [False, True])
@pytest.mark.parametrize("target", ["full", "early"])
def test_every_clip_reverberated_equals_the_float64_oracle(target, eq):
    from cruse_amd.data import DevicePairs
    ds = DevicePairs(reverb_target=target, **REV, **SMALL, **(dict(eq_prob=1.0, eq_filters=3, hp_prob=1.0) if eq else {}))
    idx = torch.tensor([3, 0, 7, 5, 1, 6])
    noisy, clean = ds.device_batch(idx, dev())
    torch.cuda.synchronize()
    ic, inz = ds.reverb_index
    assert ic.dtype == np.int32 and ic.shape == inz.shape == (6,) and ic.min() >= 0 and inz.min() >= 0 and max(ic.max(), inz.max()) < 4
    want_noisy, full, early, noise = oracle(ds, idx)
    assert rel_l2(torch.from_numpy(early), torch.from_numpy(full)) > 1e-2              # the early target is another signal
    e_noisy = rel_l2(noisy.cpu().double(), torch.from_numpy(want_noisy))
    e_clean = rel_l2(clean.cpu().double(), torch.from_numpy(early if target == "early" else full))
    print(f"target {target}, eq {eq}: noisy rel-L2 {e_noisy:.2e}, clean rel-L2 {e_clean:.2e}")
    assert e_noisy <= STAGE_BAR and e_clean <= STAGE_BAR
    if target == "early":                                                              # inside `noisy` sits the FULL reverberant speech
        e = rel_l2(noisy.cpu().double() - torch.from_numpy(noise), torch.from_numpy(full))
        print(f"noisy - scaled noise vs the full speech: rel-L2 {e:.2e}")
        assert e <= STAGE_BAR
    plain = DevicePairs(**SMALL).device_batch(idx, dev())
    assert rel_l2(clean, plain[1]) > 1e-2


def test_half_the_clips_reverberated():
    from cruse_amd.data import DevicePairs
    kw = dict(num=64, length=4099, pool=4, seed=5)
    ds = DevicePairs(reverb_proportion=0.5, reverb_noise_proportion=0.5, rir_pool=4, rir_len=600, **kw)
    other = DevicePairs(reverb_proportion=0.5, reverb_noise_proportion=0.5, rir_pool=4, rir_len=600, **kw)
    idx = torch.arange(64)
    noisy, clean = ds.device_batch(idx, dev())
    on, oc = other.device_batch(idx, dev())
    plain_noisy, plain_clean = DevicePairs(**kw).device_batch(idx, dev())
    torch.cuda.synchronize()
    assert torch.equal(noisy, on) and torch.equal(clean, oc)                           # one seed: the same bits
    ic, inz = ds.reverb_index
    first = (ic.copy(), inz.copy())
    for sel in (ic >= 0, inz >= 0):
        assert abs(int(sel.sum()) - 32) <= 4 * 4.0                                     # sigma = sqrt(64 / 4) = 4
    for b in range(64):
        if ic[b] < 0:
            assert torch.equal(clean[b], plain_clean[b]), b                            # pass-through, then the same snr_mix: the same bits
            if inz[b] < 0:
                assert torch.equal(noisy[b], plain_noisy[b]), b
        else:
            assert rel_l2(clean[b], plain_clean[b]) > 1e-3, b
        if inz[b] >= 0:
            assert rel_l2(noisy[b], plain_noisy[b]) > 1e-3, b
    ds.device_batch(idx, dev())
    other.device_batch(idx, dev())
    assert not np.array_equal(ds.reverb_index[0], first[0]) and not np.array_equal(ds.reverb_index[1], first[1])
    assert np.array_equal(ds.reverb_index[0], other.reverb_index[0]) and np.array_equal(ds.reverb_index[1], other.reverb_index[1])


def test_same_seed_same_batches_across_the_staging_ring():
    from cruse_amd.data import DevicePairs
    kw = dict(reverb_proportion=0.5, reverb_noise_proportion=0.3, reverb_target="early", rir_pool=4, rir_len=600, predelay=10, eq_prob=0.5, eq_filters=2, hp_prob=0.5, **SMALL)
    a, b = DevicePairs(**kw), DevicePairs(**kw)
    for k in range(6):                                                                 # more batches than pinned slots: they are reused
        idx = (torch.arange(4) + k) % 8
        na, ca = a.device_batch(idx, dev())
        nb, cb = b.device_batch(idx, dev())
        torch.cuda.synchronize()
        assert torch.equal(na, nb) and torch.equal(ca, cb)
        want_noisy, full, early, _ = oracle(a, idx)                                    # the staged rows of THIS batch are the ones the kernel read
        assert rel_l2(na.cpu().double(), torch.from_numpy(want_noisy)) <= STAGE_BAR
        assert rel_l2(ca.cpu().double(), torch.from_numpy(early)) <= STAGE_BAR
    assert a._rev_k == 6 and a._aug_k == 6


def test_the_rir_pool_is_what_the_docstring_says():
    from cruse_amd.data import DevicePairs
    ds = DevicePairs(reverb_proportion=0.5, rir_pool=16, rir_len=8000, seed=3)
    rirs, early, bank = ds._ensure_rirs(dev())
    h = rirs.cpu().numpy()
    assert h.shape == (16, 8000) and h.dtype == np.float32 and bank.NR == 16 and bank.R == 8000 and bank.early
    delay = (h != 0).argmax(axis=1)
    assert delay.min() >= 0 and delay.max() <= 240 and len(set(delay.tolist())) > 4 and np.all(h[np.arange(16), delay] == 1.0)
    # the tail decays by 60 dB over rt60 in [0.2, 0.8] s: its level at 0.1 s against the level at the start lies between the two slopes
    lvl = lambda a, b: np.sqrt((h[:, a:b] ** 2).mean(axis=1))
    drop_db = 20 * np.log10(lvl(1600, 2400) / lvl(300, 1100))
    assert np.all(drop_db < -60 * 1300 / (0.8 * 16000) + 3) and np.all(drop_db > -60 * 1300 / (0.2 * 16000) - 3)
    assert np.array_equal(early.cpu().numpy(), h.argmax(axis=1) + 800)
    again = DevicePairs(reverb_proportion=0.5, rir_pool=16, rir_len=8000, seed=3)._ensure_rirs(dev())[0]
    assert torch.equal(again, rirs)
