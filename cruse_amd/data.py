"""Synthetic 16 kHz noisy/clean pairs: the reference's SynDataset is unfinished
(dataset/dataset.py ends mid-function) and the metric is quoted on synthetic data."""
from __future__ import annotations

import torch
from torch.utils.data import Dataset


def synth_batch(batch: int, length: int, device, seed: int):
    """clean = 4 * one-pole low-pass (a = 0.95, 64-tap FIR) of 0.05*N(0,1) (speech-like tilt), noise = 0.1*N(0,1),
    noisy = clean + noise.  On a HIP device the filter and the mix are libcruse_hip kernels (cruse_onepole_fir,
    cruse_axpby); torch only draws the Gaussian samples.  On the CPU (DataLoader workers of SyntheticPairs) the same
    FIR runs through torch."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(seed)
    white = 0.05 * torch.randn(batch, length, device=dev, generator=g)
    noise = 0.1 * torch.randn(batch, length, device=dev, generator=g)
    a, taps = 0.95, 64
    if dev.type == "cuda":
        from . import ops
        from ._lib import check, lib
        clean = torch.empty_like(white)
        check(lib.cruse_onepole_fir(ops._p(white), batch, length, a, taps, 4.0, ops._p(clean), ops._stream()))
        noisy = ops.axpby(torch.empty_like(clean), clean, noise, 1.0, 1.0)
        return noisy, clean
    w = (1 - a) * a ** torch.arange(taps - 1, -1, -1, dtype=torch.float32)
    clean = torch.nn.functional.conv1d(white.unsqueeze(1), w.view(1, 1, -1), padding=taps - 1)[..., :length].squeeze(1) * 4.0
    return (clean + noise).contiguous(), clean.contiguous()


def fir_causal(x: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """scipy.signal.fftconvolve(x, h)[:len(x)] per clip on the GPU (cruse_fir_causal).  x [B,L]; h [R] (shared) or [B,R]."""
    from . import ops
    from ._lib import check, lib
    x = x.contiguous().float()
    h = h.to(x.device).contiguous().float()
    B, L = x.shape
    if h.dim() == 1:
        R, hs = h.shape[0], 0
    elif h.dim() == 2 and h.shape[0] == B:
        R, hs = h.shape[1], h.shape[1]
    else:
        raise RuntimeError(f"fir_causal: taps {tuple(h.shape)} must be [R] or [{B}, R]")
    y = torch.empty_like(x)
    check(lib.cruse_fir_causal(ops._p(x), ops._p(h), hs, B, L, R, ops._p(y), ops._stream()))
    return y


def snr_mix(clean_y: torch.Tensor, noise_y: torch.Tensor, snr, target_dB_FS=None, target_dB_FS_floating_val=None, rir=None,
            rir_noise=None, eps: float = 1e-7, return_parts: bool = False):
    """SynDataset.snr_mix (dataset/dataset.py:235-264) with the reference's argument order, for a whole batch ON THE GPU:
    optional room impulse responses `rir` / `rir_noise` ([R] shared or [B,R]: fftconvolve(.)[:L], :245-248, as a direct FIR
    kernel), peak-normalise clean and noise, scale the noise by clean_rms / 10^(snr/20) / (noise_rms + eps), mix.
    clean_y, noise_y [B,L] (or [L]); snr: dB, scalar or [B].  Returns noisy (and the normalised clean / scaled noise with
    return_parts).  The reference's function ENDS after drawing `noisy_target_dB_FS` from
    np.random.randint(target_dB_FS - floating, target_dB_FS + floating) (the file is truncated there, :261-264): when both
    are given the draw is made -- once per clip of the batch -- to consume numpy's RNG exactly as B calls of the reference's
    per-clip function do, and nothing else is done with it."""
    from . import ops
    from ._lib import check, lib
    one = clean_y.dim() == 1
    c = clean_y.reshape(1, -1) if one else clean_y
    n = noise_y.reshape(1, -1) if one else noise_y
    if c.shape != n.shape or c.dim() != 2:
        raise RuntimeError(f"snr_mix: clean {tuple(clean_y.shape)} and noise {tuple(noise_y.shape)} must match ([B,L] or [L])")
    c = c.contiguous().float(); n = n.contiguous().float()
    if rir is not None:
        c = fir_causal(c, torch.as_tensor(rir))
    if rir_noise is not None:
        n = fir_causal(n, torch.as_tensor(rir_noise))
    B, L = c.shape
    snr_t = torch.as_tensor(snr, dtype=torch.float32, device=c.device).reshape(-1)
    if snr_t.numel() == 1:
        snr_t = snr_t.expand(B)
    snr_t = snr_t.contiguous()
    scratch = torch.empty(3 * B, device=c.device, dtype=torch.float64)
    noisy = torch.empty_like(c)
    co = torch.empty_like(c) if return_parts else None
    no = torch.empty_like(c) if return_parts else None
    check(lib.cruse_snr_mix(ops._p(c), ops._p(n), ops._p(snr_t), B, L, eps, ops._p(scratch), ops._p(co), ops._p(no), ops._p(noisy),
                            ops._stream()))
    if target_dB_FS is not None and target_dB_FS_floating_val is not None:
        import numpy as np
        # one draw PER CLIP: the reference's snr_mix is a per-clip function, so a batch of B clips consumes B draws there
        # (a single draw per batched call let identically seeded host RNG streams diverge for B > 1)
        np.random.randint(target_dB_FS - target_dB_FS_floating_val, target_dB_FS + target_dB_FS_floating_val,
                          size=None if one else B)                                                               # :261-264
    if one:
        noisy = noisy[0]; co = None if co is None else co[0]; no = None if no is None else no[0]
    return (noisy, co, no) if return_parts else noisy


def synth_rirs(n: int, rir_len: int, rt60_low: float, rt60_high: float, sr: int, device, generator):
    """[n, rir_len] f32 synthetic room impulse responses in the manner of fixture G20's: a unit direct path after a delay of 0-15 ms,
    zeros before it, and after it 0.3 N(0,1) 10^(-3 k / (rt60 sr)) at tap k (-60 dB at k = rt60 sr), one rt60 per response drawn
    uniformly from [rt60_low, rt60_high] seconds.  Drawn on `device` from `generator` (delay, rt60, tail, in this order)."""
    delay = torch.randint(0, 15 * sr // 1000 + 1, (n,), device=device, generator=generator).clamp_(max=rir_len - 1)
    rt60 = rt60_low + (rt60_high - rt60_low) * torch.rand(n, device=device, generator=generator)
    k = torch.arange(rir_len, device=device, dtype=torch.float32)
    h = 0.3 * torch.randn(n, rir_len, device=device, generator=generator) * torch.pow(10.0, -3.0 * k[None, :] / (rt60[:, None] * sr))
    h = torch.where(k[None, :] < delay[:, None], torch.zeros_like(h), h)
    h.scatter_(1, delay[:, None], 1.0)
    return h.contiguous()


def rir_early_len(rir: torch.Tensor, predelay: int = 50, sr: int = 16000) -> torch.Tensor:
    """int32 [NR]: add_reverb's `et` of every row of rir [NR, R] -- the index of the largest VALUE (not magnitude, dataset.py:219)
    plus predelay ms.  Not clamped to R: cruse_fftconv_prepare clamps, as the reference's slice rir[:et] saturates."""
    return (torch.argmax(rir, dim=1) + (predelay * sr) // 1000).to(torch.int32)


def add_reverb(cln_wav: torch.Tensor, rir_wav: torch.Tensor, channels: int = 1, predelay: int = 50, sr: int = 16000):
    """SynDataset.add_reverb (dataset/dataset.py:215-233) for one clip or a batch ON THE GPU: the reverberant speech
    fftconvolve(cln, rir)[:L] and the early-reflection target fftconvolve(cln, rir[:et])[:L], et = argmax(rir) + predelay ms, both from
    one cruse_fftconv_apply on the same input spectra.  cln_wav [L] or [B, L]; rir_wav [R] (one response for all clips) or [B, R].
    Returns (wav_tgt, wav_early_tgt) in the shape of cln_wav, f32.
    Repairs, stated: (1) the reference returns [L, channels] float64 arrays; here the mono pair comes back in the shape of cln_wav in
    f32 (dataset.SynDataset.add_reverb keeps the reference's [L, 1]).  (2) channels > 1 is refused: the reference's multi-microphone
    branch also picks a random row of a 2-D cln_wav (:224) -- multi-channel paths are out of scope.  (3) rir[:et]
    with et > R is the whole response there (a slice saturates) and is here by the kernel's clamp; et is never read by the host.
    (4) argmax is taken over the values, as :219 does: a negative tap of larger magnitude than the direct path does not move et."""
    from . import ops
    if channels != 1:
        raise NotImplementedError("add_reverb: channels > 1 (multi-microphone responses) is not built (SURVEY section 2)")
    one = cln_wav.dim() == 1
    x = (cln_wav.reshape(1, -1) if one else cln_wav).contiguous().float()
    if x.dim() != 2:
        raise RuntimeError(f"add_reverb: cln_wav {tuple(cln_wav.shape)} must be [L] or [B, L]")
    h = torch.as_tensor(rir_wav).to(x.device).float()
    h = (h.reshape(1, -1) if h.dim() == 1 else h).contiguous()
    if h.dim() != 2 or h.shape[0] not in (1, x.shape[0]):
        raise RuntimeError(f"add_reverb: rir_wav {tuple(rir_wav.shape)} must be [R] or [{x.shape[0]}, R]")
    bank = ops.fft_conv_prepare(h, rir_early_len(h, predelay, sr))
    full, early = ops.fft_conv_apply(x, bank, want_early=True)
    return (full[0], early[0]) if one else (full, early)


class SyntheticPairs(Dataset):
    """[train_dataset] plug-in: path = "cruse_amd.data.SyntheticPairs", args = {num, length, seed}."""

    def __init__(self, num: int = 64, length: int = 64000, seed: int = 0):
        self.num, self.length, self.seed = num, length, seed

    def __len__(self):
        return self.num

    def __getitem__(self, i):
        noisy, clean = synth_batch(1, self.length, "cpu", self.seed * 100003 + i)
        return noisy[0], clean[0]


class HostPoolPairs(Dataset):
    """[train_dataset] plug-in for a HOST dataset that costs the workers nothing per item: `pool` clips are synthesised once (per
    process) and item i is a view of clip i % pool -- the DataLoader's workers only collate.  With the trainer's pinned, double-buffered
    prefetcher (trainer_casual._Prefetcher) this measures what the reference's DataLoader path (tools/train_stand.py:46-57) can feed.
    path = "cruse_amd.data.HostPoolPairs", args = {num, length, seed, pool, dtype}."""

    def __init__(self, num: int = 2048, length: int = 64000, seed: int = 0, pool: int = 128, dtype: str = "float32"):
        self.num, self.length, self.seed, self.pool = num, length, seed, max(1, min(pool, num))
        # "float16": the samples are STORED as 16-bit values (as PCM audio is) -- half the bytes through the DataLoader's queue, the
        # staging copy and PCIe; the trainer widens them on the device (exactly)
        self.dtype = {"float32": torch.float32, "float16": torch.float16}[dtype]
        self._data = None

    def __len__(self):
        return self.num

    def _ensure(self):
        if self._data is None:
            noisy, clean = synth_batch(self.pool, self.length, "cpu", self.seed * 100003 + 17)
            self._data = (noisy.to(self.dtype).share_memory_(), clean.to(self.dtype).share_memory_())      # (forked workers read the parent's pages)
        return self._data

    def __getitem__(self, i):
        noisy, clean = self._ensure()
        return noisy[i % self.pool], clean[i % self.pool]


class DevicePairs(Dataset):
    """[train_dataset] plug-in for a DEVICE-RESIDENT dataset ("so real-data training is not host-bound"): clean and noise
    pools live in HBM and a batch is an index gather + the on-GPU SynDataset.snr_mix (dataset/dataset.py:235-264, cruse_snr_mix: peak
    normalisation, RMS-based SNR scaling, mix) at a per-clip SNR drawn from [snr_low, snr_high] dB -- no host tensor, no PCIe copy.
    The trainer recognises `device_resident` and asks for whole batches (device_batch) with the indices of the DataLoader's own
    sampler; the DataLoader object the reference flow builds around the dataset is never iterated.  __getitem__ still works (host
    copies of one pair) for anything that wants to look at an item.
    path = "cruse_amd.data.DevicePairs", args = {num, length, seed, pool, snr_low, snr_high, eq_prob, eq_filters, hp_prob,
    reverb_proportion, reverb_noise_proportion, reverb_target, rir_pool, rir_len, rt60_low, rt60_high, predelay}.

    EQ augmentation (train_base/acoustics/audioAug.py: compositeSecFilt, hp_filter), off by default: with
    eq_prob / hp_prob > 0 every clean clip and every noise clip of a batch independently gets a cascade of `eq_filters` random
    sections with probability eq_prob and the 150 Hz high-pass with probability hp_prob, BEFORE snr_mix and without clipping (the
    pools are not normalised to +-1; snr_mix peak-normalises afterwards).  The returned clean is the filtered, normalised speech: the
    target follows the augmentation.  A clip that is not selected gets identity sections, so one cruse_biquad_cascade launch of
    S = eq_filters + 1 sections per tensor covers the batch.  The draws come from a numpy Generator the dataset owns (seeded from
    `seed`), the sections are designed on the host in float64 and reach the device by one non-blocking copy per tensor from a ring
    of pinned buffers; a buffer is rewritten only after the event behind its last copy has completed, and the stream is never
    synchronised with the host.  `aug_coefs` holds the last batch's (clean, noise) coefficient arrays [B, S, 6].

    Reverberation (SynDataset._select_rir / snr_mix(rir=, rir_noise=) / add_reverb, dataset/dataset.py:205-247), off
    by default: every clean clip is convolved with a room impulse response with probability reverb_proportion and every noise clip
    with probability reverb_noise_proportion, each with an independently drawn row of a pool of `rir_pool` synthetic responses of
    `rir_len` taps (synth_rirs; filepairs.DeviceFilePairs is the subclass that fills all the pools from WAV files), FIRST -- then the EQ, then snr_mix, the order
    the reference marks (:249).  One cruse_fftconv_apply per tensor covers the batch: a clip that is not selected carries index -1 and
    passes through bit for bit.  The rows come from a numpy Generator of their own (seed * 100003 + 43: the EQ draws are the same
    with reverb on or off) and reach the device as int32 [B] through a pinned ring under the same event discipline as the
    coefficients.  `reverb_index` holds the last batch's (clean, noise) index arrays.  reverb_target "full": the returned clean is
    the reverberant, normalised speech (what the reference's snr_mix returns); "early": the speech through the first
    argmax(rir) + predelay ms of its response (add_reverb's wav_early_tgt), through the same EQ coefficients, at the scale
    1 / (max |full| + eps) snr_mix gave the speech inside `noisy` -- the target of a dereverberating enhancer."""

    device_resident = True
    NPIN = 4                   # pinned coefficient buffers per tensor: a slot is reused four batches later
    AUG_SR = 16000             # the filters are designed for the rate of the pools (synth_batch: 16 kHz), whatever [acoustics] sr says

    def __init__(self, num: int = 2048, length: int = 64000, seed: int = 0, pool: int = 128, snr_low: float = 0.0, snr_high: float = 20.0,
                 eq_prob: float = 0.0, eq_filters: int = 3, hp_prob: float = 0.0, reverb_proportion: float = 0.0,
                 reverb_noise_proportion: float = 0.0, reverb_target: str = "full", rir_pool: int = 32, rir_len: int = 8000,
                 rt60_low: float = 0.2, rt60_high: float = 0.8, predelay: int = 50):
        self.num, self.length, self.seed, self.pool = num, length, seed, max(1, min(pool, num))
        self.snr_low, self.snr_high = float(snr_low), float(snr_high)
        self.eq_prob, self.eq_filters, self.hp_prob = float(eq_prob), int(eq_filters), float(hp_prob)
        if not (0.0 <= self.eq_prob <= 1.0 and 0.0 <= self.hp_prob <= 1.0):
            raise ValueError(f"DevicePairs: eq_prob = {eq_prob} and hp_prob = {hp_prob} are probabilities")
        if self.augments and not 0 < self.eq_filters < 6:
            raise ValueError(f"DevicePairs: eq_filters = {eq_filters} must lie in 1..5 (six filter types, distinct per clip)")
        self.aug_coefs = None
        self._aug_rng = None
        self._pin = {}             # (device, B) -> [NPIN][2] pinned [B, S, 6] f64
        self._pin_ev = {}          # (device, B) -> [NPIN] event behind the slot's last copies
        self._aug_k = 0
        self._pools = {}
        self.reverb_proportion, self.reverb_noise_proportion = float(reverb_proportion), float(reverb_noise_proportion)
        self.reverb_target, self.rir_pool, self.rir_len = reverb_target, int(rir_pool), int(rir_len)
        self.rt60_low, self.rt60_high, self.predelay = float(rt60_low), float(rt60_high), int(predelay)
        if not (0.0 <= self.reverb_proportion <= 1.0 and 0.0 <= self.reverb_noise_proportion <= 1.0):
            raise ValueError(f"DevicePairs: reverb_proportion = {reverb_proportion} and reverb_noise_proportion = {reverb_noise_proportion} "
                             "are probabilities")
        if reverb_target not in ("full", "early"):
            raise ValueError(f"DevicePairs: reverb_target = {reverb_target!r} must be 'full' or 'early'")
        if self.rir_len < 1 or self.rir_pool < 1 or self.rt60_low > self.rt60_high or self.rt60_low <= 0.0:
            raise ValueError(f"DevicePairs: rir_len = {rir_len}, rir_pool = {rir_pool} must be >= 1 and 0 < rt60_low = {rt60_low} <= rt60_high = {rt60_high}")
        self.reverb_index = None
        self._rev_rng = None
        self._rpin = {}            # (device, B) -> [NPIN] pinned [2, B] int32
        self._rpin_ev = {}
        self._rev_k = 0
        self._rirs = {}            # device -> (rir pool [rir_pool, rir_len], early_len int32 [rir_pool], prepared bank)

    @property
    def augments(self) -> bool:
        return self.eq_prob > 0.0 or self.hp_prob > 0.0

    @property
    def reverberates(self) -> bool:
        return self.reverb_proportion > 0.0 or self.reverb_noise_proportion > 0.0

    def draw_reverb_index(self, n: int, proportion: float, rows=None):
        """int32 [n]: per clip a row of the RIR pool (of `rows` responses, rir_pool by default) with probability `proportion`, -1
        otherwise.  Consumes the dataset's reverb generator."""
        import numpy as np
        if self._rev_rng is None:
            self._rev_rng = np.random.default_rng(self.seed * 100003 + 43)
        sel = self._rev_rng.random(n) < proportion
        rows = self._rev_rng.integers(0, self.rir_pool if rows is None else rows, size=n)
        return np.where(sel, rows, -1).astype(np.int32)

    def _draw_reverb_rows(self, B: int):
        """(clean, noise) int32 [B] rows of this batch; a subclass with other pools or other draws overrides it"""
        return self.draw_reverb_index(B, self.reverb_proportion), self.draw_reverb_index(B, self.reverb_noise_proportion)

    def _noise_rir_bank(self, device):
        """the prepared bank the NOISE clips are convolved with: the speech's own here"""
        return self._ensure_rirs(device)[2]

    def _ensure_rirs(self, device):
        from . import ops
        device = torch.device(device)
        if device not in self._rirs:
            g = torch.Generator(device=device).manual_seed(self.seed * 100003 + 31)
            rirs = synth_rirs(self.rir_pool, self.rir_len, self.rt60_low, self.rt60_high, self.AUG_SR, device, g)
            early = rir_early_len(rirs, self.predelay, self.AUG_SR)
            self._rirs[device] = (rirs, early, ops.fft_conv_prepare(rirs, early))
        return self._rirs[device]

    def _reverb(self, c, n, device):
        """-> (clean, noise, early clean or None): the two tensors through their drawn responses"""
        from . import ops
        B = c.shape[0]
        key = (device, B)
        if key not in self._rpin:
            self._rpin[key] = [torch.empty(2, B, dtype=torch.int32).pin_memory() for _ in range(self.NPIN)]
            self._rpin_ev[key] = [None] * self.NPIN
        slot = self._rev_k % self.NPIN
        self._rev_k += 1
        ev = self._rpin_ev[key][slot]
        if ev is not None:
            ev.synchronize()                       # the copy issued NPIN batches ago: a wait on that event, not on the stream
        host = self._draw_reverb_rows(B)
        buf = self._rpin[key][slot]
        buf.numpy()[0], buf.numpy()[1] = host
        idx = buf.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._rpin_ev[key][slot] = ev
        self.reverb_index = host
        bank = self._ensure_rirs(device)[2]
        early = None
        if self.reverb_proportion > 0.0 and self.reverb_target == "early":
            c, early = ops.fft_conv_apply(c, bank, h_index=idx[0], want_early=True)
        elif self.reverb_proportion > 0.0:
            c = ops.fft_conv_apply(c, bank, h_index=idx[0])
        if self.reverb_noise_proportion > 0.0:
            n = ops.fft_conv_apply(n, self._noise_rir_bank(device), h_index=idx[1])
        return c, n, early

    def draw_aug_coefs(self, n: int):
        """[n, eq_filters + 1, 6] float64: per clip the EQ cascade with probability eq_prob, then the high-pass with probability hp_prob;
        identity sections where not selected.  Consumes the dataset's own generator."""
        import numpy as np
        from .acoustics import audio_aug as A
        if self._aug_rng is None:
            self._aug_rng = np.random.default_rng(self.seed * 100003 + 41)
        rng = self._aug_rng
        coef = np.empty((n, self.eq_filters + 1, 6), dtype=np.float64)
        coef[:] = A.IDENTITY_SECTION
        eq = rng.random(n) < self.eq_prob
        hp = rng.random(n) < self.hp_prob
        if eq.any():
            coef[eq, :self.eq_filters] = A.draw_sec_filters(int(eq.sum()), self.eq_filters, self.AUG_SR, rng)
        if hp.any():
            coef[hp, self.eq_filters] = A.draw_hp_filters(int(hp.sum()), 1, self.AUG_SR, rng)[:, 0]
        return coef

    def _augment(self, c, n, device, early=None):
        from . import ops
        B = c.shape[0]
        key = (device, B)
        if key not in self._pin:
            S = self.eq_filters + 1
            self._pin[key] = [[torch.empty(B, S, 6, dtype=torch.float64).pin_memory() for _ in range(2)] for _ in range(self.NPIN)]
            self._pin_ev[key] = [None] * self.NPIN
        slot = self._aug_k % self.NPIN
        self._aug_k += 1
        ev = self._pin_ev[key][slot]
        if ev is not None:
            ev.synchronize()                       # the copies issued NPIN batches ago: a wait on that event, not on the stream
        host = (self.draw_aug_coefs(B), self.draw_aug_coefs(B))
        dev = []
        for buf, h in zip(self._pin[key][slot], host):
            buf.numpy()[...] = h
            dev.append(buf.to(device, non_blocking=True))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._pin_ev[key][slot] = ev
        self.aug_coefs = host
        if early is not None:                      # the early target follows the speech: the same sections
            early = ops.biquad_cascade(early, dev[0], clamp=False)
        return ops.biquad_cascade(c, dev[0], clamp=False), ops.biquad_cascade(n, dev[1], clamp=False), early

    def __len__(self):
        return self.num

    def _ensure(self, device):
        device = torch.device(device)
        if device not in self._pools:
            g = torch.Generator(device=device).manual_seed(self.seed * 100003 + 29)
            _, clean = synth_batch(self.pool, self.length, device, self.seed * 100003 + 17)
            noise = torch.randn(self.pool, self.length, device=device, generator=g)
            snr = self.snr_low + (self.snr_high - self.snr_low) * torch.rand(self.num, device=device, generator=g)
            self._pools[device] = (clean, noise, snr)
        return self._pools[device]

    def _gather(self, idx: torch.Tensor, device):
        """-> (clean clips [B, length], noise clips [B, length], snr [B] in dB) of a batch before any filtering; a subclass that fills
        its batches from other pools (filepairs.DeviceFilePairs) overrides this and inherits the rest of device_batch"""
        clean_p, noise_p, snr = self._ensure(device)
        idx = idx.to(device, non_blocking=True)
        return clean_p.index_select(0, idx % self.pool), noise_p.index_select(0, (idx * 7 + 3) % self.pool), snr.index_select(0, idx % self.num)

    def device_batch(self, idx: torch.Tensor, device):
        """idx [B] int64 (host or device): -> (noisy, clean) [B, length] f32 on `device`, issued on the current stream"""
        c, n, snr = self._gather(idx, device)
        early = None
        if self.reverberates:
            c, n, early = self._reverb(c, n, torch.device(device))
        if self.augments:
            c, n, early = self._augment(c, n, torch.device(device), early)
        noisy, clean, _ = snr_mix(c, n, snr, return_parts=True)
        if early is not None:
            from . import ops
            clean = ops.peak_scale(early, c)        # 1 / (max |full| + eps): the scale of the speech inside `noisy`
        return noisy, clean

    def __getitem__(self, i):
        dev = torch.device("cuda", torch.cuda.current_device())
        noisy, clean = self.device_batch(torch.tensor([int(i)]), dev)
        return noisy[0].cpu(), clean[0].cpu()
