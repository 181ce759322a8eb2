"""Training pairs from WAV file lists, device-resident: the reference's SynDataset (dataset/dataset.py:49-213) on the
kernels cruse_resample_poly and cruse_assemble_clips, in front of the chain DevicePairs already runs (reverberation, EQ, snr_mix)."""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import resample_design as D
from . import wavio
from .data import DevicePairs, rir_early_len


def plan_clip(first: Optional[int], lengths: Sequence[int], target: int, silence: int, rng: np.random.Generator) -> np.ndarray:
    """SynDataset._select_clean_y (dataset/dataset.py:147-182; `first` = the item's own utterance) and _select_noise_y (:184-203;
    first = None: from empty) as a PLAN over the table of utterance lengths, no sample touched: start with `first`, remain = target -
    len; while remain > 0 append a uniformly drawn utterance (rng.integers(len(lengths))), remain -= its length, and if remain is still
    > 0 append min(remain, silence) zeros, remain -= that; a total beyond target is cropped at start = rng.integers(total - target)
    (a total equal to target draws nothing).  -> int64 [nseg, 4] rows (utterance, offset inside it, dst, len) of the pieces that
    survive the crop, ascending in dst; everything between them is silence."""
    lengths = np.asarray(lengths)
    target, silence = int(target), int(silence)
    parts = []                                                 # (utterance or -1 for silence, samples)
    remain = target
    if first is not None:
        parts.append((int(first), int(lengths[first])))
        remain -= parts[0][1]
    while remain > 0:
        u = int(rng.integers(len(lengths)))
        parts.append((u, int(lengths[u])))
        remain -= parts[-1][1]
        if remain > 0:
            gap = min(remain, silence)
            parts.append((-1, gap))
            remain -= gap
    total = sum(n for _, n in parts)
    start = int(rng.integers(total - target)) if total > target else 0
    rows, pos = [], 0
    for u, n in parts:
        a, b = max(pos, start), min(pos + n, start + target)
        if u >= 0 and b > a:
            rows.append((u, a - pos, a - start, b - a))
        pos += n
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


def parse_snr_range(snr_range) -> List[int]:
    """BaseDataset._parse_snr_range (dataset/dataset.py:34-46): the integers low .. high"""
    if len(snr_range) != 2:
        raise ValueError(f"The range of snr should be [low, high], not {snr_range}")
    low, high = int(snr_range[0]), int(snr_range[1])
    if low > high:
        raise ValueError("The low snr should not larger than high snr")
    return list(range(low, high + 1))


def load_pool(paths: Sequence[str], device, sr: int = 16000, chunk_values: int = 1 << 26, files=None):
    """Read the 16-bit PCM files `paths` (wavio.read_pcm16; `files`: what it returned for them, where the caller has read them already),
    group them by (rate, channels), upload each group as concatenated PCM in chunks of at most chunk_values samples and convert every
    chunk with one cruse_resample_poly launch (channel 0, x / 32768) into one flat f32 pool at `sr`, laid out group by group.
    -> (pool, start int64 [n], len int64 [n]: where file i lies in the pool, one stats row per group)"""
    from . import ops
    t_read = [0.0] * len(paths)
    if files is None:
        files = []
        for k, p in enumerate(paths):
            t0 = time.perf_counter()
            files.append(wavio.read_pcm16(p))
            t_read[k] = time.perf_counter() - t0
    groups = {}
    for i, (_, ch, rate) in enumerate(files):
        groups.setdefault((rate, ch), []).append(i)
    start, lens = np.zeros(len(files), dtype=np.int64), np.zeros(len(files), dtype=np.int64)
    pos = 0
    for (rate, ch), members in sorted(groups.items()):
        up, down = D.ratio(sr, rate)
        for i in members:
            start[i], lens[i] = pos, D.out_len(files[i][0].shape[0] // ch, up, down)
            pos += lens[i]
    pool = torch.empty(pos, device=device, dtype=torch.float32)
    stats = []
    for (rate, ch), members in sorted(groups.items()):
        up, down = D.ratio(sr, rate)
        t0 = time.perf_counter()
        k = 0
        while k < len(members):                                # chunks of bounded size; a file is never split
            e, values = k, 0
            while e < len(members) and (e == k or values + files[members[e]][0].shape[0] <= chunk_values):
                values += files[members[e]][0].shape[0]
                e += 1
            part = members[k:e]
            frames = np.array([files[i][0].shape[0] // ch for i in part], dtype=np.int64)
            off_in = np.concatenate([[0], np.cumsum(frames)])
            off_out = np.concatenate([[start[part[0]]], start[part[0]] + np.cumsum(lens[part])])
            src = torch.from_numpy(np.concatenate([files[i][0] for i in part])).to(device)
            ops.resample_poly(src, off_in, off_out, up, down, pool, channels=ch, channel=0)          # repair (2): channel 0
            k = e
        torch.cuda.synchronize(device)                         # once per group, at preload only: the time below is the device's
        stats.append(dict(rate=rate, channels=ch, files=len(members), frames=int(sum(files[i][0].shape[0] // ch for i in members)),
                          read_s=sum(t_read[i] for i in members), device_s=time.perf_counter() - t0))
    return pool, start, lens, stats


class DeviceFilePairs(DevicePairs):
    """[train_dataset] / [validation_dataset] plug-in: the reference's SynDataset on file lists, DEVICE-RESIDENT.
    path = "cruse_amd.filepairs.DeviceFilePairs" (also dataset.dataset.DeviceFilePairs), args = the reference constructor's names:
    clean_dataset / noise_dataset / rir_dataset / rir_noise_dataset (list files: one WAV path per line) each with _limit and _offset,
    snr_range = [low, high] (integers; the SNR of a clip is drawn from the integer list), reverb_proportion, reverb_noise_proportion,
    silence_length and sub_sample_length in seconds (length = int(sub_sample_length * sr) samples), sr (16000 only: anything else is
    refused), dataset_length (items; the number of clean files when 0 / None), valid_mode; plus DevicePairs' switches seed, eq_prob,
    eq_filters, hp_prob, reverb_target, rir_len, predelay.  target_dB_FS, target_dB_FS_floating_val, pre_load_clean_dataset,
    pre_load_noise, pre_load_rir and num_workers are accepted and have NO effect: the reference's file ends before it uses the first
    two (:262-264), and everything is preloaded here.

    Preload, once per device at the first batch: every file is read on the host (wavio.read_pcm16: 16-bit PCM only), the files are
    grouped by (rate, channels), each group is uploaded as concatenated PCM in chunks of at most CHUNK_VALUES samples and one
    cruse_resample_poly launch per chunk converts it (channel 0, x / 32768, Kaiser polyphase low-pass of resample_design) into one
    flat f32 pool at 16 kHz.  The pool is laid out group by group; `clean_utt_start` / `clean_utt_len` (and noise_, rir_, rir_noise_) are
    the HOST tables of where utterance i of the list lies.  RIR files take the same path, are cut or zero-padded to rir_len by one
    cruse_assemble_clips into [n, rir_len] and prepared with their early lengths exactly as the synthetic pool is; with
    rir_noise_dataset the noise clips use a second bank made from it, otherwise the first.

    A batch: for every item the host plans the clean clip (plan_clip from general_mix_dataset_list[i], the item's first utterance,
    drawn at construction as at :134) and the noise clip (from empty) and draws the SNR; the plans and SNRs reach the device by ONE
    non-blocking copy from a ring of pinned buffers (a slot is rewritten only after the event behind its last copy has completed;
    the stream is never synchronised), one cruse_assemble_clips launch per tensor stitches the clips, and DevicePairs' chain follows
    unchanged: _reverb -> _augment -> snr_mix, with the reverb_target = "early" handling.  `last_plan` holds the last batch's
    (clean seg, clean first, noise seg, noise first) host arrays and `last_snr` its SNRs.

    Determinism: the plans and SNRs come from a numpy Generator of the dataset's own (seed * 100003 + 47; the EQ and reverb streams
    are DevicePairs', so they are the same with or without files).  With valid_mode the plan, the SNR and the RIR rows of item i are
    a pure function of (seed, i) -- a generator seeded [seed * 100003 + 47, i] per item -- so every validation epoch scores the same
    mixtures; without it consecutive batches continue one stream and two epochs differ.

    Silent frames: where a gap of the speech meets a gap of the noise the mixture is exactly zero; a frame that is zero throughout makes
    the WO-MALE loss non-finite (it divides by the noisy magnitude, as the reference does) and the guarded optimizer step skips that batch
    (TrainEngine.skipped_steps).

    Repairs of the reference, stated: (1) the noise-RIR list is cut with (offset, limit), not the swapped (limit, offset) of
    :106-108.  (2) A multi-channel file contributes channel 0; the reference's random choice (:156-166) indexes the sample axis of
    librosa's [channels, samples] array.  (3) The reference class has no __getitem__ (its file is cut off inside snr_mix); the flow
    here is the one its methods imply: _select_clean_y, _select_noise_y, _select_rir for speech and noise, snr_mix.  (4) lib.load's
    resampler (soxr) is replaced by the Kaiser design above; agreement with librosa's samples is not claimed."""

    SR = 16000
    CHUNK_VALUES = 1 << 26     # int16 values per upload and resample launch (128 MiB)

    def __init__(self, clean_dataset, noise_dataset, clean_dataset_limit=None, clean_dataset_offset=0, noise_dataset_limit=None,
                 noise_dataset_offset=0, rir_dataset=None, rir_dataset_limit=None, rir_dataset_offset=0, rir_noise_dataset=None,
                 rir_noise_dataset_limit=None, rir_noise_dataset_offset=0, snr_range=(0, 20), reverb_proportion: float = 0.0,
                 reverb_noise_proportion: float = 0.0, silence_length: float = 0.2, target_dB_FS=None, target_dB_FS_floating_val=None,
                 sub_sample_length: float = 4.0, sr: int = 16000, dataset_length=None, pre_load_clean_dataset=None, pre_load_noise=None,
                 pre_load_rir=None, num_workers=None, valid_mode: bool = False, seed: int = 0, eq_prob: float = 0.0, eq_filters: int = 3,
                 hp_prob: float = 0.0, reverb_target: str = "full", rir_len: int = 8000, predelay: int = 50):
        if int(sr) != self.SR:
            raise ValueError(f"DeviceFilePairs: sr = {sr}: the pools, the filters and the model are at {self.SR} Hz only for now")
        self.clean_dataset_list = wavio.read_list(clean_dataset, clean_dataset_offset, clean_dataset_limit)
        self.noise_dataset_list = wavio.read_list(noise_dataset, noise_dataset_offset, noise_dataset_limit)
        self.rir_dataset_list = wavio.read_list(rir_dataset, rir_dataset_offset, rir_dataset_limit) if rir_dataset else []
        self.rir_noise_dataset_list = (wavio.read_list(rir_noise_dataset, rir_noise_dataset_offset, rir_noise_dataset_limit)
                                       if rir_noise_dataset else [])                     # repair (1): (offset, limit)
        if not self.clean_dataset_list or not self.noise_dataset_list:
            raise ValueError("DeviceFilePairs: the clean and the noise list must each name a file")
        if (float(reverb_proportion) > 0.0 or float(reverb_noise_proportion) > 0.0) and not self.rir_dataset_list:
            raise ValueError("DeviceFilePairs: reverberation needs rir_dataset")
        self.snr_list = parse_snr_range(snr_range)
        length = int(float(sub_sample_length) * self.SR)
        if length < 1:
            raise ValueError(f"DeviceFilePairs: sub_sample_length = {sub_sample_length} s is no sample")
        num = int(dataset_length) if dataset_length else len(self.clean_dataset_list)
        super().__init__(num=num, length=length, seed=seed, pool=1, snr_low=self.snr_list[0], snr_high=self.snr_list[-1], eq_prob=eq_prob,
                         eq_filters=eq_filters, hp_prob=hp_prob, reverb_proportion=reverb_proportion,
                         reverb_noise_proportion=reverb_noise_proportion, reverb_target=reverb_target,
                         rir_pool=max(1, len(self.rir_dataset_list)), rir_len=rir_len, predelay=predelay)
        self.silence = int(self.SR * float(silence_length))
        self.valid_mode = bool(valid_mode)
        self._rng = np.random.default_rng(self.seed * 100003 + 47)
        self.general_mix_dataset_list = self._rng.integers(0, len(self.clean_dataset_list), self.num)          # :134
        self._fp = {}              # device -> {"clean" / "noise": flat f32 pool}
        self._rirs_noise = {}      # device -> (responses, early_len, bank) of rir_noise_dataset
        self._ppin = {}            # (device, B) -> [NPIN] pinned int64 staging buffers
        self._ppin_ev = {}
        self._plan_k = 0
        self._valid_rows = None
        self.preload_stats = []    # one row per (pool, rate, channels) group: files, seconds of reading, of upload + conversion
        self.last_plan = self.last_snr = None
        for name in ("clean", "noise", "rir", "rir_noise"):
            setattr(self, name + "_utt_start", None)
            setattr(self, name + "_utt_len", None)

    # ---- preload -----------------------------------------------------------------------------------------------------
    def _load_pool(self, name: str, paths: List[str], device) -> torch.Tensor:
        """read, upload and convert the files of one list -> the flat 16 kHz pool; fills self.<name>_utt_start / _utt_len"""
        pool, start, lens, stats = load_pool(paths, device, self.SR, self.CHUNK_VALUES)
        self.preload_stats += [dict(pool=name, **row) for row in stats]
        setattr(self, name + "_utt_start", start)
        setattr(self, name + "_utt_len", lens)
        return pool

    def _ensure(self, device):
        device = torch.device(device)
        if device not in self._fp:
            with torch.cuda.device(device):
                self._fp[device] = {"clean": self._load_pool("clean", self.clean_dataset_list, device),
                                    "noise": self._load_pool("noise", self.noise_dataset_list, device)}
        return self._fp[device]

    def _rir_bank(self, name: str, paths: List[str], device):
        from . import ops
        with torch.cuda.device(device):
            pool = self._load_pool(name, paths, device)
            start, lens = getattr(self, name + "_utt_start"), getattr(self, name + "_utt_len")
            n = len(paths)
            seg = np.stack([start, np.zeros(n, dtype=np.int64), np.minimum(lens, self.rir_len)], axis=1)
            rirs = ops.assemble_clips(pool, seg, np.arange(n + 1), self.rir_len)       # cut or zero-padded to rir_len
            early = rir_early_len(rirs, self.predelay, self.SR)
            return rirs, early, ops.fft_conv_prepare(rirs, early)

    def _ensure_rirs(self, device):
        device = torch.device(device)
        if device not in self._rirs:
            if not self.rir_dataset_list:
                raise RuntimeError("DeviceFilePairs: no rir_dataset was given")
            self._rirs[device] = self._rir_bank("rir", self.rir_dataset_list, device)
        return self._rirs[device]

    def _ensure_noise_rirs(self, device):
        device = torch.device(device)
        if not self.rir_noise_dataset_list:
            return self._ensure_rirs(device)
        if device not in self._rirs_noise:
            self._rirs_noise[device] = self._rir_bank("rir_noise", self.rir_noise_dataset_list, device)
        return self._rirs_noise[device]

    def _noise_rir_bank(self, device):
        return self._ensure_noise_rirs(device)[2]

    # ---- report ------------------------------------------------------------------------------------------------------
    def screen(self, device) -> dict:
        """The statistics table of cruse_amd.screen.screen_files for what this dataset holds on `device` (preloading it if no batch
        was drawn yet; no file is read twice): {"clean": table, "noise": table, "rir": table, "rir_noise": table}, the last two only
        where their lists were given, and with the RT60 columns.  The clean and noise tables are over the flat pools; the RIR tables
        over the bank rows as the reverberation uses them, i.e. every response cut to rir_len.  Report only: nothing is filtered
        (every reason is "", keep names every file), no generator is consumed and no batch changes."""
        from . import screen as S
        device = torch.device(device)
        pools = self._ensure(device)
        out = {}
        with torch.cuda.device(device):
            for name, paths in (("clean", self.clean_dataset_list), ("noise", self.noise_dataset_list)):
                start, lens = getattr(self, name + "_utt_start"), getattr(self, name + "_utt_len")
                stats, _ = S.stats_of(pools[name], start, lens, self.SR)
                out[name] = S.table(paths, lens, self.SR, stats, None)
            for name, paths, bank in (("rir", self.rir_dataset_list, self._ensure_rirs),
                                      ("rir_noise", self.rir_noise_dataset_list, self._ensure_noise_rirs)):
                if not paths:
                    continue
                rirs = bank(device)[0]                         # [n, rir_len], cut or zero-padded
                lens = np.minimum(getattr(self, name + "_utt_len"), self.rir_len)
                stats, rt = S.stats_of(rirs.reshape(-1), np.arange(len(paths), dtype=np.int64) * self.rir_len, lens, self.SR, with_rt60=True)
                out[name] = S.table(paths, lens, self.SR, stats, rt)
        return out

    # ---- draws -------------------------------------------------------------------------------------------------------
    def _rows(self, rng, proportion: float, n: int) -> int:
        """SynDataset._select_rir (:205-213) as a row: a response with probability `proportion`, else -1"""
        use = rng.random() < proportion
        return int(rng.integers(n)) if use else -1

    def _draw_reverb_rows(self, B: int):
        if self._valid_rows is not None:                       # valid_mode: drawn with the items' own generators in _gather
            rows, self._valid_rows = self._valid_rows, None
            return rows
        return (self.draw_reverb_index(B, self.reverb_proportion, rows=len(self.rir_dataset_list)),
                self.draw_reverb_index(B, self.reverb_noise_proportion, rows=len(self.rir_noise_dataset_list or self.rir_dataset_list)))

    def plan_batch(self, items: Sequence[int]):
        """-> (clean seg [nc, 3], clean first [B + 1], noise seg, noise first, snr f32 [B]) for the items, on the host; needs the length
        tables (a preload).  Consumes the dataset's generator unless valid_mode."""
        segs, firsts, snr = ([], []), ([0], [0]), []
        rows_c, rows_n = [], []
        nr, nrn = len(self.rir_dataset_list), len(self.rir_noise_dataset_list or self.rir_dataset_list)
        for i in items:
            rng = np.random.default_rng([self.seed * 100003 + 47, int(i)]) if self.valid_mode else self._rng
            pc = plan_clip(int(self.general_mix_dataset_list[i]), self.clean_utt_len, self.length, self.silence, rng)
            pn = plan_clip(None, self.noise_utt_len, self.length, self.silence, rng)
            snr.append(self.snr_list[int(rng.integers(len(self.snr_list)))])
            if self.valid_mode and self.reverberates:
                rows_c.append(self._rows(rng, self.reverb_proportion, nr))
                rows_n.append(self._rows(rng, self.reverb_noise_proportion, nrn))
            for k, (p, st) in enumerate(((pc, self.clean_utt_start), (pn, self.noise_utt_start))):
                segs[k].append(np.stack([st[p[:, 0]] + p[:, 1], p[:, 2], p[:, 3]], axis=1))
                firsts[k].append(firsts[k][-1] + p.shape[0])
        if self.valid_mode and self.reverberates:
            self._valid_rows = (np.asarray(rows_c, dtype=np.int32), np.asarray(rows_n, dtype=np.int32))
        return (np.concatenate(segs[0]).astype(np.int64), np.asarray(firsts[0], dtype=np.int32), np.concatenate(segs[1]).astype(np.int64),
                np.asarray(firsts[1], dtype=np.int32), np.asarray(snr, dtype=np.float32))

    # ---- a batch -----------------------------------------------------------------------------------------------------
    def _gather(self, idx: torch.Tensor, device):
        """the plans of the batch on the host, one staged copy, one cruse_assemble_clips per tensor (idx on the device costs a
        synchronising read: the trainer hands host indices)"""
        from . import ops
        device = torch.device(device)
        pools = self._ensure(device)
        items = [int(i) % self.num for i in idx.tolist()]
        B = len(items)
        seg_c, first_c, seg_n, first_n, snr = self.plan_batch(items)
        nc, nn, hf, hs = seg_c.shape[0], seg_n.shape[0], (B + 2) // 2, (B + 1) // 2       # int64 words: int32 [B + 1], f32 [B]
        words = 3 * nc + 3 * nn + 2 * hf + hs
        key = (device, B)
        if key not in self._ppin:
            self._ppin[key] = [None] * self.NPIN
            self._ppin_ev[key] = [None] * self.NPIN
        slot = self._plan_k % self.NPIN
        self._plan_k += 1
        ev = self._ppin_ev[key][slot]
        if ev is not None:
            ev.synchronize()                                   # the copy issued NPIN batches ago: a wait on that event, not on the stream
        buf = self._ppin[key][slot]
        if buf is None or buf.numel() < words:                 # grown after the wait above: the old buffer is no longer read
            buf = self._ppin[key][slot] = torch.empty(max(2 * words, 1024), dtype=torch.int64).pin_memory()
        a = buf.numpy()
        o_n, o_fc = 3 * nc, 3 * nc + 3 * nn
        o_fn, o_s = o_fc + hf, o_fc + 2 * hf
        a[:o_n] = seg_c.ravel()
        a[o_n:o_fc] = seg_n.ravel()
        a[o_fc:o_fn].view(np.int32)[:B + 1] = first_c
        a[o_fn:o_s].view(np.int32)[:B + 1] = first_n
        a[o_s:words].view(np.float32)[:B] = snr
        dev = buf[:words].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._ppin_ev[key][slot] = ev
        self.last_plan, self.last_snr = (seg_c, first_c, seg_n, first_n), snr
        c = ops.assemble_clips(pools["clean"], seg_c, first_c, self.length, seg_dev=dev[:o_n].view(nc, 3),
                               first_dev=dev[o_fc:o_fn].view(torch.int32)[:B + 1])
        n = ops.assemble_clips(pools["noise"], seg_n, first_n, self.length, seg_dev=dev[o_n:o_fc].view(nn, 3),
                               first_dev=dev[o_fn:o_s].view(torch.int32)[:B + 1])
        return c, n, dev[o_s:words].view(torch.float32)[:B]
