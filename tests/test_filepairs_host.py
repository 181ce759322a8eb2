"""Host: the planning, list handling and WAV reading under filepairs.DeviceFilePairs against the restated reference of
tests/filepairs_ref.py.  No device: the kernels' side is tests/test_gpu_assemble.py and tests/test_gpu_file_dataset.py."""
import numpy as np
import pytest

import filepairs_ref as R
from cruse_amd import wavio

UTTS = [np.random.default_rng(k).standard_normal(n) for k, n in enumerate([300, 1200, 50, 777, 4000, 2500])]
LENS = [len(u) for u in UTTS]


def both(first, target, silence, seed, utts=UTTS):
    """-> (reference clip, plan rows, the two generators after the call)"""
    from cruse_amd.filepairs import plan_clip
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    want = R.select_ref(first, utts, target, silence, a)
    rows = plan_clip(first, [len(u) for u in utts], target, silence, b)
    return want, rows, a, b


def agree(first, target, silence, seed, utts=UTTS):
    want, rows, a, b = both(first, target, silence, seed, utts)
    assert rows.dtype == np.int64 and rows.ndim == 2 and rows.shape[1] == 4
    assert np.array_equal(R.execute_plan(rows, utts, target), want)       # sample for sample
    assert a.integers(1 << 30) == b.integers(1 << 30)                      # ... and the same draws consumed
    if rows.shape[0] > 1:
        assert np.all(rows[1:, 2] >= rows[:-1, 2] + rows[:-1, 3])          # ascending in dst, no overlap
    assert np.all(rows[:, 3] >= 1) and np.all(rows[:, 2] >= 0) and np.all(rows[:, 2] + rows[:, 3] <= target)
    return rows


def test_first_utterance_longer_than_the_target_is_cropped_only():
    rows = agree(4, 1000, 100, 0)
    assert rows.shape == (1, 4) and rows[0, 0] == 4 and rows[0, 2] == 0 and rows[0, 3] == 1000 and 0 <= rows[0, 1] < 3000


def test_exact_fit_is_not_cropped_and_draws_nothing():
    want, rows, a, b = both(1, 1200, 100, 1)
    assert rows.tolist() == [[1, 0, 0, 1200]] and np.array_equal(want, UTTS[1])
    fresh = np.random.default_rng(1)
    assert b.integers(1 << 30) == fresh.integers(1 << 30)                  # the generator is untouched


def test_several_utterances_with_silence_gaps():
    hit = 0
    for seed in range(12):
        rows = agree(0, 4000, 160, seed, UTTS[:4])                            # no utterance fills the clip alone
        hit += rows.shape[0] >= 3
    assert hit >= 8
    rows = agree(2, 3000, 500, 5, UTTS[:4])
    clip = R.execute_plan(rows, UTTS, 3000)
    assert (clip == 0.0).sum() >= 100                                      # there is silence inside


def test_silence_zero():
    for seed in range(6):
        rows = agree(0, 4000, 0, seed)
        assert np.array_equal(rows[1:, 2], rows[:-1, 2] + rows[:-1, 3])    # the pieces abut
    assert rows[-1, 2] + rows[-1, 3] == 4000


def test_a_gap_cut_by_the_crop_at_either_end():
    """Gaps of 1000 between utterances of 100 and 3000.  A gap is only ever appended while the clip is short of its target, so it is cut
    at the END by min(remain, silence) (the clip then closes in silence, uncropped) and at the START by a crop that begins inside it
    (after a long utterance overshot the target)."""
    utts = [np.full(100, 1.0), np.full(3000, 2.0)]
    head = tail = 0
    for seed in range(40):
        rows = agree(0, 2500, 1000, seed, utts)
        head += rows[0, 2] > 0                                             # the clip opens with the rest of a gap
        tail += rows[-1, 2] + rows[-1, 3] < 2500                           # ... or closes inside one
    assert head >= 1 and tail >= 1, (head, tail)
    short = [np.full(100, k + 1.0) for k in range(3)]                      # 100 + 2 * (100 + 1000) + 100 = 2400: the last gap is cut to 100
    for seed in range(4):
        rows = agree(0, 2500, 1000, seed, short)
        assert rows[-1, 2] + rows[-1, 3] == 2400 and rows.shape[0] == 4


def test_noise_from_empty():
    for seed in range(8):
        agree(None, 4000, 160, seed)
    rows = agree(None, 30, 160, 3)
    assert rows.shape[0] == 1 and rows[0, 3] == 30


def write_lists(tmp_path, n=6):
    """n tiny 16 kHz files per list -> the list files"""
    out = {}
    for name in ("clean", "noise", "rir", "rir_noise"):
        paths = []
        for k in range(n):
            p = tmp_path / f"{name}_{k}.wav"
            R.write_wav(p, R.to_pcm(R.harmonic(400 + 37 * k, 16000, 10 * k + len(out))), 16000)
            paths.append(str(p))
        lst = tmp_path / f"{name}.lst"
        lst.write_text("\n".join(paths) + "\n")
        out[name] = (str(lst), paths)
    return out


def make(lists, **kw):
    from cruse_amd.filepairs import DeviceFilePairs
    args = dict(clean_dataset=lists["clean"][0], noise_dataset=lists["noise"][0], snr_range=[-5, 20], silence_length=0.01, sub_sample_length=0.1,
                dataset_length=16, seed=3)
    args.update(kw)
    return DeviceFilePairs(**args)


def with_tables(ds):
    """the host tables a preload would leave (every file is at 16 kHz here: length = frames)"""
    for name, lst in (("clean", ds.clean_dataset_list), ("noise", ds.noise_dataset_list)):
        lens = np.array([wavio.read_pcm16(p)[0].shape[0] for p in lst], dtype=np.int64)
        setattr(ds, name + "_utt_len", lens)
        setattr(ds, name + "_utt_start", np.concatenate([[0], np.cumsum(lens)[:-1]]))
    return ds


def test_valid_mode_plans_are_a_function_of_the_item_and_train_plans_move_on(tmp_path):
    lists = write_lists(tmp_path)
    v = with_tables(make(lists, valid_mode=True))
    first = v.plan_batch([3, 0, 7])
    again = v.plan_batch([3, 0, 7])                                         # the next epoch
    other = with_tables(make(lists, valid_mode=True)).plan_batch([7])      # another call shape, another object
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    n7 = first[1][3] - first[1][2]
    assert np.array_equal(other[0], first[0][first[1][2]:first[1][3]]) and other[0].shape[0] == n7 and other[4][0] == first[4][2]
    t = with_tables(make(lists))
    e1, e2 = t.plan_batch([3, 0, 7]), t.plan_batch([3, 0, 7])
    assert not (np.array_equal(e1[0], e2[0]) and np.array_equal(e1[2], e2[2]))
    t2 = with_tables(make(lists))
    for a, b in zip(e1, t2.plan_batch([3, 0, 7])):                         # one seed, one stream
        assert np.array_equal(a, b)
    assert set(np.unique(first[4]).tolist()) <= set(range(-5, 21)) and first[4].dtype == np.float32
    assert v.general_mix_dataset_list.shape == (16,) and np.array_equal(v.general_mix_dataset_list, t.general_mix_dataset_list)
    assert v.length == 1600 and len(v) == 16 and v.silence == 160 and v.snr_list == list(range(-5, 21))


def test_offset_and_limit_and_the_repaired_noise_rir_arguments(tmp_path):
    assert wavio.offset_and_limit(list("abcdef"), 2, 3) == list("cde")
    assert wavio.offset_and_limit(list("abcdef"), 4, None) == list("ef") and wavio.offset_and_limit(list("abcdef"), 0, 0) == list("abcdef")
    lists = write_lists(tmp_path)
    ds = make(lists, clean_dataset_offset=1, clean_dataset_limit=4, noise_dataset_offset=2, rir_dataset=lists["rir"][0], rir_dataset_limit=2,
              rir_noise_dataset=lists["rir_noise"][0], rir_noise_dataset_offset=1, rir_noise_dataset_limit=3, dataset_length=None)
    assert ds.clean_dataset_list == lists["clean"][1][1:5] and ds.noise_dataset_list == lists["noise"][1][2:]
    assert ds.rir_dataset_list == lists["rir"][1][:2]
    assert ds.rir_noise_dataset_list == lists["rir_noise"][1][1:4]           # (offset 1, limit 3); the reference's swap would give [3:4]
    assert len(ds) == 4 and ds.rir_pool == 2
    with pytest.raises(ValueError, match="16000"):
        make(lists, sr=8000)
    with pytest.raises(ValueError, match="rir_dataset"):
        make(lists, reverb_proportion=0.5)
    make(lists, target_dB_FS=-25, target_dB_FS_floating_val=10, pre_load_clean_dataset=False, pre_load_noise=False, pre_load_rir=False, num_workers=8)
    import dataset.dataset as DS
    from cruse_amd.filepairs import DeviceFilePairs
    assert DS.DeviceFilePairs is DeviceFilePairs


def test_wav_round_trip_and_refusals(tmp_path):
    mono = R.to_pcm(R.harmonic(801, 22050, 1))
    R.write_wav(tmp_path / "m.wav", mono, 22050)
    pcm, ch, rate = wavio.read_pcm16(str(tmp_path / "m.wav"))
    assert pcm.dtype == np.int16 and np.array_equal(pcm, mono) and (ch, rate) == (1, 22050)
    stereo = np.stack([R.to_pcm(R.harmonic(333, 48000, 2)), R.to_pcm(R.harmonic(333, 48000, 3))], axis=1).reshape(-1)
    R.write_wav(tmp_path / "s.wav", stereo, 48000, channels=2)
    pcm, ch, rate = wavio.read_pcm16(str(tmp_path / "s.wav"))
    assert np.array_equal(pcm, stereo) and (ch, rate) == (2, 48000) and pcm.shape == (666,)
    R.write_wav(tmp_path / "b.wav", np.arange(100, dtype=np.uint8), 16000, width=1)
    with pytest.raises(ValueError, match=r"b\.wav.*8-bit"):
        wavio.read_pcm16(str(tmp_path / "b.wav"))
    (tmp_path / "n.wav").write_bytes(b"OggS" + bytes(100))
    with pytest.raises(ValueError, match=r"n\.wav"):
        wavio.read_pcm16(str(tmp_path / "n.wav"))
    lst = tmp_path / "l.lst"
    lst.write_text("~/a.wav\n/x/b.wav\n\n")
    import os
    assert wavio.read_list(str(lst)) == [os.path.expanduser("~/a.wav"), "/x/b.wav"]


def test_check_clip_plan_refuses_malformed_plans():
    from cruse_amd.ops import check_clip_plan
    ok = np.array([[0, 0, 10], [50, 20, 5], [3, 0, 7]], dtype=np.int64)
    check_clip_plan(ok, [0, 2, 3], 2, 30, 100)
    check_clip_plan(np.zeros((0, 3), dtype=np.int64), [0, 0], 1, 30, 100)  # all silence
    for seg, first, B in ((np.array([[0, 0, 10], [50, 9, 5]], dtype=np.int64), [0, 2], 1),      # overlap
                          (np.array([[0, 20, 10], [50, 0, 5]], dtype=np.int64), [0, 2], 1),     # descending
                          (np.array([[0, 25, 10]], dtype=np.int64), [0, 1], 1),                 # leaves the clip
                          (np.array([[95, 0, 10]], dtype=np.int64), [0, 1], 1),                 # leaves the pool
                          (np.array([[0, 0, 0]], dtype=np.int64), [0, 1], 1),                   # empty
                          (ok, [0, 2, 2], 2), (ok.astype(np.int32), [0, 2, 3], 2)):
        with pytest.raises(ValueError):
            check_clip_plan(seg, first, B, 30, 100)
