"""Host: the low-pass of cruse_resample_poly (cruse_amd/resample_design.py): sizes, symmetry, the phase-major table,
the direct-sum restatement against scipy in float64, and the measured response of the 44.1 kHz design."""
import numpy as np
import pytest
from scipy import signal

import filepairs_ref as R
from cruse_amd import resample_design as D

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)
RATIOS = {8000: (2, 1), 11025: (640, 441), 22050: (320, 441), 24000: (2, 3), 32000: (1, 2), 44100: (160, 441), 48000: (1, 3), 96000: (1, 6)}


@pytest.mark.parametrize("rate", RATES)
def test_taps(rate):
    up, down = D.ratio(16000, rate)
    assert (up, down) == RATIOS[rate]
    h = D.design(up, down)
    q = max(up, down)
    assert h.dtype == np.float64 and h.shape == (32 * q + 1,)
    assert abs(h.sum() - 1.0) <= 1e-13
    assert np.array_equal(h, h[::-1])                                    # symmetric: zero phase about tap 16 q
    assert h.argmax() == 16 * q
    assert D.taps_per_phase(up, down) == -(-(32 * q + 1) // up)


def test_taps_per_output_of_the_issue():
    assert [D.taps_per_phase(*D.ratio(16000, r)) for r in (44100, 11025, 48000)] == [89, 33, 97]


def test_the_streaming_design_is_the_same_filter():
    from cruse_amd.inferencer import resample as S
    for rate, (up, down) in ((8000, (2, 1)), (32000, (1, 2)), (48000, (1, 3))):
        assert np.array_equal(S.design(rate)[1], D.design(up, down))


@pytest.mark.parametrize("rate", RATES)
def test_phase_table_round_trips(rate):
    up, down = D.ratio(16000, rate)
    h = D.design(up, down)
    tab = D.phase_table(h, up)
    T = D.taps_per_phase(up, down)
    assert tab.shape == (up, (T + 3) // 4 * 4) and tab.dtype == h.dtype
    assert np.array_equal(D.from_phase_table(tab, h.shape[0]), h)
    for p, j in ((0, 0), (up - 1, 0), (up // 2, T - 1), (0, T - 1)):
        k = p + up * j
        assert tab[p, j] == (h[k] if k < h.shape[0] else 0.0)
    assert not tab[:, T:].any()
    t32 = D.phase_table(h.astype(np.float32), up)
    assert t32.dtype == np.float32 and np.array_equal(t32, tab.astype(np.float32))     # rounded once


@pytest.mark.parametrize("rate", RATES)
def test_direct_sum_is_scipy_resample_poly(rate):
    up, down = D.ratio(16000, rate)
    x = R.harmonic(1237, rate, 7)
    want = signal.resample_poly(x, up, down, window=D.design(up, down))
    got = D.direct_sum(x, up, down, D.design(up, down))
    assert got.shape == want.shape == (D.out_len(1237, up, down),)
    e = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"{rate} Hz: direct sum vs scipy, rel-L2 {e:.1e}")
    assert e <= 1e-12


def test_out_len_and_refusals():
    assert [D.out_len(L, 160, 441) for L in (1, 441, 442, 2822, 2823)] == [1, 160, 161, 1024, 1025]
    for bad in ((1025, 1), (1, 1025), (2, 4), (0, 1)):
        with pytest.raises(ValueError):
            D.design(*bad)
    with pytest.raises(ValueError):
        D.ratio(16000, 0)


def test_response_of_the_44100_design():
    """Measured: within +0.0004 / -0.022 dB up to 6 kHz, -0.61 dB at 6.5 kHz, -6.02 dB at 7.2 kHz (the cutoff 0.9 * 8 kHz),
    -27.5 dB at 8 kHz, below -62.5 dB from 8.5 kHz and below -93.7 dB from 9 kHz.  Pinned with a small margin."""
    up, down = D.ratio(16000, 44100)
    h = D.design(up, down)
    fs, nfft = up * 44100, 1 << 22
    db = 20 * np.log10(np.maximum(np.abs(np.fft.rfft(h, nfft)), 1e-300))
    f = np.arange(db.shape[0]) * fs / nfft
    at = lambda hz: db[np.searchsorted(f, hz)]
    assert db[f <= 6000].max() <= 0.001 and db[f <= 6000].min() >= -0.025
    assert -0.65 <= at(6500) <= -0.57
    assert -6.1 <= at(7200) <= -5.95
    assert -28.0 <= at(8000) <= -27.0
    assert db[f >= 8500].max() <= -62.0
    assert db[f >= 9000].max() <= -93.0
