"""CPU: the rate converters of StreamingInferencer(io_rate=...) -- the package's filter design (cruse_amd/inferencer/resample.py) against
the restatement of tests/stream_rs_ref.py, the filter's response, the restatement's own consistency (block by block == whole clip) and
what In then Out does to a signal inside the pass band: a pure delay of io_delay samples.
"""
import math

import numpy as np
import pytest
import torch

from cruse_amd.inferencer import resample
from tests import stream_rs_ref as RS

RATES = RS.RATES


@pytest.mark.parametrize("io_rate", RATES)
def test_design_equals_the_restatement(io_rate):
    q, h = resample.design(io_rate)
    want = RS.design(io_rate)
    assert q == RS.ratio(io_rate) and h.dtype == np.float64 and h.shape == (32 * q + 1,)
    d = float(np.abs(h - want.numpy()).max())
    print(f"io_rate {io_rate}: design() vs the restatement, max abs {d:.2e}")
    assert d <= 1e-15
    assert abs(h.sum() - 1.0) <= 1e-15 and float(np.abs(h - h[::-1]).max()) <= 1e-16          # unit DC gain, linear phase
    assert resample.io_block(io_rate) == io_rate // 100 and resample.io_delay(io_rate) == RS.io_delay(io_rate)
    N = 32 * q + 1
    assert resample.history(io_rate) == (((N - 1) // 2, N - 1) if io_rate == 8000 else (N - 1, (N - 1) // q))


def test_sixteen_kilohertz_and_unknown_rates():
    assert resample.io_block(16000) == 160 and resample.io_delay(16000) == 0 and resample.history(16000) == (0, 0)
    for bad in (44100, 0, None, "48000"):
        with pytest.raises(ValueError, match="8000, 16000, 32000, 48000"):
            resample.check_rate(bad)
    with pytest.raises(ValueError):
        resample.design(16000)


@pytest.mark.parametrize("io_rate", RATES)
def test_response(io_rate):
    """the four figures of the design: pass-band peak, 0.8 x and 1.0 x the low rate's Nyquist frequency, the stop band from 1.1 x on"""
    q, h = resample.design(io_rate)
    h = torch.from_numpy(h)
    nyq = 0.5 / q                                                          # cycles per sample of the higher rate
    f = torch.linspace(0.0, 0.5, 20001, dtype=torch.float64)
    g = RS.response_db(h, f)
    peak, stop = float(g[f <= nyq].max()), float(g[f >= 1.1 * nyq].max())
    at08, at10 = (float(RS.response_db(h, torch.tensor([c * nyq]))[0]) for c in (0.8, 1.0))
    print(f"io_rate {io_rate}: peak {peak:+.5f} dB, 0.8 Nyquist {at08:.4f} dB, Nyquist {at10:.3f} dB, stop band {stop:.2f} dB")
    assert abs(peak - 0.0003) <= 0.01 and abs(at08 + 0.375) <= 0.01
    assert abs(at10 + 27.5) <= 1.0 and stop <= -90.0


@pytest.mark.parametrize("io_rate", RATES)
def test_block_by_block_equals_whole_clip(io_rate):
    B = io_rate // 100
    u = 0.1 * torch.randn(7 * B, generator=torch.Generator().manual_seed(io_rate), dtype=torch.float64)
    x = RS.resample_in(u, io_rate)
    v = RS.resample_out(x, io_rate)
    assert x.shape == (7 * 160,) and v.shape == u.shape
    hi = ho = None
    xs, vs = [], []
    for b in range(7):
        xb, hi = RS.resample_in(u[b * B:(b + 1) * B], io_rate, hi, with_hist=True)
        vb, ho = RS.resample_out(xb, io_rate, ho, with_hist=True)
        assert xb.shape == (160,) and vb.shape == (B,)
        xs.append(xb)
        vs.append(vb)
    assert torch.equal(torch.cat(xs), x) and torch.equal(torch.cat(vs), v)


@pytest.mark.parametrize("io_rate", RATES)
def test_in_then_out_is_a_delay_of_io_delay(io_rate):
    """1 kHz + 2.5 kHz lie inside every rate's pass band: Out(In(u)) is u, io_delay samples late, up to the pass-band ripple and the
    aliases the stop band leaves.  The bar of 1e-4 was set at design time, when the same filters with decimation phase q - 1 measured
    1.0e-5 (q = 2) and 1.4e-5 (q = 3); with phase 0 this test measures 2.9e-5 (8 kHz), 1.6e-5 (32 kHz) and 2.2e-5 (48 kHz) rel-L2.
    One sample off is worth more than 0.1."""
    n = io_rate // 4
    t = torch.arange(n, dtype=torch.float64) / io_rate
    u = 0.5 * torch.sin(2 * math.pi * 1000.0 * t) + 0.5 * torch.sin(2 * math.pi * 2500.0 * t + 0.3)
    v = RS.resample_out(RS.resample_in(u, io_rate), io_rate)
    d = resample.io_delay(io_rate)
    err = {dd: float((v[200:] - u[200 - dd:n - dd]).norm() / u[200 - dd:n - dd].norm()) for dd in (d - 1, d, d + 1)}
    print(f"io_rate {io_rate}: Out(In(u)) vs u delayed by {d}: rel-L2 {err[d]:.2e}; by {d - 1}: {err[d - 1]:.2f}, by {d + 1}: {err[d + 1]:.2f}")
    assert err[d] <= 1e-4
    assert err[d - 1] > 0.1 and err[d + 1] > 0.1
