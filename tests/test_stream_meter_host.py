"""CPU: the float64 restatement of the streaming level meters and voice-activity detector (tests/stream_meter_ref.py), the host surface
of cruse_stream_meter / _meter_n (header, ctypes table, library, refusals) and the decision margin tests/test_gpu_stream_meter.py relies
on: no frame of the float64 reference of the committed inputs has |p - threshold| < 1e-3, so a kernel within 1e-3 of p decides alike."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from cruse_amd.inferencer.packets import flush_plan, packet_plan
from tests import stream_meter_ref as M
from tests.stream_ref import frame_of, stream_clip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("cruse_stream_meter_layout", "cruse_stream_meter", "cruse_stream_meter_n")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_power_is_the_mean_square_of_the_windowed_frame():
    """Parseval: P_in from the one-sided spectrum = sum((w x)^2) / W2, to 1e-12; a stationary signal of mean square sigma^2 reads sigma^2"""
    assert abs(M.W2 - 120.0) < 1e-9                           # a periodic Hann window: 3 N / 8
    for i, L in enumerate((320, 1600)):
        x = M.clip(L, i).double()
        for t in range(L // 160 + 1):
            fr = frame_of(x, t).numpy() * M.WIN
            spec = np.fft.rfft(fr)
            want = float(np.sum(fr ** 2) / M.W2)
            got = M.power(spec.real, spec.imag)
            assert abs(got - want) <= 1e-12 * max(want, 1.0), (L, t, got, want)
    rng = np.random.default_rng(1)
    est = []
    for _ in range(400):
        spec = np.fft.rfft(0.05 * rng.standard_normal(320) * M.WIN)
        est.append(M.power(spec.real, spec.imag))
    assert abs(np.mean(est) / 0.05 ** 2 - 1.0) < 0.05
    g = np.full(161, 0.5)
    assert abs(M.power(spec.real, spec.imag, g) - 0.25 * M.power(spec.real, spec.imag)) < 1e-18
    assert M.level(0.0) == -120.0


def test_per_hop_constants_reproduce_the_references_windows():
    d = M.DEFAULTS
    for per_hop, per_window in ((d["attack"], 0.8), (d["release"], 0.05)):
        p = 0.0
        for _ in range(5):                                    # five hops towards a constant p_raw = 1
            p += per_hop * (1.0 - p)
        assert abs(p - per_window) <= 1e-12
        assert abs(1.0 - (1.0 - per_hop) ** 5 - per_window) <= 1e-12
    assert d["threshold"] == 0.13
    # x = a + b + 10 log10(sum of 800 squares) on a clip at -25 dBFS is L - level_db on absolute levels
    want = -25.0 - (-1.0 + 0.2 + 10.0 * math.log10(800.0)) - (-25.0)
    assert abs(d["level_db"] - want) <= 1e-12 and abs(d["level_db"] + 28.23) < 5e-3
    sig = 10.0 ** (-25.0 / 20.0)
    x_ref = -1.0 + 0.2 + 10.0 * math.log10(800 * sig ** 2)
    assert abs((10.0 * math.log10(sig ** 2) - d["level_db"]) - x_ref) < 1e-12
    from cruse_amd import ops
    assert ops.stream_vad_defaults() == pytest.approx(d, rel=0, abs=1e-15)


def test_gain_restates_the_decode_kernels():
    m = np.linspace(0.0, 1.0, 160)
    assert np.array_equal(M.gain(m)[:160], m) and M.gain(m)[160] == 0.0
    g = M.gain(m, lim=0.25)
    assert np.allclose(g[:160], 0.25 + 0.75 * m, rtol=0, atol=1e-15) and g[160] == 0.25
    assert np.array_equal(M.gain(m, lim=1.0), np.ones(161))                     # 0 dB: the input passes
    for kind in (1, 2):
        assert np.array_equal(M.gain(m, tau=0.0, kind=kind), M.gain(m))         # tau == 0: the bypass
        pf = M.post_filter(m, 0.02, kind)
        assert pf[0] == 0.0 and abs(pf[-1] - 1.0) < 1e-12 and np.all(pf <= m + 1e-15)
        assert np.allclose(M.gain(m, lim=0.5, tau=0.02, kind=kind)[:160], 0.5 + 0.5 * pf, rtol=0, atol=1e-15)
    # the offline kernel's float64 restatement of the same header agrees
    s = np.sin(0.5 * np.pi * m)
    assert np.allclose(M.post_filter(m, 0.02, 1), m * (1.02 * s * s) / (s * s + 0.02), rtol=0, atol=1e-15)


@functools.lru_cache(maxsize=None)
def rows64(name, L, i):
    _, frames = stream_clip(M.model64(name), M.clip(L, i).double(), dtype=torch.float64)
    return M.rows_of(frames)


def _splits(nb, cmax):
    if nb == 0:
        yield ()
        return
    for c in range(1, min(cmax, nb) + 1):
        for rest in _splits(nb - c, cmax):
            yield (c,) + rest


def test_frame0_rule_and_alignment_agree_for_every_split():
    rows = rows64("small_g2", 1600, 0)
    nb = 10
    want, ref = M.meter_clip(rows)
    assert want.shape == (nb, 4) and ref.acc[0] == nb
    n = 0
    for split in _splits(nb, 4):
        m = M.Meter()
        m.p, m.acc = 0.7, np.array([5.0, 5.0, 1.0, 1.0])                        # frame 0 resets whatever the state held
        got, b = np.zeros((nb, 4)), 0
        for c in (0,) + split + (0,):
            p = packet_plan(b, c)
            assert p.n_frames == M.frames_of_packet(p.start, c)[0] and (p.n_frames == 0 or (p.first_frame == 0) == M.frames_of_packet(p.start, c)[1])
            r, _ = M.meter_clip(rows[p.first_frame:p.first_frame + p.n_frames], first=p.first_frame, meter=m)
            assert len(r) == p.n_out                                            # one row per block returned, aligned with it
            got[p.first_out:p.first_out + p.n_out] = r
            b += c
        p = flush_plan(b)
        r, _ = M.meter_clip(rows[p.first_frame:p.first_frame + 1], first=p.first_frame, meter=m)
        assert len(r) == 1 and p.first_out == nb - 1
        got[p.first_out] = r[0]
        assert np.array_equal(got, want) and np.array_equal(m.acc, ref.acc), split
        n += 1
    assert n == 401                                           # the compositions of 10 into parts of at most 4
    # the first row belongs to frame 1, and frame 0 took part in the recursion
    skipped, _ = M.meter_clip(rows[1:], first=1)
    assert np.array_equal(skipped[:, :2], want[:, :2]) and skipped[0, 2] != want[0, 2]
    a = ref.activity()
    assert a[0] == nb and 0 <= a[1] <= nb and M.Meter().activity().tolist() == [0.0, 0.0, -120.0, -120.0]


# ---- the decision margin of the committed inputs ---------------------------------------------------------------------------------------
def test_margin_of_the_kernel_level_inputs():
    worst = math.inf
    for form in M.KERNEL_FORMS:
        _, lim, kind, tau = form
        for s in range(M.S):
            r, m = M.meter_clip(M.kernel_slot_rows(s)[:M.KERNEL_FRAMES], lim=lim, tau=tau, kind=kind)
            worst = min(worst, M.min_margin(r, m.par["threshold"]))
            assert 0 < r[:, 3].sum() < len(r), (form[0], s)   # the inputs exercise both decisions
        for name, calls in M.KERNEL_PACKETS.items():
            out, meters = M.run_packet_case(calls, form)
            for per in out:
                for s, (_, _, want) in enumerate(per):
                    worst = min(worst, M.min_margin(want, meters[s].par["threshold"]))
    print(f"kernel-level inputs: min |p - threshold| = {worst:.3e}")
    assert worst >= M.MARGIN


def _switched(rows):
    m = M.Meter(lim=0.0)
    a, _ = M.meter_clip(rows[:M.SWITCH_AT], meter=m)
    m.set(lim=10.0 ** (-M.SWITCH_LIM_DB / 20.0), **M.SWITCH_VAD)
    b, _ = M.meter_clip(rows[M.SWITCH_AT:], first=M.SWITCH_AT, meter=m)
    return a, b, m


def test_margin_of_the_server_level_inputs():
    worst = math.inf
    for name in M.CONFIGS:
        for L in M.LENGTHS:
            for i in range(M.S):
                rows = rows64(name, L, i)
                for form in M.SERVER_FORMS:
                    r, m = M.meter_clip(rows, **M.form_kwargs(form))
                    assert r.shape == (L // 160, 4)
                    worst = min(worst, M.min_margin(r, m.par["threshold"]))
                if L == 1600:
                    a, b, m = _switched(rows)
                    worst = min(worst, M.min_margin(a, M.DEFAULTS["threshold"]), M.min_margin(b, m.par["threshold"]))
    print(f"server-level inputs: min |p - threshold| = {worst:.3e}")
    assert worst >= M.MARGIN


# ---- the host surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    from cruse_amd._abi_check import parse_header
    from cruse_amd._lib import ABI_VERSION, SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "cruse_hip.h")).read()
    assert "#define CRUSE_ABI_VERSION 15" in header and ABI_VERSION == 15 and lib.cruse_abi_version() == 15       # additive symbols
    parsed = parse_header()
    for sym in SYMBOLS:
        assert re.search(rf"\bint {sym}\(", header), f"{sym} is not declared in include/cruse_hip.h"
        assert SIGNATURES[sym] == parsed[sym]
        assert hasattr(lib, sym)
    assert SIGNATURES["cruse_stream_meter"][0] == "pipiiiippipppippip" and SIGNATURES["cruse_stream_meter_n"][0] == "piiiipiiiippipppippip"
    assert "stream_meter" in open(os.path.join(ROOT, "cruse_amd", "csrc", "build.sh")).read()
    from cruse_amd import ops
    lay = ops.stream_meter_layout()
    assert lay["row"] == 4 and lay["acc"] == 4 and 0 <= lay["p"] < lay["stride"]
    # not a boundary-plan entry: its 14 entries stay
    assert len(ops.STREAM_BOUNDARY_ENTRIES) == 14 and not any("meter" in e for e in ops.STREAM_BOUNDARY_ENTRIES)


WK = 2048                                                     # a work row stride with room for the three rows
# the arguments of a call that would launch, by name, in the order of the header; pointers: 1 = a buffer, 0 = null
GOOD = dict(ctl=1, S=3, hops=4, out_hops=4, work_frames=5, work=1, wk_stride=WK, wk_re=0, wk_im=161, wk_mask=322, tab=1, lim=1, pf_kind=1,
            pf_tau=1, vad_par=1, meter_state=1, st_stride=4, meter_acc=1, out=1, out_stride=16)
PACKET_ONLY = ("hops", "out_hops", "work_frames")
REFUSALS = [
    (dict(S=0), "S = 0"),
    (dict(ctl=0), "null buffer"), (dict(work=0), "null buffer"), (dict(tab=0), "null buffer"), (dict(vad_par=0), "null buffer"),
    (dict(meter_state=0), "null buffer"), (dict(meter_acc=0), "null buffer"), (dict(out=0), "null buffer"),
    (dict(pf_tau=0), "null buffer (pf_kind 1 needs pf_tau)"),
    (dict(wk_re=WK - 160), "do not lie in a work row"), (dict(wk_im=-1), "do not lie in a work row"),
    (dict(wk_mask=WK - 159), "do not lie in a work row"), (dict(wk_stride=481, wk_re=0, wk_im=161, wk_mask=321), "do not lie in a work row"),
    (dict(pf_kind=3), "post-filter kind 3"), (dict(pf_kind=-1), "post-filter kind -1"),
    (dict(st_stride=3), "meter_state rows of 3 floats"),
]
REFUSALS_1 = [(dict(out_stride=3), "out rows of 3 floats")]
REFUSALS_N = [(dict(hops=0), "hops = 0"), (dict(hops=65, out_hops=65, work_frames=66, out_stride=260), "hops = 65"),
              (dict(work_frames=4), "work_frames = 4"), (dict(out_hops=3), "out_hops = 3"), (dict(out_stride=15), "out rows of 15 floats")]


def _call(packet, **change):
    """(return code, message) of the real entry point on stand-in pointers (the host only asks whether a pointer is null; where a device
    is present the stand-in is device memory larger than any tensor of these calls, as in tests/test_stream_boundary_host.py)"""
    from cruse_amd._lib import lib
    from tests.test_stream_boundary_host import standin
    a = dict(GOOD, **change)
    if not packet:
        a["out_stride"] = change.get("out_stride", 4)
    P = standin()
    vals = [(P if v else None) if k in ("ctl", "work", "tab", "lim", "pf_tau", "vad_par", "meter_state", "meter_acc", "out") else v
            for k, v in a.items() if packet or k not in PACKET_ONLY]
    fn = lib.cruse_stream_meter_n if packet else lib.cruse_stream_meter
    rc = fn(*vals, None)
    return rc, lib.cruse_last_error().decode()


@pytest.mark.parametrize("packet", [False, True], ids=["meter", "meter_n"])
def test_every_refusal_comes_with_its_code_and_message(packet):
    who = "cruse_stream_meter_n" if packet else "cruse_stream_meter"
    for change, msg in REFUSALS + (REFUSALS_N if packet else REFUSALS_1):
        rc, said = _call(packet, **change)
        assert rc == -1 and said.startswith(who + ":") and msg in said, (change, rc, said)
    from cruse_amd._lib import lib
    assert lib.cruse_stream_meter_layout(None) == -1 and b"stream_meter_layout: null output" in lib.cruse_last_error()
    out = (ctypes.c_int * 4)()
    assert lib.cruse_stream_meter_layout(out) == 0 and list(out) == [0, 4, 4, 4]


def test_server_arguments_are_refused_on_the_host():
    """meters with head="df" raises a ValueError naming the argument before anything touches a device"""
    from cruse_amd.inferencer import StreamingInferencer

    class Model(torch.nn.Module):
        pass
    with pytest.raises(ValueError, match="meters"):
        StreamingInferencer(Model(), 1, head="df", meters=True, device="cpu")
