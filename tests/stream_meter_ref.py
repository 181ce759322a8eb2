"""Test-only: the float64 restatement of the streaming level meters and voice-activity detector (cruse_stream_meter / _meter_n,
DESIGN 12g), on the rows tests/stream_ref.py produces frame by frame (or on any rows of the same shapes).

For frame t of a slot, N_f (f = 0..160) the noisy spectrum of the windowed frame and m_f (f = 0..159) the raw mask:
  G_f    = pf(m_f) on f < 160, 0 on bin 160; with a limit lim: lim + (1 - lim) pf(m_f), and lim on bin 160 (the decode kernels' gain)
  P_in   = (|N_0|^2 + 2 sum_{f=1..159} |N_f|^2 + |N_160|^2) / (320 W2), W2 = sum_n win[n]^2;  P_out the same of G_f N_f
  L      = 10 log10(P + 1e-12)
  p      = p_prev + alpha (p_raw - p_prev), p_raw = 1 / (1 + exp(-(L_out - level_db))), alpha = attack if p_raw > p_prev else release
  vad    = p > threshold
Frame 0 of a clip resets p_prev and the accumulators, takes part in the recursion and yields no row; every later frame yields the row
[L_in, L_out, p, vad] of the output block it completes.

Defaults (the reference's activitydetector, utils/utils.py:143-183, for a clip at its -25 dBFS target): it takes
x = a + b + 10 log10(sum of 800 squared samples) = a + b + 10 log10(800) + L on the clip normalised to -25 dBFS; here x = L_out - level_db
on absolute levels, so level_db = -25 - (a + b + 10 log10(800)) - (-25) = -28.23 (a = -1, b = 0.2).  A 50 ms window is five hops:
attack = 1 - (1 - 0.8)^(1/5), release = 1 - (1 - 0.05)^(1/5).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import stream_ref as SR

NFFT, NB, F0 = SR.NFFT, 161, 160
WIN = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)             # torch.hann_window(320), periodic, float64
W2 = float(np.sum(WIN ** 2))
A_REF, B_REF, WINDOW_REF, ATT_REF, REL_REF, TARGET_REF = -1.0, 0.2, 800, 0.8, 0.05, -25.0
DEFAULTS = dict(level_db=TARGET_REF - (A_REF + B_REF + 10.0 * math.log10(WINDOW_REF)) - TARGET_REF, threshold=0.13,
                attack=1.0 - (1.0 - ATT_REF) ** 0.2, release=1.0 - (1.0 - REL_REF) ** 0.2)
KINDS = {None: 0, "iam": 1, "envelope": 2}

# the bars of tests/test_gpu_stream_meter.py: f32 sums of <= 322 non-negative terms (relative error <= 322 * 2^-24 = 1.9e-5, 8.3e-5 dB)
# and a logistic whose slope is at most 0.25 per dB, so 1e-3 dB moves p by at most 2.5e-4
BAR_DB, BAR_P, MARGIN = 1e-3, 1e-3, 1e-3


def post_filter(g, tau, kind):
    """postfilter.h in float64: kind 1 "iam", 2 "envelope"; tau == 0 or kind 0: the identity"""
    g = np.asarray(g, dtype=np.float64)
    if not kind or tau == 0.0:
        return g
    s = np.sin(0.5 * np.pi * g)
    s2, den = s * s, s * s + tau
    if kind == 1:
        return g * (((1.0 + tau) * s2) / den)
    return g * s * np.sqrt(((1.0 + tau) * s) / den)


def gain(mask, lim=None, tau=0.0, kind=0):
    """G [161] from the raw mask [160]; lim None: the kernels without a limit"""
    g = np.concatenate([post_filter(mask, tau, kind), [0.0]])
    if lim is None:
        return g
    g = lim + (1.0 - lim) * g
    g[F0] = lim
    return g


def power(re, im, g=None):
    """P of the spectrum (re, im) [161], times the gain g [161]"""
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    if g is not None:
        re, im = re * g, im * g
    w = np.full(NB, 2.0)
    w[0] = w[F0] = 1.0
    return float(np.sum(w * (re * re + im * im)) / (NFFT * W2))


def level(p):
    return 10.0 * math.log10(p + 1e-12)


class Meter:
    """one slot: p_prev and the accumulators [frames, active frames, sum P_in, sum P_out over active frames]"""

    def __init__(self, lim=None, tau=0.0, kind=0, **par):
        self.par = dict(DEFAULTS, **par)
        self.lim, self.tau, self.kind = lim, float(tau), int(kind)
        self.p, self.acc = 0.0, np.zeros(4)

    def set(self, lim=None, **par):
        """what set_vad / set_atten_lim change on a running slot: later frames only"""
        self.par.update(par)
        if lim is not None:
            self.lim = lim

    def step(self, re, im, mask, f0=False):
        """one frame; -> its row [L_in, L_out, p, vad], None for frame 0 of a clip"""
        if f0:
            self.p, self.acc = 0.0, np.zeros(4)
        pin, pout = power(re, im), power(re, im, gain(mask, self.lim, self.tau, self.kind))
        lin, lout = level(pin), level(pout)
        x = lout - self.par["level_db"]
        praw = 1.0 / (1.0 + math.exp(-x)) if x > -700.0 else 0.0
        alpha = self.par["attack"] if praw > self.p else self.par["release"]
        self.p += alpha * (praw - self.p)
        if f0:
            return None
        vad = self.p > self.par["threshold"]
        self.acc += [1.0, float(vad), pin * vad, pout * vad]
        return [lin, lout, self.p, float(vad)]

    def activity(self):
        """what StreamingInferencer.activity() returns for the slot"""
        n = max(self.acc[1], 1.0)
        return np.array([self.acc[0], self.acc[1], level(self.acc[2] / n), level(self.acc[3] / n)])


def rows_of(frames):
    """[(re, im, mask)] as float64 numpy from the intermediates of stream_ref.stream_clip, or from tensors of a server's stage()"""
    return [tuple(f[k].detach().double().cpu().numpy().reshape(-1) for k in ("re", "im", "mask")) for f in frames]


def meter_clip(rows, first=0, meter=None, **kw):
    """rows: frames first, first + 1, ... of a clip, frame 0 (first == 0) being the clip's frame 0; -> (meter rows [n, 4], the Meter)"""
    m = Meter(**kw) if meter is None else meter
    out = [m.step(*r, f0=(first + i == 0)) for i, r in enumerate(rows)]
    out = [r for r in out if r is not None]
    return np.array(out, dtype=np.float64).reshape(len(out), 4), m


def min_margin(rows4, threshold):
    """the smallest |p - threshold| of meter rows [n, 4]"""
    return float(np.min(np.abs(rows4[:, 2] - threshold))) if len(rows4) else math.inf


# ---- the committed inputs of the kernel-level GPU tests: synthetic work rows ---------------------------------------------------------
def synthetic_rows(seed, n, quiet=2):
    """n work rows (re [161], im [161], mask [160]) as float32: a complex Gaussian spectrum, `quiet` + 1 quiet frames first (the detector
    stays off), then a level that jumps between loud and quiet (it attacks and releases), and a mask in [0, 1]; the imaginary parts of
    bins 0 and 160 are zero as of a real frame"""
    rng = np.random.default_rng(seed)
    db = rng.uniform(-70.0, 10.0, n)
    db[:quiet + 1] = rng.uniform(-90.0, -70.0, min(quiet + 1, n))
    rows = []
    for t in range(n):
        a = 10.0 ** (db[t] / 20.0)
        re, im = (a * rng.standard_normal(NB)).astype(np.float32), (a * rng.standard_normal(NB)).astype(np.float32)
        im[0] = im[F0] = 0.0
        rows.append((re, im, rng.uniform(0.0, 1.0, F0).astype(np.float32)))
    return rows


# (name, lim gain or None, post-filter kind, tau): with and without a limit, each pf_kind, tau = 0
KERNEL_FORMS = [("plain", None, 0, 0.0), ("lim", 10.0 ** (-12.0 / 20.0), 0, 0.0), ("iam", None, 1, 0.02), ("envelope", None, 2, 0.02),
                ("iam_tau0", None, 1, 0.0), ("lim_iam", 10.0 ** (-6.0 / 20.0), 1, 0.05), ("lim_envelope_tau0", 0.25, 2, 0.0)]
# the kernel-level packet cases (hops = 4, 3 slots): a case is a list of calls, a call one (start, count) per slot as pk[0], pk[1] say
KERNEL_HOPS = 4
KERNEL_PACKETS = {
    "ones": [[(0, 1)] * 3, [(1, 1)] * 3, [(2, 1)] * 3, [(2, 1)] * 3],       # a block stored (no frame), frames 0 + 1, one frame per call
    "threes": [[(0, 3)] * 3, [(2, 3)] * 3, [(2, 3)] * 3],
    "fours": [[(0, 4)] * 3, [(2, 4)] * 3],
    "mixed": [[(0, 2), (1, 3), (0, 1)], [(2, 4), (2, 0), (1, 4)], [(2, 0), (2, 1), (2, 3)], [(2, 2), (2, 4), (2, 0)]],
}
KERNEL_SEED = 4100
KERNEL_FRAMES = 12             # frames per slot of the single-hop test: FRAME0, 10 x FRAME, END


def frames_of_packet(start, count):
    """(frames computed, f0) of packet_of(start, count) in stream_common.h"""
    nf = 0 if count == 0 else (count if count >= 2 else 0) if start == 0 else count + 1 if start == 1 else count
    return nf, start <= 1


def kernel_slot_rows(slot, n=64):
    """the synthetic row stream of slot `slot` of the kernel-level tests"""
    return synthetic_rows(KERNEL_SEED + slot, n, quiet=2 + slot)


def run_packet_case(calls, form):
    """-> per call, per slot: (frames [(re, im, mask)], f0, expected meter rows [n, 4]); and the slots' Meters at the end.  Each slot
    draws its frames in order from kernel_slot_rows(slot)"""
    _, lim, kind, tau = form
    meters = [Meter(lim=lim, tau=tau, kind=kind) for _ in range(S)]
    streams, at, out = [kernel_slot_rows(s) for s in range(S)], [0] * S, []
    for call in calls:
        per = []
        for s, (start, count) in enumerate(call):
            nf, f0 = frames_of_packet(start, count)
            frames = streams[s][at[s]:at[s] + nf]
            at[s] += nf
            want = [meters[s].step(*r, f0=(f0 and i == 0)) for i, r in enumerate(frames)]
            want = [w for w in want if w is not None]
            per.append((frames, f0, np.array(want, dtype=np.float64).reshape(len(want), 4)))
        out.append(per)
    return out, meters


# ---- the committed inputs of the server-level GPU tests -----------------------------------------------------------------------------
CONFIGS = {"small_g2": dict(ch=(1, 4, 8, 16, 32), rnn_groups=2), "g4": dict(rnn_groups=4)}
LENGTHS = (320, 480, 1600)
S = 3
CLIP_SEED = 340
# detector settings a server test runs a clip with: (name, set_vad kwargs, atten_lim dB or None, (post_filter, tau) or None)
SERVER_FORMS = [("default", {}, None, None), ("lim12", {}, 12.0, None), ("lim0", {}, 0.0, None), ("iam", {}, None, ("iam", 0.02)),
                ("vad_moved", dict(level_db=-38.0, threshold=0.5), None, None)]


# the mid-clip change of the server test: after SWITCH_AT blocks, set_vad(**SWITCH_VAD) and set_atten_lim(SWITCH_LIM_DB)
SWITCH_AT, SWITCH_VAD, SWITCH_LIM_DB = 5, dict(level_db=-45.0, threshold=0.4, attack=0.5, release=0.1), 6.0


def clip(L, i):
    from oracle import cruse_oracle as O
    return O.synth_pair(1, L, seed=CLIP_SEED + i)[0].view(-1)


def model64(name):
    """the float64 oracle model the GPU tests' models are made from (tests/test_gpu_streaming.py:models)"""
    from oracle import cruse_oracle as O
    m = O.unet_2(**CONFIGS[name])
    O.closed_form_init(m)
    SR.nontrivial_bn(m)
    return SR.as_double(m.eval())


def form_kwargs(form):
    """Meter(**kwargs) of a SERVER_FORMS entry"""
    _, vad, lim_db, pf = form
    kw = dict(vad)
    if lim_db is not None:
        kw["lim"] = 10.0 ** (-lim_db / 20.0)
    if pf is not None:
        kw["kind"], kw["tau"] = KINDS[pf[0]], pf[1]
    return kw
