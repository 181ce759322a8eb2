#!/usr/bin/env python3
"""Headline benchmark: spectrogram frames/s, CRUSE training step, on N MI355X of one node.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A step = STFT(noisy) + STFT(clean) -> unet_2 (4 enc/dec convs, 1 GRU group) forward -> mask*spectrum
-> WO-MALE -> backward -> gradient all-reduce (RCCL) -> Adam, on 64 clips x 4 s per GPU
(BASELINE.json configs[1]); inputs are synthetic, seeded and resident in HBM before the timed region.
Prints ONE JSON line on rank 0: metric, value (frames/s), unit, higher_is_better, dtype, ms_per_step (wall time of one timed
step) and the run's configuration.  A plain run does only that: set up, warm up, time --steps steps, print.
  --dump-outputs DIR  after the timed steps, run the timed path's step once more from the seeded start state on the last
                      timed step's inputs and write what it computed (loss, parameters after Adam, their gradients,
                      BatchNorm running statistics) as DIR/<name>.npy, to compare two builds output for output
  --full              also measure and check everything beyond the headline, in the same JSON line:
    roofline     -- the dominant kernel of the step, timed live with HIP events
    cpu_baseline -- the torch-CPU oracle (a port of the reference; oracle/) on the host's CPU cores
    parity_rel_l2, secondary rows (other precisions, configurations, batch sizes, trainer path), regressions
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: 8 TB/s spec
PEAK_MFMA_TFLOPS = {"bf16": 2500.0, "bf16x3": 2500.0 / 3.0, "f32": 157.3}


_T0 = time.perf_counter()


def log(msg):
    print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64, help="clips per GPU")
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--prec", default="bf16", choices=["bf16", "bf16x3", "f32"])
    ap.add_argument("--no-graph", action="store_true", help="launch the step's kernels eagerly (no HIP graph)")
    ap.add_argument("--graph", action="store_true", help="replay the step from HIP graph(s); default: time both forms during "
                                                          "warm-up and keep the faster")
    ap.add_argument("--full", action="store_true", help="besides the headline: CPU baseline, oracle parity, per-kernel timing and "
                                                        "rooflines, secondary rows and the regression check (the --no-* options "
                                                        "below drop single parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps: one step from the seeded start on the "
                                                                        "last timed step's inputs; its loss, parameters, gradients "
                                                                        "and BatchNorm running statistics to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the T=401 oracle parity figure (parity_rel_l2)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the f32 gate-mode, hop=320 STFT and upsample-decoder rows")
    ap.add_argument("--df", action="store_true", help="BASELINE config 4: DeepFilter(1,5) head + WO-MALE on its output")
    ap.add_argument("--bucketed", action="store_true", help="force the segmented (multi-GPU) schedule at world 1")
    ap.add_argument("--no-pin", action="store_true", help="multi-GPU runs: do NOT pin each rank's host threads to its GPU's NUMA-local cores "
                                                           "(cruse_amd/hostpin.py)")
    ap.add_argument("--ref-1gpu", type=float, default=None, help="frames/s of the 1-GPU run of the same configuration: adds "
                                                                 "scaling_efficiency = value / (n_gpus * ref) to the JSON line")
    return ap.parse_args()


def self_launch(a) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (the reference does it with mp.spawn,
    tools/train_stand.py:151-155) -- one process per GPU under torch.distributed.run on 127.0.0.1, rank r bound to device r.
    More ranks than devices are refused unless CRUSE_DIST_BACKEND=gloo (the single-GPU test rig: every rank on device 0)."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()
    backend = os.environ.get("CRUSE_DIST_BACKEND", "nccl")
    if a.gpus > ndev and backend != "gloo":
        raise SystemExit(f"bench.py --gpus {a.gpus}: this node has {ndev} HIP device(s) (RCCL needs one device per rank; "
                         f"CRUSE_DIST_BACKEND=gloo lets test rigs oversubscribe)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"--gpus {a.gpus} without a launcher: starting {a.gpus} ranks ({backend}) on 127.0.0.1:{port}")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # N ranks share the host: cap each rank's CPU thread pools (torch / OpenMP default to every core -- N x 128 threads spinning
    # beside N eager launch loops); the CPU-baseline leg sets its own count on rank 0
    env.setdefault("OMP_NUM_THREADS", str(max(1, min(8, (os.cpu_count() or 8) // max(a.gpus, 1)))))
    return subprocess.call(cmd, env=env)


# algorithmic work per frame of the training step (F = 160 geometry)
F_ALG_MFLOP = {1: 32.84, 4: 10.73}            # MFLOP / frame, training = 3 x forward
B_ALG_ELEMS = 16640                           # retained elements / frame; B_alg = 1280 + 2 * 16640 * s bytes


def parity_figure(model, groups: int, prec: str, B: int = 8, T: int = 401):
    """Enhanced-spectrum rel-L2 of THIS model (its weights, its precision mode) vs the CPU oracle at the bench's
    sequence length.  The oracle is the checker here, never the thing measured."""
    from cruse_amd import ops
    from cruse_amd.model.cruse_net import unet2_forward
    from oracle import cruse_oracle as O
    o = O.unet_2(rnn_groups=groups)
    o.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    o.train()
    noisy, _ = O.synth_pair(B, (T - 1) * 160, seed=11)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with torch.no_grad():
        _, est_o, _ = O.enhanced_spectrum(o, noisy)
    P = dict(model.named_parameters()); P = {k: v.data for k, v in P.items()}
    Bf = {k: v.clone() for k, v in model.named_buffers()}
    nre, nim, mag = ops.stft(noisy.cuda(), 320, 160, mag_bins=160, mag_eps=1e-8)
    mask, _ = unet2_forward(mag.view(B, 1, T, 160), P, Bf, model.ch, groups, prec, training=True, save=False,
                            update_running=False)
    er, ei = ops.mask_apply(mask.contiguous().view(B * T, 160), nre, nim, B * T, 160, 161)
    est = torch.stack([er.view(B, T, 161), ei.view(B, T, 161)], dim=-1).double().cpu()
    return float((est - est_o.double()).norm() / est_o.double().norm())


def profile_avg_ns(kernel_substr: str):
    """average in-graph duration of a kernel from the newest committed rocprofv3 kernel-stats CSV (profiles/)."""
    import csv, glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_kernel_stats_final.csv")))
    for f in reversed(files):                       # newest round first
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if kernel_substr in r["Name"]:
                    return float(r["AverageNs"]), os.path.basename(f)
    return None, None


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(groups: int, budget_s: float = 14.0):
    """the oracle (torch-CPU port of the reference path; the reference's own files do not import and do
    not travel) timed on this box's host cores -- one training step without optimizer (STFT x2 -> unet_2 -> mask -> WO-MALE ->
    backward), f32, 4 s clips, B in {1, 8}, 1 warm-up + >= 5 timed iterations (median) inside a time budget.
    Threads: BASELINE.md asks for os.cpu_count(); on the 256-core GPU host torch with 128+ threads is > 100x slower from
    oversubscription (8 threads 6.6 k, 16: 7.0-7.9 k, 32: 3.3 k frames/s at B = 8, measured in round 2), so the run uses
    min(os.cpu_count(), 16) -- the fastest setting found -- and says so; `cores` is the thread count actually used."""
    from oracle import cruse_oracle as O
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    model = O.unet_2(rnn_groups=groups)
    O.closed_form_init(model)
    model.train()
    L = 64000
    rows = {}
    for B, share in ((8, 0.7), (1, 0.3)):
        noisy, clean = O.synth_pair(B, L, seed=1)

        def one():
            model.zero_grad(set_to_none=True)
            loss, _ = O.train_step_loss(model, noisy, clean)
            loss.backward()
        one()                                                   # warm-up
        times, t_all = [], time.perf_counter()
        while len(times) < 5 or (time.perf_counter() - t_all < budget_s * share and len(times) < 20):
            t0 = time.perf_counter(); one(); times.append(time.perf_counter() - t0)
            if time.perf_counter() - t_all > 2.5 * budget_s * share:
                break
        med = sorted(times)[len(times) // 2]
        rows[B] = {"frames_per_s": round(B * 401 / med, 1), "ms_per_step_median": round(med * 1e3, 1), "iterations": len(times)}
    return {"value": rows[8]["frames_per_s"], "unit": "frames/s", "cores": cores, "kind": "port", "cpu_model": _cpu_model(),
            "host_cores": os.cpu_count(), "by_batch": {"B=8": rows[8], "B=1": rows[1]},
            "sample": f"fwd+WO-MALE+bwd (no optimizer) of the torch-CPU oracle, f32, 4 s clips, rnn_groups={groups}: B=8 "
                      f"{rows[8]['iterations']} it (value), B=1 {rows[1]['iterations']} it, median step; torch {torch.__version__}, "
                      f"{cores} threads of {os.cpu_count()} host cores ({_cpu_model()})"}


class KernelTimer:
    """Wraps cruse_amd.ops entry points with HIP events on torch's current stream (where the kernels run)."""

    NAMES = ["stft", "conv_gather", "conv_scatter2", "conv_gather_bnin", "conv_scatter2_bnin", "conv_wgrad", "channel_sum", "col_sum", "bn_stats", "bn_finalize",
             "bn_act_fwd", "bn_finalize_act_fwd", "bn_act_bwd", "ln_fwd", "ln_bwd", "gemm", "gemm_bf16_nt", "gemm_bf16x3_nt", "cast_bf16", "cast_bf16_padded",
             "ktile_bf16", "transpose_bf16", "gemm_bf16_nt_cat", "gemm_f16_nt", "ktile_f16",
             "gru_seq_fwd", "gru_seq_bwd", "gru_gate_grads", "gru_gate_grads_bf16", "mask_loss"]
    # entry points that launch the same kernel as another one are booked under that family
    FAMILY = {"gemm_bf16_nt_cat": "gemm_bf16_nt", "ktile_f16": "ktile_bf16"}

    def __init__(self, ops, eng):
        self.ops, self.rec, self.saved, self.eng = ops, [], {}, eng
        self.bytes, self.ncall = {}, {}                    # operand bytes of every call of a family (all passes) / its calls

    def bytes_per_launch(self):
        """ALGORITHMIC bytes of a launch, dtype-aware: the distinct tensors (>= 1 MB) a call takes and returns, each counted once --
        what a kernel that reads its inputs once and writes its outputs once must move (round 5: half the step's tensors are bf16 now,
        the fixed f32 figures of DESIGN section 4 overstated the achieved GB/s of the kernels that take them)."""
        return {n: self.bytes[n] / max(self.ncall.get(n, 1), 1) for n in self.bytes}

    def __enter__(self):
        # leaves run inline for this pass: an event pair around a launch only times that kernel when
        # nothing else shares the device with it
        self.side, self.side_was = self.eng.side, self.eng.side.enabled
        self.eng.side.enabled = False
        for n in self.NAMES:
            f = getattr(self.ops, n)
            self.saved[n] = f

            def wrap(*a, _f=f, _n=self.FAMILY.get(n, n), **k):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); out = _f(*a, **k); e1.record()
                self.rec.append((_n, e0, e1))
                self.bytes[_n] = self.bytes.get(_n, 0) + _operand_bytes((a, k, out))
                self.ncall[_n] = self.ncall.get(_n, 0) + 1
                return out
            setattr(self.ops, n, wrap)
        return self

    def __exit__(self, *exc):
        self.side.enabled = self.side_was
        for n, f in self.saved.items():
            setattr(self.ops, n, f)

    def mark_pass(self):
        self.rec.append(None)

    def summary(self):
        """Per-family ms and launch count of ONE pass: each launch's time is its MINIMUM over the passes (an event pair
        also brackets the wrapper's host work -- output allocation, first-use attribute calls -- so a slow host moment
        would otherwise be booked as kernel time)."""
        torch.cuda.synchronize()
        passes, cur = [], []
        for r in self.rec:
            if r is None:
                passes.append(cur); cur = []
            else:
                cur.append((r[0], r[1].elapsed_time(r[2])))
        if cur:
            passes.append(cur)
        passes = [p for p in passes if len(p) == len(passes[0])]
        tot, cnt = {}, {}
        for i, (n, _) in enumerate(passes[0]):
            tot[n] = tot.get(n, 0.0) + min(p[i][1] for p in passes)
            cnt[n] = cnt.get(n, 0) + 1
        return tot, cnt


def _operand_bytes(obj, seen=None, depth=0) -> int:
    """bytes of the distinct large tensors reachable from a call's arguments / results (lists, tuples, dicts, plain objects)"""
    seen = set() if seen is None else seen
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda and obj.numel() * obj.element_size() >= (1 << 20) and obj.data_ptr() not in seen:
            seen.add(obj.data_ptr())
            return obj.numel() * obj.element_size()
        return 0
    if depth > 3 or obj is None or isinstance(obj, (int, float, str, bool)):
        return 0
    if isinstance(obj, dict):
        return sum(_operand_bytes(v, seen, depth + 1) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(_operand_bytes(v, seen, depth + 1) for v in obj)
    if hasattr(obj, "__dict__"):
        return sum(_operand_bytes(v, seen, depth + 1) for v in vars(obj).values())
    return 0


def _newest_profile(suffix: str) -> str:
    """profiles/rNN_<suffix> of the latest round that committed one (the PMC passes are separate rocprofv3 runs, tools/profile_round.sh)"""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    for r in range(9, 0, -1):
        if os.path.exists(os.path.join(d, f"r{r:02d}_{suffix}")):
            return os.path.join(d, f"r{r:02d}_{suffix}")
    return os.path.join(d, f"r01_{suffix}")


PMC_FILE = _newest_profile("pmc_hbm_traffic.csv")
PMC_MFMA_FILE = _newest_profile("pmc_mfma_util.csv")


PMC_STEPS = 4            # the PMC passes ran `bench.py --steps 3 --warmup 1`: launch counts in the CSV are per 4 steps


def pmc_traffic():
    """HBM bytes per launch and kernel family from the committed rocprofv3 PMC passes (profiles/r01_pmc_hbm_traffic.csv:
    separate FETCH_SIZE / WRITE_SIZE runs of this script at the bench shape, gfx950 correction applied as
    MI355X_MICROARCH.md prescribes).  bench.py cannot run the PMC passes itself; the figures are valid for the
    default workload only."""
    out = {}
    if not os.path.exists(PMC_FILE):
        return out
    import csv
    import re
    acc = {}
    steps = float(PMC_STEPS)
    with open(PMC_FILE) as f:
        lines = f.readlines()
    for l in lines:                              # "# ... launches = over the N steps of the run" (tools/pmc_traffic.py)
        m = re.search(r"over the (\d+) steps", l) if l.startswith("#") else None
        if m:
            steps = float(m.group(1))
    if True:
        rows = csv.DictReader(l for l in lines if not l.startswith("#"))
        for r in rows:
            n, b = int(r["launches"]), float(r["hbm_bytes_per_launch_corrected"])
            a = acc.setdefault(r["bench_family"], [0, 0.0])
            a[0] += n; a[1] += n * b
    for fam, (n, tot) in acc.items():
        out[fam] = tot / max(n, 1)
    out["__step_total__"] = sum(tot for _, tot in acc.values()) / steps
    out["conv_gather"] = out["conv_scatter2"] = out.get("conv", 0.0) or None
    return out


def pmc_mfma_util():
    """MFMA utilisation per kernel family from the committed rocprofv3 PMC pass (profiles/r03_pmc_mfma_util.csv, made by
    tools/pmc_traffic.py --mfma at the bench shape): sum(SQ_VALU_MFMA_BUSY_CYCLES) / sum(GRBM_GUI_ACTIVE / 8 XCDs * 256 CUs * 4)."""
    path = PMC_MFMA_FILE
    out = {}
    if not os.path.exists(path):
        return out
    import csv
    acc = {}
    with open(path) as f:
        for r in csv.DictReader(l for l in f if not l.startswith("#")):
            a = acc.setdefault(r["bench_family"], [0.0, 0.0])
            n = int(r["launches"])
            a[0] += n * float(r["mfma_busy_cycles_per_launch"]); a[1] += n * float(r["gui_active_cycles_per_launch"]) * 256 * 4
    for fam, (busy, cap) in acc.items():
        out[fam] = round(busy / cap, 4) if cap else 0.0
    out["conv_gather"] = out["conv_scatter2"] = out.get("conv")
    out["gemm_bf16x3_nt"] = out["gemm_f16_nt"] = out.get("gemm_bf16_nt")
    return out


def kernel_rooflines(B, T, H, G, prec, per_step_ms, calls, op_bytes=None):
    """Algorithmic work per launch for the kernels that can dominate."""
    Hg = H // G
    rows = B * T
    out = {}
    rec_flops = 2.0 * rows * 3 * Hg * Hg * G               # W_hh h_{t-1} over all steps, one launch
    for name in ("gru_seq_fwd", "gru_seq_bwd"):
        if name in per_step_ms:
            avg_ms = per_step_ms[name] / calls[name]
            ach = rec_flops / (avg_ms * 1e-3) / 1e12
            out[name] = {"bound": "mfma", "achieved": round(ach, 3), "peak": PEAK_MFMA_TFLOPS[prec], "unit": "TFLOP/s",
                         "frac": round(ach / PEAK_MFMA_TFLOPS[prec], 5), "traffic": None,
                         "avg_launch_ms": round(avg_ms, 4),
                         "note": f"latency-bound by design: {T} dependent steps per launch, "
                                 f"{avg_ms * 1e3 / T:.2f} us per step"}
    # ALGORITHMIC flops: 2 layers x (gi, dX, dW_ih, dW_hh) = 8 products of 2 * rows * 3 Hg * Hg * G flops.  The forward projections run in their
    # own families -- split-bf16 x3 (its extra MFMA passes are not counted) and / or the single f16 pass: one launch per group and layer, so
    # launches / G = products --, the rest is gemm_bf16_nt's (the
    # concatenated weight-gradient launch and the transposed-A dX are booked there).
    fwd_prod = {f: calls[f] / float(G) for f in ("gemm_bf16x3_nt", "gemm_f16_nt") if f in per_step_ms}
    for gname in ("gemm", "gemm_bf16_nt", "gemm_bf16x3_nt", "gemm_f16_nt"):
        if gname in per_step_ms:
            if gname in fwd_prod:
                nprod = fwd_prod[gname]
            else:
                nprod = 8 - sum(fwd_prod.values())
            flops = 2.0 * rows * 3 * Hg * Hg * G * nprod
            avg_ms = per_step_ms[gname] / calls[gname]
            ach = flops / (per_step_ms[gname] * 1e-3) / 1e12
            out[gname] = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_MFMA_TFLOPS[prec], "unit": "TFLOP/s",
                          "frac": round(ach / PEAK_MFMA_TFLOPS[prec], 4), "traffic": None,
                          "avg_launch_ms": round(avg_ms, 4)}
    hbm = {"conv_gather": 2 * 640 * 4.0, "conv_scatter2": 2 * 640 * 4.0, "conv_gather_bnin": 2 * 640 * 4.0, "conv_scatter2_bnin": 3 * 640 * 4.0, "bn_act_fwd": 2 * 640 * 4.0, "bn_finalize_act_fwd": 2 * 640 * 4.0,
           "bn_act_bwd": 5 * 640 * 4.0, "conv_wgrad": 2 * 640 * 4.0, "ln_fwd": 2 * 640 * 4.0, "ln_bwd": 3 * 640 * 4.0}
    for name, bpf in hbm.items():
        if name in per_step_ms:
            avg_ms = per_step_ms[name] / calls[name]
            nbytes, src = bpf * rows, "f32 tensors of DESIGN section 4"
            if op_bytes and op_bytes.get(name):
                nbytes, src = op_bytes[name], "distinct tensor operands of the calls, as stored (f32 / bf16 / f16)"
            ach = nbytes / (avg_ms * 1e-3) / 1e9
            out[name] = {"bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": None, "avg_launch_ms": round(avg_ms, 4),
                         "algorithmic_bytes_per_launch": int(nbytes), "algorithmic_bytes_source": src}
    return out


def step_roofline(fps: float, groups: int, prec: str, B: int, T: int):
    """BASELINE.md section 4 / SURVEY 8(d): whole-step achieved fraction, both terms."""
    f_alg = F_ALG_MFLOP.get(groups)
    out = {}
    if f_alg:
        tf = fps * f_alg * 1e6 / 1e12
        out["mfma"] = {"achieved": round(tf, 2), "peak": PEAK_MFMA_TFLOPS[prec], "unit": "TFLOP/s",
                       "frac": round(tf / PEAK_MFMA_TFLOPS[prec], 5), "F_alg_MFLOP_per_frame": f_alg}
    for name, sz in (("hbm_f32_storage", 4), ("hbm_bf16_storage", 2)):
        b_alg = 1280 + 2 * B_ALG_ELEMS * sz
        gbs = fps * b_alg / 1e9
        out[name] = {"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 5),
                     "B_alg_bytes_per_frame": b_alg}
    out["achieved"] = max(v["frac"] for v in out.values())
    pmc = pmc_traffic()
    if pmc.get("__step_total__") and (B, T, groups, prec) == (64, 401, 1, "bf16"):
        tot = pmc["__step_total__"]
        b_alg = (1280 + 2 * B_ALG_ELEMS * 4) * B * T
        out["pmc_hbm_bytes_per_step"] = round(tot)
        out["pmc_vs_B_alg_f32"] = round(tot / b_alg, 2)
        out["pmc_source"] = "profiles/" + os.path.basename(PMC_FILE)
    return out


def secondary_rows(a, dev, pool):
    """Not the headline: (1) the same step in the parity-GATE mode (exact-f32 MFMA), (2) the literal reading of
    BASELINE.json's "20ms-hop": a forward STFT at hop = 320 (T = 201; hop = win violates NOLA, so no iSTFT / training
    step exists for it -- SURVEY 8d)."""
    from cruse_amd import ops
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse_net import unet_2
    out = {}
    try:
        torch.manual_seed(0)
        m = unet_2(rnn_groups=a.groups, precision="f32").to(dev)
        e = TrainEngine(m, lr=1e-3, use_graph=not a.no_graph)
        n = 8
        forms = {}
        # both launch forms, as for the headline (graph replay / eager launches): the faster one is this mode's figure
        for form in ([False] if a.no_graph else [True, False]):
            e.use_graph = form
            for s in range(3):
                e.step(*pool[s % len(pool)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(n):
                e.step(*pool[s % len(pool)])
            torch.cuda.synchronize()
            forms["graph" if form else "eager"] = (time.perf_counter() - t0) / n
        kept = min(forms, key=forms.get)
        dt = forms[kept]
        B, L = pool[0][0].shape
        out["f32_gate_mode"] = {"value": round(B * (1 + L // 160) / dt, 1), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3),
                                "steps": n, "dtype": "f32", "launch_form": kept,
                                "ms_per_step_by_form": {k: round(v * 1e3, 3) for k, v in forms.items()},
                                "note": "same step, v_mfma_f32_16x16x4_f32 everywhere (parity <= 1e-6)"}
        del e, m
    except Exception as ex:                                  # secondary rows never break the headline line
        out["f32_gate_mode"] = {"error": repr(ex)[:200]}
    skip = os.environ.get("CRUSE_BENCH_SKIP", "").split(",")
    # (1b) the headline's bf16 mode with GGRU layer 1's gate projection on f16 x against two f16 planes of W_ih as well (EngineConfig.gi_f16 = 3;
    #      cruse_gemm_f16x2_nt): the same two passes as the default's bf16 x . W hi / lo, 11 instead of 8 bits on x.  Not the default: one vector of
    #      the closed-form fixture G16 leaves its gradient-norm tolerance by 0.006
    try:
        if "layer1_f16x2_mode" in skip:
            raise RuntimeError("skipped")
        from cruse_amd import config as _cfg
        torch.manual_seed(0)
        m = unet_2(rnn_groups=a.groups, precision="bf16").to(dev)
        cfg = _cfg.EngineConfig(gi_f16=3)
        n = 20
        forms = {}
        # both launch forms, the faster is the figure (as the headline and the config rows: host threads of the CPU legs may still be winding down)
        for form in ([False] if a.no_graph else [True, False]):
            e = TrainEngine(m, lr=1e-3, use_graph=form, config=cfg)
            forms["graph" if form else "eager"] = _time_steps(e, pool, n_warm=4, n=n) * 1e-3
        kept = min(forms, key=forms.get)
        dt = forms[kept]
        B, L = pool[0][0].shape
        row = {"value": round(B * (1 + L // 160) / dt, 1), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "steps": n, "dtype": "bf16",
               "launch_form": kept, "ms_per_step_by_form": {k: round(v * 1e3, 3) for k, v in forms.items()}, "timeouts": ops.gru_status(),
               "note": "the headline step with EngineConfig.gi_f16 = 3: layer-1 gate projection as f16 x . (W_ih hi + lo)^T (cruse_gemm_f16x2_nt)"}
        if not a.no_parity:
            torch.manual_seed(0)
            m2 = unet_2(rnn_groups=a.groups, precision="bf16").to(dev)          # (fresh weights, as the headline's parity figure)
            with _cfg.use(cfg):
                row["parity_rel_l2"] = float(f"{parity_figure(m2, a.groups, 'bf16'):.4g}")
            row["parity_note"] = "enhanced-spectrum rel-L2 vs the CPU oracle at T=401, B=8 (bar 1e-3; the default mode: parity_rel_l2 of the main line)"
        out["layer1_f16x2_mode"] = row
        del e, m
    except Exception as ex:
        out["layer1_f16x2_mode"] = {"error": repr(ex)[:200]}
    try:
        x = pool[0][0]
        B, L = x.shape
        ops.stft(x, 320, 320, mag_bins=160, mag_eps=1e-8); torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.stft(x, 320, 320, mag_bins=160, mag_eps=1e-8)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        T2 = 1 + L // 320
        byts = B * (L * 4 + T2 * (161 * 8 + 160 * 4))
        out["stft_hop320_forward"] = {"value": round(B * T2 / (ms * 1e-3), 1), "unit": "frames/s", "frames_per_clip": T2,
                                      "ms": round(ms, 4), "hbm_GBs": round(byts / (ms * 1e-3) / 1e9, 1),
                                      "note": "forward STFT only, hop = win = 320 (20 ms hop)"}
    except Exception as ex:
        out["stft_hop320_forward"] = {"error": repr(ex)[:200]}
    # (3) the nearest-upsample decoder variant (model/cruse.py:14 CRUSE4MagAddSkipUpsample): forward + MSE + backward
    #     through the nn.Module / autograd surface -- the frame-major engine of unet_2 with dec_mode="upsample" behind one autograd
    #     node; no optimizer: the cost of the variant's model, not a training-step figure
    try:
        from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
        torch.manual_seed(0)
        B, L = pool[0][0].shape
        Bu, T = min(B, 64), 1 + L // 160
        mu = CRUSE4MagAddSkipUpsample(rnn_groups=a.groups, precision="bf16").to(dev).train()
        xin = torch.rand(Bu, 1, T, 160, device=dev) + 0.05
        tgt = torch.rand(Bu, 1, T, 160, device=dev)

        def it():
            for q in mu.parameters():
                q.grad = None
            ((mu(xin) - tgt) ** 2).mean().backward()
        it(); torch.cuda.synchronize()
        n = 10
        t0 = time.perf_counter()
        for _ in range(n):
            it()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        out["upsample_decoder_variant"] = {"value": round(Bu * T / dt, 1), "unit": "frames/s", "ms_per_step": round(dt * 1e3, 3), "batch": Bu,
                                           "steps": n, "dtype": "bf16",
                                           "note": "CRUSE4MagAddSkipUpsample forward + MSE + backward (one autograd node over the frame-major "
                                                   "MFMA convs / persistent GRU kernels, nearest upsample materialised once per level; no optimizer)"}
        del mu
    except Exception as ex:
        out["upsample_decoder_variant"] = {"error": repr(ex)[:200]}
    return out


def trainer_path_rows(a, dev, headline_fps):
    """epoch throughput of the TRAINER -- train.trainer_casual.Trainer._train_epoch as tools/train_stand.py's entry()
    drives it (torch DataLoader built from the [train_dataset] section, DistributedSampler, Adam, wo_male_loss, clip 10) -- for
      device: the device-resident dataset plug-in (cruse_amd.data.DevicePairs: pools in HBM, gather + on-GPU snr_mix per batch),
      host:   a host dataset behind the reference's DataLoader (cruse_amd.data.HostPoolPairs, 4 workers; samples stored as f16 / f32) through
              the trainer's pinned prefetcher on its own copy stream (PCIe-inclusive: 16.4 / 32.8 MB per step) -- bounded by the consumer
              side of torch's DataLoader, which hands a [64, 64000] f32 pair over every ~5-9 ms on the bench host whatever the worker count;
    frames/s of the SECOND epoch (the first holds graph capture / the launch-form tuner) and the ratio to the headline line."""
    from torch.utils.data import DataLoader, DistributedSampler
    import train_base.loss as L
    from cruse_amd.data import DevicePairs, HostPoolPairs
    from cruse_amd.model.cruse_net import unet_2
    from cruse_amd.train.trainer_casual import Trainer
    B, Ls = a.batch, int(a.seconds * 16000)
    nb = 120
    out = {}
    for name, ds, kw in (("device_dataset", DevicePairs(num=nb * B, length=Ls, seed=1, pool=128), dict(num_workers=0)),
                         ("host_dataset_f16_prefetched", HostPoolPairs(num=nb * B, length=Ls, seed=1, pool=128, dtype="float16"),
                          dict(num_workers=4, persistent_workers=True, prefetch_factor=2)),
                         ("host_dataset_f32_prefetched", HostPoolPairs(num=nb * B, length=Ls, seed=1, pool=128),
                          dict(num_workers=4, persistent_workers=True, prefetch_factor=2))):
        try:
            torch.manual_seed(0)
            m = unet_2(rnn_groups=a.groups)
            cfg = {"acoustics": {"n_fft": 320, "hop_length": 160}, "trainer": {"train": {"epochs": 3, "clip_grad_norm_value": 10.0}},
                   "meta": {"save_dir": "/tmp/cruse_bench_trainer", "precision": a.prec, "hip_graph": "auto"}}
            sampler = DistributedSampler(dataset=ds, num_replicas=1, rank=0, shuffle=True)
            loader = DataLoader(dataset=ds, sampler=sampler, shuffle=False, batch_size=B, drop_last=True, **kw)
            tr = Trainer(dist=None, rank=0, config=cfg, resume=False, only_validation=False, model=m, loss_function=L.wo_male_loss(),
                         optimizer=torch.optim.Adam(m.parameters(), lr=1e-3), train_dataloader=loader, validation_dataloader=None)
            import contextlib, io
            fps = []
            with contextlib.redirect_stdout(io.StringIO()):
                for ep in (1, 2, 3):
                    tr._train_epoch(ep)
                    fps.append(tr.last_epoch_frames_per_s)
            best = max(fps[1:])
            out[name] = {"value": round(best, 1), "unit": "frames/s", "epochs_frames_per_s": [round(f, 1) for f in fps],
                         "batches_per_epoch": nb, "ratio_to_headline": round(best / headline_fps, 4),
                         "launch_form": getattr(tr.engine, "launch_form_timing", None)}
            del tr, loader
        except Exception as ex:
            out[name] = {"error": repr(ex)[:300]}
    out["note"] = ("Trainer._train_epoch (tools/train_stand.py flow: DataLoader + DistributedSampler + Adam + wo_male_loss + clip) on 120 batches "
                   "of the headline shape; epoch 1 holds capture / tuning, the better of epochs 2-3 is the figure; host row = PCIe-inclusive")
    return out


def rccl_world1_row(a, dev, pool):
    """what the multi-GPU SCHEDULE costs before a byte crosses xGMI -- the headline step on backend nccl (= RCCL) at
    world size 1 with the collectives forced (CRUSE_FORCE_COLLECTIVES=1): three gradient buckets all-reduced asynchronously between
    three graph segments (or from the launcher stream when launched eagerly), the health words MAX-reduced, 1 / world folded into Adam
    -- beside the same engine without a process group.  Runs LAST (it initialises a process group in this process)."""
    import socket
    from cruse_amd.config import EngineConfig
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse_net import unet_2
    out = {}
    try:
        torch.manual_seed(0)
        cfg = EngineConfig.from_env()

        def run(bucketed):
            m = unet_2(rnn_groups=a.groups, precision=a.prec).to(dev)
            e = TrainEngine(m, lr=1e-3, use_graph=True, bucketed=bucketed, config=cfg)
            forms = {}
            for form in (True, False):
                e.use_graph = form
                forms["graph" if form else "eager"] = _time_steps(e, pool, n_warm=4, n=10)
            return forms, e
        single, _ = run(False)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        os.environ["CRUSE_FORCE_COLLECTIVES"] = "1"
        dist.init_process_group("nccl", rank=0, world_size=1)
        try:
            bucketed, eng = run(True)
            ids = torch.tensor([0], device=dev, dtype=torch.int64)
            got = [torch.zeros_like(ids)]
            dist.all_gather(got, ids)
            seen = len({int(g_.item()) for g_ in got})
            nb = [4 * (e_ - s_) for s_, e_ in eng.flat.bucket_range]
        finally:
            dist.destroy_process_group()
            os.environ.pop("CRUSE_FORCE_COLLECTIVES", None)
        best_s, best_b = min(single.values()), min(bucketed.values())
        out = {"ms_per_step": round(best_b, 3), "ms_per_step_by_form": {k: round(v, 3) for k, v in bucketed.items()},
               "single_segment_ms_per_step": round(best_s, 3), "single_segment_by_form": {k: round(v, 3) for k, v in single.items()},
               "bucketed_over_single": round(best_b / best_s, 4), "backend": "rccl", "rccl_ranks_seen": seen, "world_size": 1,
               "bucket_bytes": nb,
               "note": "headline step with forced collectives on backend nccl at world 1: 3 gradient buckets all-reduced asynchronously "
                       "between 3 graph segments / from the launcher stream + MAX-reduced health words, against the same engine with no "
                       "process group (one segment); the gap bounds what the schedule itself costs at N > 1 before any xGMI traffic"}
    except Exception as ex:
        out = {"error": repr(ex)[:300]}
    return out


HOST_ISSUE_MS = {}           # id(engine) -> host time to ISSUE one step of the last _time_steps() call (no synchronisation inside)


def host_contention_row(a, dev, pool, nsib=7, steps=30):
    """what seven sibling ranks do to THIS rank's launch loop, without the node -- the headline step (eager launches and
    graph replay) alone, beside seven processes spinning the host side of a launch loop (ctypes calls into the library that are rejected
    before any device work: tools/host_contention_probe.py) unpinned, and with every process on the core slice cruse_amd/hostpin.py gives
    rank r of 8 (this process = rank 0).  The figure that matters at N = 8 is pinned / alone."""
    import multiprocessing as mp
    from cruse_amd import hostpin
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse_net import unet_2
    from tools.host_contention_probe import sibling
    torch.manual_seed(0)
    m = unet_2(rnn_groups=a.groups, precision=a.prec).to(dev)
    engs = {"graph": TrainEngine(m, lr=1e-3, use_graph=True), "eager": TrainEngine(m, lr=1e-3, use_graph=False)}

    def measure():
        return {k: round(_time_steps(e, pool, n_warm=4, n=steps), 3) for k, e in engs.items()}
    out = {"alone": measure(), "siblings": nsib, "host_cores": os.cpu_count()}
    allowed = sorted(os.sched_getaffinity(0))
    ctx = mp.get_context("spawn")
    try:
        for label, pinned in (("unpinned", False), ("pinned", True)):
            stop = ctx.Event()
            procs = [ctx.Process(target=sibling, args=(stop, i), daemon=True) for i in range(nsib)]
            for p in procs:
                p.start()
            try:
                if pinned:
                    none = {r: None for r in range(nsib + 1)}
                    for i, p in enumerate(procs):
                        os.sched_setaffinity(p.pid, hostpin.plan(i + 1, nsib + 1, allowed, none))
                    mine = hostpin.plan(0, nsib + 1, allowed, none)
                    os.sched_setaffinity(0, mine)
                    out["cores_per_rank"] = len(mine)
                time.sleep(1.5)                                 # (the siblings' interpreters are up and spinning)
                out[label] = measure()
            finally:
                stop.set()
                for p in procs:
                    p.join(timeout=10)
                    if p.is_alive():
                        p.terminate()
    finally:
        os.sched_setaffinity(0, allowed)
    for label in ("unpinned", "pinned"):
        if label in out:
            out[label + "_over_alone"] = {k: round(out[label][k] / out["alone"][k], 4) for k in out["alone"]}
    out["note"] = ("headline step beside seven host-side launch loops: ms per step by launch form; pinned = every process on its own "
                   "1/8 slice of the allowed cores (cruse_amd/hostpin.py: what bench.py / tools/train_stand.py do per rank at N > 1)")
    return out


def _time_steps(eng, pool, n_warm=3, n=8):
    """device ms per step (HIP events around n steps); the host's issue time per step of the same loop is left in HOST_ISSUE_MS:
    a form whose issue time is about its device time is HOST-bound (an eager B = 32 step issues ~400 launches in ~3 ms)"""
    for s_ in range(n_warm):
        eng.step(*pool[s_ % len(pool)])
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for s_ in range(n):
        eng.step(*pool[s_ % len(pool)])
    t_issue = time.perf_counter() - t0
    e1.record(); torch.cuda.synchronize()
    HOST_ISSUE_MS[id(eng)] = t_issue / n * 1e3
    return e0.elapsed_time(e1) / n


def config_rows(a, dev, pool):
    """BASELINE.json configs 3, 4 and 5 as driver-visible rows: the per-GPU share of each on ONE device --
    config 3: g = 4, 64 clips (512 / 8 GPUs); config 4: g = 4 + DeepFilter(1,5) head, 32 clips (256 / 8); config 5: the blocks
    model/mtfaa.py defines (STFT -> PhaseEncoder -> 6 x TFCM_Block) in fp16 storage, 8 clips.  Each: ms per step (the faster of
    HIP-graph replay and eager launches, as the headline does), frames/s, the dominant kernel family with its roofline
    fraction from an instrumented pass, and the enhanced-spectrum (config 5: stack output) rel-L2 against the CPU oracle."""
    from cruse_amd import ops
    from cruse_amd.data import synth_batch
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse_net import unet_2
    out = {}
    L = pool[0][0].shape[1]
    T = 1 + L // 160

    def unet_row(name, groups, B, df, note, parity=True, into=None):
        into = out if into is None else into
        torch.manual_seed(0)
        m = unet_2(rnn_groups=groups, precision="bf16").to(dev)
        bp = [synth_batch(B, L, dev, 7000 + i) for i in range(2)]
        best, forms = None, {}
        for graph in (True, False):
            e = TrainEngine(m, lr=1e-3, use_graph=graph, loss="wo_male_df" if df else "wo_male")
            ms = _time_steps(e, bp)
            forms["graph" if graph else "eager"] = {"ms": round(ms, 3), "host_issue_ms": round(HOST_ISSUE_MS[id(e)], 3)}
            if best is None or ms < best[0]:
                best = (ms, graph, e)
        ms, graph, e = best
        with KernelTimer(ops, e) as kt:
            e._fwd_bwd(*bp[0]); torch.cuda.synchronize(); kt.rec.clear()
            for s_ in range(2):
                e._fwd_bwd(*bp[s_ % 2]); kt.mark_pass()
            per_step, calls = kt.summary()
        rl = kernel_rooflines(B, T, m.hidden_size, groups, "bf16", per_step, calls, kt.bytes_per_launch())
        dom = max(per_step, key=per_step.get)
        roof = dict(rl.get(dom, {"bound": "hbm", "achieved": None, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": None}))
        roof["kernel"] = dom; roof["ms_per_step_all_launches"] = round(per_step[dom], 3)
        fps = B * T / (ms * 1e-3)
        sr = step_roofline(fps, groups, "bf16", B, T)
        kms = {k: round(v, 3) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])[:8]}
        row = {"kernel_ms_per_step_top8": kms, "value": round(fps, 1), "unit": "frames/s", "ms_per_step": round(ms, 3), "per_gpu_batch": B, "groups": groups,
               "launch_form": "graph" if graph else "eager", "by_form": forms, "dtype": "bf16", "roofline": roof,
               "roofline_step_hbm_f32_storage_frac": sr["hbm_f32_storage"]["frac"], "roofline_step_mfma_frac": sr.get("mfma", {}).get("frac"),
               "timeouts": ops.gru_status(), "note": note}
        row["gru_plan"] = {"fwd": ops.gru_plan(B, groups, m.hidden_size // groups, "bf16", True),
                           "bwd": ops.gru_plan(B, groups, m.hidden_size // groups, "bf16", False)}
        if parity and not a.no_parity:
            if df:
                from oracle import cruse_oracle as O
                from oracle import cruse_oracle_ext as X
                o = O.unet_2(rnn_groups=groups)
                o.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
                o.train()
                noisy, clean = O.synth_pair(2, (T - 1) * 160, seed=12)
                torch.set_num_threads(min(os.cpu_count() or 1, 16))
                with torch.no_grad():
                    _, aux = X.train_step_loss_df(o, noisy, clean)
                e2 = TrainEngine(m, lr=0.0, use_graph=False, loss="wo_male_df")
                e2._fwd_bwd(noisy.to(dev), clean.to(dev)); torch.cuda.synchronize()
                est = e2._last_est.permute(1, 0, 2, 3).double().cpu()                 # [2,B,T,F] -> [B,2,T,F]
                row["parity_rel_l2"] = float(f"{float((est - aux['est'].double()).norm() / aux['est'].double().norm()):.4g}")
                row["parity_note"] = "DeepFilter output (enhanced spectrum) vs oracle_ext.train_step_loss_df at T=401, B=2"
            else:
                row["parity_rel_l2"] = float(f"{parity_figure(m, groups, 'bf16', B=2, T=T):.4g}")
                row["parity_note"] = "enhanced-spectrum rel-L2 vs the CPU oracle at T=401, B=2 (bar 1e-3)"
        into[name] = row
        del e, best

    for name, args in (("config3_g4", (4, 64, False, "BASELINE config 3 per-GPU share: 4 grouped GRUs of 160, 64 of the 512 clips")),
                       ("config4_df_g4_b32", (4, 32, True, "BASELINE config 4 per-GPU share: + DeepFilter(1,5) head, 32 of the 256 clips"))):
        try:
            unet_row(name, *args)
        except Exception as ex:                              # secondary rows never break the headline line
            out[name] = {"error": repr(ex)[:300]}
    # ---- batch sweep ("B per GPU should be as large as memory allows ... stated next to the roofline fraction"):
    #      the headline model at 128 and 256 clips per GPU.  Above 96 clips make_plan takes the 16-clip-chain kernels (gru_w16.hip);
    #      tests/test_gpu_parity_bench_shape.py::test_wide_chain_plan_at_b128_vs_oracle checks that plan against the oracle
    sweep = {}
    for Bs in (128, 256):
        try:
            unet_row(f"B={Bs}", a.groups, Bs, False, f"the headline model and step at {Bs} clips x 4 s per GPU", parity=False, into=sweep)
        except Exception as ex:
            sweep[f"B={Bs}"] = {"error": repr(ex)[:300]}
        torch.cuda.empty_cache()
    out["batch_sweep"] = sweep
    # ---- config 5: tools/mtfaa_stress.py's step (fp16 storage) ---------------------------------------------------------
    # The row runs on a stream of its own: autograd's AccumulateGrad nodes remember the stream of the first backward pass, and a capture
    # that has to synchronise with the legacy DEFAULT stream through them crashes in hipStreamEndCapture (rounds 2-5 ran this row on the
    # bench's high-priority stream and never saw it)
    _prev5 = torch.cuda.current_stream()
    _s5 = torch.cuda.Stream()
    _s5.wait_stream(_prev5)
    torch.cuda.set_stream(_s5)
    try:
        from model import mtfaa as M
        from cruse_amd.nn_generic import to_f16, to_f32
        torch.manual_seed(0)
        Bm = 8
        stft = M.STFT(320, 160, 320, "hann")
        pe = M.PhaseEncoder(4, 1).to(dev)
        tfcm = M.TFCM(24, (3, 3), 6).to(dev)
        x = (0.1 * torch.randn(Bm, L)).to(dev)
        params = [q for mod in (pe, tfcm) for q in mod.parameters()]

        def step():
            c = stft.transform(x)
            h = torch.cat([pe([c])] * 12, dim=1)             # [B,24,161,T] (channel plumbing, as tools/mtfaa_stress.py)
            y = to_f32(tfcm(to_f16(h)))
            for q in params:
                q.grad = None
            (y.square().mean() * 65536.0).backward()         # (the usual loss scale of fp16 training)
            return y
        step(); step(); torch.cuda.synchronize()

        def timed(fn, n=8):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n
        ms_eager = timed(step, 4)
        y = step()
        # the same step replayed as ONE HIP graph (284 launches per step: eager issue is host-bound, ~0.8 ms over the kernels' sum);
        # like the headline row, the faster form is the one reported
        ms_graph, launch_form = None, "eager"
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                yg = step()
            gr.replay(); torch.cuda.synchronize()
            ms_graph = timed(gr.replay)
            for _ in range(2):                                # (the graph's own branch streams may share the launching stream's hardware
                with torch.cuda.stream(torch.cuda.Stream()):  #  queue -- cruse_amd/streams.py: the fastest of three launchers is the figure)
                    ms_graph = min(ms_graph, timed(gr.replay))
            if not bool(torch.isfinite(yg).all()) or float((yg - y).abs().max()) > 1e-2 * float(y.abs().max()):
                ms_graph = None                               # (a replay that does not reproduce the eager step is not reported)
        except Exception as ex:                               # capture is an optimisation of the issue path only
            log(f"config 5: graph capture not used ({repr(ex)[:120]})")
            torch.cuda.synchronize()
        ms = ms_eager
        if ms_graph is not None and ms_graph < ms_eager:
            ms, launch_form = ms_graph, "graph"
        tensor = Bm * 24 * 161 * T * 2                       # one [B,24,161,T] f16 tensor
        # per block forward: conv, BN+PReLU, depthwise, BN+PReLU, conv + add = 5 kernels reading and writing one tensor each,
        # + 2 statistics passes; backward ~2.5 x: ~3.5 x (5*2 + 2) tensors per block (the figure tools/mtfaa_stress.py prints)
        alg_bytes = 6 * (5 * 2 + 2) * tensor * 3.5
        row = {"value": round(Bm * T / (ms * 1e-3), 1), "unit": "frames/s", "ms_per_step": round(ms, 3), "batch": Bm, "dtype": "f16 storage",
               "finite": bool(torch.isfinite(y).all()), "launch_form": launch_form,
               "launch_form_timing": {"eager_ms": round(ms_eager, 3), "graph_ms": round(ms_graph, 3) if ms_graph is not None else None},
               "roofline": {"bound": "hbm", "achieved": round(alg_bytes / (ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": round(alg_bytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4), "kernel": "whole TFCM stack (NCHW f16 streams)",
                            "algorithmic_bytes_per_step": int(alg_bytes)},
               "note": "BASELINE config 5: STFT -> PhaseEncoder -> 6 x TFCM_Block forward + backward (autograd over the NCHW f16 kernels: "
                       "pointwise convs on v_mfma_f32_16x16x32_f16, depthwise convs on a zero-padded LDS image, BatchNorm passes on 16-byte "
                       "groups); no optimizer"}
        if not a.no_parity:
            from oracle import cruse_oracle_ext as X
            o = X.TFCM(24, (3, 3), 6)
            o.load_state_dict({k: v.detach().cpu() for k, v in tfcm.state_dict().items()})
            o.train(); tfcm.train()
            xin = torch.randn(1, 24, 161, 201, generator=torch.Generator().manual_seed(5))
            torch.set_num_threads(min(os.cpu_count() or 1, 16))
            with torch.no_grad():
                yo = o(xin)
                yp = to_f32(tfcm(to_f16(xin.to(dev)))).cpu()
            row["parity_rel_l2"] = float(f"{float((yp.double() - yo.double()).norm() / yo.double().norm()):.4g}")
            row["parity_note"] = "6 x TFCM_Block output in f16 storage vs the f32 CPU oracle on [1,24,161,201] (train-mode BatchNorm)"
        out["config5_mtfaa_fp16"] = row
    except Exception as ex:
        out["config5_mtfaa_fp16"] = {"error": repr(ex)[:300]}
    torch.cuda.synchronize()
    torch.cuda.set_stream(_prev5)
    return out


def _stream_probe_report():
    """what cruse_amd/streams.py measured when it chose this process's side / launcher / data streams (serial fraction per pool stream drawn:
    ~0.3 = runs beside the main stream, ~1 = shares its hardware queue) -- the first entries, the headline engine's among them"""
    try:
        from cruse_amd import streams
        return {"selections": len(streams.REPORT), "rejected_draws": sum(1 for r in streams.REPORT for f in r.get("serial_fraction_by_draw", [])[:-1]),
                "first": streams.REPORT[:4]}
    except Exception as ex:
        return {"error": repr(ex)[:120]}


def regression_guard(out, threshold=0.08):
    """every row of this run against the newest COMMITTED bench line (profiles/rNN_bench_final.json): a row
    whose ms per step grew by more than `threshold` is flagged -- in the JSON line and on stderr.  BENCH_r05's config-4 row went
    3.56 -> 5.92 ms in a commit that did not touch its path and nobody saw it.  Box-to-box spread of these rows is 1-2 %."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_final.json")))
    if not files:
        return {"reference": None}
    ref_file = files[-1]
    try:
        with open(ref_file) as f:
            ref = json.loads(f.read().strip().splitlines()[-1])
    except Exception as ex:
        return {"reference": os.path.basename(ref_file), "error": repr(ex)[:120]}
    same = (ref.get("config", {}).get("workload") == out["config"]["workload"] and ref.get("n_gpus") == out["n_gpus"]
            and ref.get("dtype") == out["dtype"])
    if not same:
        return {"reference": "profiles/" + os.path.basename(ref_file), "skipped": "reference line is for another workload / world size"}

    def rows_of(line):
        r = {"headline": line.get("ms_per_step")}
        for k, v in (line.get("secondary") or {}).items():
            if isinstance(v, dict):
                if v.get("ms_per_step") is not None:
                    r[k] = v["ms_per_step"]
                for k2, v2 in v.items():                          # nested rows (trainer_path.*, batch_sweep.*): time per frame
                    if isinstance(v2, dict) and v2.get("value") and v2.get("unit") == "frames/s":
                        r[f"{k}.{k2}"] = 1e6 / v2["value"]
        return r
    now, was = rows_of(out), rows_of(ref)
    flagged, checked = {}, 0
    for k, v in now.items():
        if v and was.get(k):
            checked += 1
            if v > (1.0 + threshold) * was[k]:
                flagged[k] = {"now": round(v, 3), "reference": round(was[k], 3), "ratio": round(v / was[k], 3)}
    missing = sorted(k for k in was if k not in now or not now[k])
    return {"reference": "profiles/" + os.path.basename(ref_file), "threshold": threshold, "rows_checked": checked, "flagged": flagged,
            "rows_missing_now": missing}


DUMP_LIMIT_BYTES = 64 << 20


def engine_state(eng) -> dict:
    """The parameters and BatchNorm buffers an engine starts from (taken before its first step)."""
    return {"params": eng.flat.params.clone(), "buffers": {k: b.clone() for k, b in eng.Bf.items()}}


def replay_one_step(eng, start: dict, noisy, clean) -> float:
    """Put the engine back to `start` with fresh Adam state and run ONE step of the timed path -- same engine, same launch form
    (the captured graphs when it replays them), same kernels -- on the given inputs; returns that step's loss.
    Why not dump the last timed step itself: the library's BatchNorm / bias reductions accumulate with atomics, so a step's
    gradients differ from run to run in the last bits, and every later Adam step carries that on; after tens of chained steps two
    runs of one build stood 1e-2 apart (rel-L2 of the parameters).  One step from the seeded start state is the same every run
    up to rounding.  (On every rank: the step all-reduces at world > 1.)"""
    eng.flat.params.copy_(start["params"])
    for k, b in start["buffers"].items():
        eng.Bf[k].copy_(b)
    for t in (eng.flat.grads, eng.flat.exp_avg, eng.flat.exp_avg_sq, eng._skipped, eng._health, eng._loss_acc):
        t.zero_()
    eng.step_count = 0
    ls = eng.step(noisy, clean)
    torch.cuda.synchronize()
    return eng.loss_value(ls)


def dump_outputs(out_dir: str, eng, loss: float) -> dict:
    """What the caller of TrainEngine.step holds after the step of replay_one_step(), as float32 / float64 .npy files: the loss,
    the parameters after Adam and the step's gradients (each concatenated in model.named_parameters() order, independent of the
    flat buffer's bucket layout), and the BatchNorm running statistics the forward pass updated.  Returns {name: shape}."""
    import numpy as np
    names = [n for n in eng.flat.order if n in eng.flat.G]
    stats = [b.reshape(-1).float() for k, b in eng.model.named_buffers() if k.endswith((".running_mean", ".running_var"))]
    arrays = {
        "loss": np.array([loss], dtype=np.float64),
        "params": torch.cat([eng.flat.P[n].reshape(-1) for n in names]).float().cpu().numpy(),
        "grads": torch.cat([eng.flat.G[n].reshape(-1) for n in names]).float().cpu().numpy(),
        "bn_running_stats": torch.cat(stats).cpu().numpy(),
    }
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)
    return {k: list(v.shape) for k, v in arrays.items()}


def main():
    a = parse()
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        raise SystemExit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus:
        raise SystemExit(f"bench.py --gpus {a.gpus} was started with WORLD_SIZE={world}: launch one rank per GPU "
                         f"(--nproc-per-node {a.gpus}), or drop the launcher and let bench.py start the ranks itself")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
    local = local % torch.cuda.device_count()         # (test rigs may oversubscribe one GPU)
    torch.cuda.set_device(local)
    from cruse_amd import hostpin
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    pin = hostpin.pin_rank(int(os.environ.get("LOCAL_RANK", "0")), local_world, device_index=local, enable=not a.no_pin)
    force_pg = os.environ.get("CRUSE_FORCE_COLLECTIVES") == "1"      # a world of ONE still issues its (RCCL) collectives
    backend = None
    if world > 1 or force_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:               # (world 1 with forced collectives, no launcher: any free port will do)
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        dist.init_process_group(os.environ.get("CRUSE_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
        backend = dist.get_backend()
        assert dist.get_world_size() == world
    dev = torch.device("cuda", local)

    from cruse_amd import ops
    from cruse_amd.data import synth_batch
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse_net import unet_2

    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        log("cpu baseline (oracle on host cores) ...")
        cpu = cpu_baseline(a.groups)
        log(f"cpu baseline done: {cpu['value']} frames/s on {cpu['cores']} threads")

    torch.manual_seed(0)
    model = unet_2(rnn_groups=a.groups, precision=a.prec).to(dev)
    parity = None
    if a.full and rank == 0 and not a.no_parity:
        log("parity figure: this model vs the CPU oracle at T=401, B=8 ...")
        parity = parity_figure(model, a.groups, a.prec)
        log(f"parity_rel_l2 = {parity:.3e}")
    # the measured-best defaults unless CRUSE_* variables ask for an A/B variant (EngineConfig.from_env: bench / tools only)
    from cruse_amd.config import EngineConfig
    cfg = EngineConfig.from_env()
    eng = TrainEngine(model, lr=1e-3, use_graph=not a.no_graph, bucketed=True if a.bucketed else None,
                      loss="wo_male_df" if a.df else "wo_male", config=cfg)
    B, L = a.batch, int(a.seconds * 16000)
    T = 1 + L // 160
    pool = [synth_batch(B, L, dev, 1234 + 1000 * rank + s) for s in range(4)]
    start = engine_state(eng) if a.dump_outputs else None

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    log("inputs ready; warm-up (includes HIP-graph capture) ...")
    launch_choice = None
    if not a.no_graph and not a.graph:
        # the same step, replayed from HIP graph(s) or launched eagerly: keep the faster form (per-rank timings, MAX over the ranks)
        def timed(mode, n=3):
            eng.use_graph = mode
            eng.step(*pool[0])                              # (capture / first-use work outside the measurement)
            sync()
            t = time.perf_counter()
            for i in range(n):
                eng.step(*pool[i % len(pool)])
            sync()
            return (time.perf_counter() - t) / n
        # two rounds each, best of the two: one-time stalls (stream / communicator set-up on first use) must not decide
        t_graph, t_eager = timed(True), timed(False)
        t_graph, t_eager = min(t_graph, timed(True)), min(t_eager, timed(False))
        # every rank measured its own pair; the job's verdict is taken on the SLOWEST rank's figures (MAX), identically everywhere
        # -- a step ends when the last rank's gradients arrive, and rank 0's host is not necessarily the busiest one
        tt = torch.tensor([t_graph, t_eager], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        t_graph, t_eager = float(tt[0].item()), float(tt[1].item())
        eng.use_graph = t_graph <= t_eager
        launch_choice = {"graph_ms": round(t_graph * 1e3, 3), "eager_ms": round(t_eager * 1e3, 3),
                         "kept": "graph" if eng.use_graph else "eager"}
        log(f"launch form: graph {t_graph * 1e3:.2f} ms, eager {t_eager * 1e3:.2f} ms -> {launch_choice['kept']}")
        done = 16
    else:
        done = 0
    # (Rounds 2-5 ran the eager loop from a HIGH-PRIORITY stream for 0.7 %.  Round 6: measured again it loses -- 4.75 against 4.69 ms --
    #  and a high-priority caller stream slows every graph replay of the process by 25-40 % and one or two in four side streams
    #  (cruse_amd/streams.py): every row of this file now runs on the default stream.)
    for s in range(max(a.warmup - done, 0)):                # (the form timing above already ran 16 untimed steps)
        eng.step(*pool[s % len(pool)])
    sync()
    # eager launches: a generational GC pause on the host (tens of ms over torch's object graph) is long enough to drain
    # the device queue and shows up as one 20-30 ms step in a hundred; the loop below allocates nothing that needs the GC
    import gc
    gc.collect()
    gc.disable()
    log("timed region ...")
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for s in range(a.steps):
        ls = eng.step(*pool[s % len(pool)])
        marks[s + 1].record()                 # on the compute stream, after this step's Adam
    sync()
    el = time.perf_counter() - t0
    gc.enable()
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps))
    med_ms = step_ms[len(step_ms) // 2]
    if world > 1:
        tmax = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        el = float(tmax.item())
    loss = eng.loss_value(ls)
    status = ops.gru_status() | eng.timeout_steps()      # (the engine latches and clears the device word every step)
    log(f"timed region done: {el / a.steps * 1e3:.2f} ms/step (median step {med_ms:.2f} ms)")
    skipped = eng.skipped_steps()
    dumped = None
    if a.dump_outputs:
        # after the timed steps (their figures and counters are taken above) and before any --full pass below
        dump_loss = replay_one_step(eng, start, *pool[(a.steps - 1) % len(pool)])
        if rank == 0:
            dumped = dump_outputs(a.dump_outputs, eng, dump_loss)
            log(f"outputs of one step from the seeded start on the last timed step's inputs written to {a.dump_outputs}: {dumped}")

    roof, breakdown = None, None
    if a.full and rank == 0 and not a.no_kernel_timing:
        with KernelTimer(ops, eng) as kt:
            eng._fwd_bwd(*pool[0])                       # un-graphed warm-up: allocator and attribute caches
            torch.cuda.synchronize()
            kt.rec.clear()
            for s in range(3):
                eng._fwd_bwd(*pool[s % len(pool)])
                kt.mark_pass()
            per_step, calls = kt.summary()
        rl = kernel_rooflines(B, T, model.hidden_size, a.groups, a.prec, per_step, calls, kt.bytes_per_launch())
        if (B, a.seconds, a.groups, a.prec) == (64, 4.0, 1, "bf16"):         # the shape the PMC passes were taken at
            pmc = pmc_traffic()
            util = pmc_mfma_util()
            for fam, ent in rl.items():
                if util.get(fam) is not None:
                    ent["mfma_util_pmc"] = util[fam]
                    ent["mfma_util_source"] = f"profiles/{os.path.basename(PMC_MFMA_FILE)} (SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE/8 * 1024 SIMDs))"
            for fam, ent in rl.items():
                if pmc.get(fam):
                    ent["traffic"] = round(pmc[fam])
                    ent["traffic_unit"] = "HBM bytes per launch (rocprofv3 PMC 2*FETCH_SIZE + WRITE_SIZE, " "profiles/" + os.path.basename(PMC_FILE) + ")"
        dom = max(per_step, key=per_step.get)
        breakdown = {k: round(v, 3) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])}
        roof = dict(rl.get(dom, {"bound": "hbm", "achieved": None, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                 "frac": None, "traffic": None}))
        roof["kernel"] = dom
        roof["ms_per_step_all_launches"] = round(per_step[dom], 3)
        # the same fraction from the committed rocprofv3 trace of the GRAPH run (the kernel beside its side-stream
        # co-runners), next to the isolated HIP-event figure above
        kname = {"gru_seq_bwd": "gru_bwd_ag_kernel", "gru_seq_fwd": "gru_fwd_lean_kernel"}.get(dom)
        if kname and roof.get("avg_launch_ms") and (B, a.seconds, a.groups, a.prec) == (64, 4.0, 1, "bf16"):
            ns, src = profile_avg_ns(kname)
            if ns:
                # `frac` / `achieved` are the IN-STEP figures (the kernel beside its side-stream co-runners, average launch duration of
                # the committed rocprofv3 trace of this command) -- the ones that follow from profiles/; the isolated HIP-event
                # measurement of this run is kept beside them
                roof["frac_isolated"], roof["achieved_isolated"] = roof["frac"], roof["achieved"]
                roof["avg_launch_ms_in_graph"] = round(ns * 1e-6, 4)
                scale = roof["avg_launch_ms"] / (ns * 1e-6)
                roof["frac_in_graph"] = round(roof["frac_isolated"] * scale, 5)
                roof["frac"], roof["achieved"] = roof["frac_in_graph"], round(roof["achieved_isolated"] * scale, 3)
                roof["in_graph_source"] = "profiles/" + src
        roof["others"] = {k: v for k, v in rl.items() if k != dom}

    secondary = None
    frames_per_s_headline = world * B * T * a.steps / el
    if a.full and rank == 0 and world == 1 and not a.no_secondary:
        secondary = secondary_rows(a, dev, pool)
        secondary.update(config_rows(a, dev, pool))
        log("secondary: trainer path (device-resident / host dataset) ...")
        secondary["trainer_path"] = trainer_path_rows(a, dev, frames_per_s_headline)
        try:
            log("secondary: host contention (7 sibling launch loops, unpinned / pinned) ...")
            secondary["host_contention"] = host_contention_row(a, dev, pool)
        except Exception as ex:
            secondary["host_contention"] = {"error": repr(ex)[:300]}
        if not force_pg:
            log("secondary: rccl world-1 bucketed schedule ...")
            secondary["rccl_world1_bucketed"] = rccl_world1_row(a, dev, pool)

    ranks_seen = devices_seen = None
    if world > 1 or force_pg:
        # which ranks did the collectives of THIS run actually reach: an all-gather of (rank, device index) over the backend
        ids = torch.tensor([rank, local], device=dev, dtype=torch.int64)
        got = [torch.zeros_like(ids) for _ in range(world)]
        dist.all_gather(got, ids)
        ranks_seen = sorted({int(g_[0].item()) for g_ in got})
        devices_seen = sorted({int(g_[1].item()) for g_ in got})
        dist.barrier()                        # rank 0's instrumented pass is done before anyone tears down
        dist.destroy_process_group()
    if rank == 0:
        frames = world * B * T * a.steps
        out = {
            "metric": "spectrogram frames/sec training CRUSE 16kHz 20ms-hop at 1/2/4/8 MI355X",
            "value": round(frames / el, 1), "unit": "frames/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(el / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": a.prec, "data": "synthetic",
            "world_size": world, "backend": ("rccl" if backend == "nccl" else backend), "bucketed_allreduce": bool(eng.bucketed),
            "rccl_ranks_seen": (None if ranks_seen is None else len(ranks_seen)), "devices_seen": devices_seen, "host_pinning_rank0": pin,
            "scaling_efficiency": (None if not a.ref_1gpu else round(frames / el / (world * a.ref_1gpu), 4)),
            "config": {"workload": f"CRUSE unet_2 4-layer enc/dec, {a.groups}xGRU group(s), H=640, "
                                   f"{B} clips x {a.seconds:g} s @16 kHz per GPU, n_fft=320 hop=160 (T={T}), "
                                   + ("STFT x2 + fwd + DeepFilter(1,5) head + WO-MALE + bwd" if a.df else "STFT x2 + fwd + WO-MALE + bwd")
                                   + " + grad all-reduce + Adam; f32 storage, "
                                   f"{a.prec} MFMA operands, f32 accumulate/statistics",
                       "framing": "20 ms frames (n_fft = win = 320) at a 10 ms hop (160): the reference's framing (conv_stft.py:10-11, "
                                  "audioAug.py:191); a literal 20 ms hop = win violates NOLA, so no iSTFT / training step exists for "
                                  "it -- its forward STFT is the secondary row stft_hop320_forward (SURVEY 8d)",
                       "global_batch": world * B, "per_gpu_batch": B, "frames_per_clip": T,
                       "parallelism": f"dp{world}", "engine_config_non_default": cfg.non_default(), "hip_graph": bool(eng.use_graph), "launch_form_timing": launch_choice, "bucketed_allreduce": bool(eng.bucketed)},
            "ms_per_step_median": round(med_ms, 3),
            "ms_per_step_p90_max": [round(step_ms[min(len(step_ms) - 1, int(0.9 * len(step_ms)))], 3), round(step_ms[-1], 3)],
            "value_at_median_step": round(world * B * T / (med_ms * 1e-3), 1),
            "parity_rel_l2": None if parity is None else float(f"{parity:.4g}"),
            "parity_note": "enhanced-spectrum rel-L2 of this model/mode vs the CPU oracle at T=401, B=8 (bar 1e-3)",
            "final_loss": round(loss, 6), "gru_handoff_timeouts": status, "skipped_steps": skipped,
            "stream_probe": _stream_probe_report(),
            "roofline": roof, "roofline_step": step_roofline(frames / el, a.groups, a.prec, B, T),
            "kernel_ms_per_step": breakdown, "cpu_baseline": cpu, "secondary": secondary, "full": a.full, "outputs_dumped": dumped,
        }
        out["regressions"] = regression_guard(out) if a.full else None
        # one compact line of row -> ms on stderr (the driver's tail of the JSON line itself cuts the secondary rows' head)
        rows = {"headline": out["ms_per_step"]}
        for k_, v_ in (secondary or {}).items():
            if isinstance(v_, dict) and v_.get("ms_per_step") is not None:
                rows[k_] = v_["ms_per_step"]
        log("ROWS ms/step: " + json.dumps(rows))
        if out["regressions"] and out["regressions"].get("flagged"):
            log("REGRESSIONS vs " + str(out["regressions"].get("reference")) + ": " + json.dumps(out["regressions"]["flagged"]))
        # RCCL writes a version banner through C stdio; push it out first so that the JSON line is the LAST line of stdout
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
