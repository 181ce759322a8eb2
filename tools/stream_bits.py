"""Bit identity of the streaming chains (cruse_amd.inferencer.StreamingInferencer) between two builds of the library: the check of a
change that must not alter what the kernels compute.

    python tools/stream_bits.py --dump FILE       (needs a GPU; run it once from each tree, each in its own process)
    python tools/stream_bits.py --compare A B     (no GPU)

--dump builds four models of tests/stream_shapes.py, one per register tiling KQ = 3 / 5 / 10 / 16 of the f32 GRU kernel, three of them
with several GRU groups (the LN1 interleave), deterministic weights and BatchNorm statistics, and serves 9 slots (a full tile of 8 and a
partial one), every slot with its own seeded clip of 6 blocks:
  (i)  pushes, one of them inactive for every slot (a different one per slot), then flush;
  (ii) where the model admits packets: one push, then push_packet calls of up to min(bound, 3) blocks with ragged counts, then flush.
Both in precision "f32" and "f16".  Every returned block tensor and, after the last call, state / work / pwork / gi go to FILE (.npz).
--compare asserts that A and B hold the same arrays with the same bits and prints the first difference otherwise.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

MODELS = ("hg20_g3", "hg196_g5_odd", "hg400_bound", "hg660")                # KQ 3 (g = 3), 5 (g = 5), 10 (g = 2), 16 (g = 1)
S, NBLK = 9, 6


def build_model(cfg):
    import torch
    from cruse_amd.model.cruse_net import unet_2
    m = unet_2(precision="f32", **cfg)
    with torch.no_grad():
        for i, (name, p) in enumerate(list(m.named_parameters()) + list(m.named_buffers())):
            if not p.dtype.is_floating_point:
                continue
            s = torch.sin(0.37 * torch.arange(p.numel(), dtype=torch.float64) + 1.3 * i + 0.1)
            if name.endswith("running_var"):
                v = 1.0 + 0.3 * s
            elif name.endswith("running_mean"):
                v = 0.1 * s
            elif ".ln" in name or "bn" in name:
                v = 1.0 + 0.1 * s if name.endswith("weight") else 0.05 * s
            else:
                v = s / math.sqrt(max(p[0].numel() if p.dim() > 1 else p.numel(), 1))
            p.copy_(v.reshape(p.shape).to(p.dtype))
    return m.cuda().eval()


def dump(path):
    import torch
    from cruse_amd import ops
    from cruse_amd.inferencer import StreamingInferencer
    from tests.stream_shapes import SHAPES, geometry, kq_of
    assert {kq_of(geometry(SHAPES[n])[3]) for n in MODELS} == {3, 5, 10, 16}
    clips = torch.stack([0.1 * torch.randn(NBLK, 160, generator=torch.Generator().manual_seed(100 + s)) for s in range(S)]).cuda()
    every = list(range(S))
    res = {}

    def keep(key, t):
        torch.cuda.synchronize()
        res[key] = t.detach().cpu().numpy().copy()

    def keep_rows(tag, inf):
        for name in ("state", "work", "pwork", "gi"):
            if hasattr(inf, name):
                keep(f"{tag}.{name}", getattr(inf, name))

    for name in MODELS:
        cfg = SHAPES[name]
        m = build_model(cfg)
        hops = min(ops.stream_packet_layout(geometry(cfg)[0])["max_hops"], 3)
        for prec in ("f32", "f16"):
            tag = f"{name}.{prec}.push"
            inf = StreamingInferencer(m, S, precision=prec)
            sent = np.zeros(S, dtype=np.int64)
            for t in range(NBLK + 1):                                       # slot s sits out push s % (NBLK + 1)
                act = np.array([t != s % (NBLK + 1) for s in every])
                blocks = clips[torch.arange(S), torch.from_numpy(np.minimum(sent, NBLK - 1)).cuda()]
                out, valid = inf.push(blocks, act)
                keep(f"{tag}.out{t}", out)
                res[f"{tag}.valid{t}"] = valid.numpy().copy()
                sent += act
            assert (sent == NBLK).all()
            keep(f"{tag}.flush", inf.flush(every))
            keep_rows(tag, inf)
            if hops < 2:
                continue
            tag = f"{name}.{prec}.packet{hops}"
            inf = StreamingInferencer(m, S, precision=prec, max_hops=hops)
            out, _ = inf.push(clips[:, 0])
            keep(f"{tag}.out0", out)
            sent, call = np.ones(S, dtype=np.int64), 0
            while (sent < NBLK).any():
                cnt = np.minimum(NBLK - sent, [1 + (s + call) % hops for s in every])
                pkt = torch.zeros(S, hops, 160, device="cuda")
                for s in every:
                    pkt[s, :cnt[s]] = clips[s, sent[s]:sent[s] + cnt[s]]
                out, n_out = inf.push_packet(pkt, cnt)
                call += 1
                keep(f"{tag}.out{call}", out)
                res[f"{tag}.n_out{call}"] = n_out.numpy().copy()
                sent += cnt
            keep(f"{tag}.flush", inf.flush(every))
            keep_rows(tag, inf)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **res)
    print(f"stream_bits: {len(res)} arrays, {sum(v.nbytes for v in res.values())} bytes -> {path} (library of {os.path.dirname(ops.__file__)}, "
          f"HIP {torch.version.hip})")


def compare(pa, pb) -> int:
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print(f"stream_bits: DIFFERENT array names: only in A {sorted(set(a.files) - set(b.files))}, only in B {sorted(set(b.files) - set(a.files))}")
        return 1
    for k in a.files:
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            print(f"stream_bits: DIFFERENT {k}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}")
            return 1
        if x.tobytes() != y.tobytes():
            bx, by = x.reshape(-1).view(np.uint8).reshape(x.size, -1), y.reshape(-1).view(np.uint8).reshape(y.size, -1)
            i = int(np.flatnonzero((bx != by).any(axis=1))[0])
            n = int((bx != by).any(axis=1).sum())
            print(f"stream_bits: DIFFERENT {k}: {n} of {x.size} elements, first at {np.unravel_index(i, x.shape)}: "
                  f"{x.reshape(-1)[i]!r} vs {y.reshape(-1)[i]!r}")
            return 1
    print(f"stream_bits: {len(a.files)} arrays bit-identical")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if (a.dump is None) == (a.compare is None):
        ap.error("give --dump FILE or --compare A B")
    if a.dump:
        dump(a.dump)
        return 0
    return compare(*a.compare)


if __name__ == "__main__":
    sys.exit(main())
