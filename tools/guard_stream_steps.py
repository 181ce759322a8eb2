"""Streaming chains for tools/engine_guard_run.py (every torch tensor end-aligned in its own hipMalloc block: an access past a tensor faults).
The cruse_stream_* kernels index per-slot rows of shared [S, stride] arrays (state, work, pwork, gi, blocks, pout); with the caching allocator an
over-read from any slot but the last lands in a neighbour's row.  Here, with S = 1 and S = 3 slots, eager launches (no HIP graphs under the guard
allocator): a short clip through push + flush, one through push_packet at max_hops = 2 and at the model's LDS bound, one enhance() of a length that
is not a multiple of 160 -- for the odd-channel model, an Hg < 64 model and the widest rows the layout accepts (tests/stream_shapes.py).  Every
output is compared with the float64 CPU restatement (tests/stream_ref.py), so a run that did nothing cannot pass.
Prints "guard stream ok" when no kernel left its tensors.  Run by tests/test_gpu_guard.py in a subprocess."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cruse_amd import ops                                             # noqa: E402
from cruse_amd.inferencer import StreamingInferencer                  # noqa: E402
from oracle import cruse_oracle as O                                  # noqa: E402
from tests.stream_ref import as_double, stream_clip                   # noqa: E402
from tests.stream_shapes import SHAPES, geometry                      # noqa: E402
from tests.test_gpu_stream_packets import run_packets                 # noqa: E402
from tests.test_gpu_streaming import models, stream_all               # noqa: E402
from tests.util import rel_l2                                         # noqa: E402

BAR = 2e-5                                                            # the project's whole-clip bar
n = 0


def compare(tag, got, refs):
    global n
    assert got.shape[0] == len(refs), tag
    for s, ref in enumerate(refs):
        err = rel_l2(got[s].cpu(), ref)
        print(f"{tag} slot {s}: {err:.2e}", flush=True)
        assert got[s].numel() == ref.numel() and err <= BAR, (tag, s, err)
        n += 1


for name in ("hg100_odd", "hg20_g3", "widest"):
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    o, m = models(cfg)
    od = as_double(o)
    bound = ops.stream_packet_layout(ch)["max_hops"]
    for S in (1, 3):
        nb = 6
        clips = torch.cat([O.synth_pair(1, 160 * nb, seed=300 + 10 * S + i)[0] for i in range(S)])
        refs = [stream_clip(od, clips[i], dtype=torch.float64)[0] for i in range(S)]
        compare(f"{name} S {S} push + flush", stream_all(StreamingInferencer(m, S, use_graph=False), clips), refs)
        if bound < 2:                                                  # the widest rows: the constructor refuses packets
            try:
                StreamingInferencer(m, S, use_graph=False, max_hops=2)
            except ValueError:
                pass
            else:
                raise AssertionError(f"{name}: max_hops = 2 accepted at a packet bound of {bound}")
        for K in ((2, bound) if bound >= 2 else ()):
            # a single push, then a packet of K (K + 1 frames: every work row), then packets of K and the remainder
            nb = K + 5
            clips = torch.cat([O.synth_pair(1, 160 * nb, seed=400 + 10 * S + i)[0] for i in range(S)])
            refs = [stream_clip(od, clips[i], dtype=torch.float64)[0] for i in range(S)]
            sizes, left = ["p", K], nb - 1 - K
            while left:
                sizes.append(min(K, left))
                left -= sizes[-1]
            inf = StreamingInferencer(m, S, use_graph=False, max_hops=K)
            compare(f"{name} S {S} push_packet max_hops {K}", run_packets(inf, clips, sizes), refs)
        # enhance(): a length that is not a multiple of 160 equals the restatement of the zero-padded clip, trimmed
        L = 160 * 9 + 37
        odd = torch.cat([O.synth_pair(1, L, seed=500 + 10 * S + i)[0] for i in range(S)])
        padded = torch.zeros(S, 160 * 10)
        padded[:, :L] = odd
        refs = [stream_clip(od, padded[i], dtype=torch.float64)[0][:L] for i in range(S)]
        inf = StreamingInferencer(m, S, use_graph=False, max_hops=3 if bound >= 3 else 1)
        compare(f"{name} S {S} enhance", inf.enhance(odd.cuda()), refs)
torch.cuda.synchronize()
print(f"guard stream ok ({n} clips compared)")
