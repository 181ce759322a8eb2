"""f16-mode streaming chains for tools/engine_guard_run.py (every torch tensor end-aligned in its own hipMalloc block: an access past a tensor
faults).  The cruse_stream_gru*_f16 kernels stage tiles of 16 rows and pad K to 32 and units to 16 in their f16 weight pack: rows beyond S, the
K padding and the unit padding must be staged as zeros / masked at the store, never read or written.  With S = 1 and S = 3 slots, eager launches
(no HIP graphs under the guard allocator), StreamingInferencer(precision="f16"): a short clip through push + flush and one through push_packet
at max_hops = 2 (a single push first, so that a packet computes max_hops + 1 frames) -- for Hg = 100 with odd channels, Hg = 20 in three groups
and the widest rows the layout accepts (Hg = 1020; no packets).  Every output is compared with the CPU emulation (tests/stream_ref_f16.py) and
held to the f16 mode's whole-clip bar, twice the emulation's own distance from float64, so a run that did nothing cannot pass.
Prints "guard stream f16 ok" when no kernel left its tensors.  Run once by tests/test_gpu_stream_f16.py in a subprocess."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cruse_amd import ops                                             # noqa: E402
from cruse_amd.inferencer import StreamingInferencer                  # noqa: E402
from tests import stream_ref_f16 as R                                 # noqa: E402
from tests.stream_shapes import SHAPES, geometry                      # noqa: E402
from tests.test_gpu_stream_packets import run_packets                 # noqa: E402
from tests.test_gpu_streaming import stream_all                       # noqa: E402

n = 0


def compare(tag, got, refs):
    global n
    assert got.shape[0] == len(refs), tag
    for s, (ref64, e_emu) in enumerate(refs):
        err = R.rel(got[s].cpu(), ref64)
        print(f"{tag} slot {s}: vs float64 {err:.2e}, emulation {e_emu:.2e}, ratio {err / e_emu:.2f}", flush=True)
        assert got[s].numel() == ref64.numel() and err <= 2 * e_emu, (tag, s, err, e_emu)
        n += 1


def refs_of(o, clips):
    out = []
    for c in clips:
        ref64, _, _, _, e_emu = R.references(o, c)
        out.append((ref64, e_emu))
    return out


for name in ("hg100_odd", "hg20_g3", "widest"):
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    o = R.oracle_model(cfg)
    m = R.gpu_model(o, cfg)
    bound = ops.stream_packet_layout(ch)["max_hops"]
    for S in (1, 3):
        clips = torch.stack([R.clip(6, 300 + 10 * S + i) for i in range(S)])
        inf = StreamingInferencer(m, S, use_graph=False, precision="f16")
        compare(f"{name} S {S} f16 push + flush", stream_all(inf, clips), refs_of(o, clips))
        if bound >= 2:
            K, nb = 2, 7
            clips = torch.stack([R.clip(nb, 400 + 10 * S + i) for i in range(S)])
            inf = StreamingInferencer(m, S, use_graph=False, max_hops=K, precision="f16")
            compare(f"{name} S {S} f16 push_packet max_hops {K}", run_packets(inf, clips, ["p", 2, 2, 2]), refs_of(o, clips))
torch.cuda.synchronize()
print(f"guard stream f16 ok ({n} clips compared)")
