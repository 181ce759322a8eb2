"""Test-only: the shape matrix of the streaming kernels (cruse_stream_*), shared by tests/test_stream_host.py (CPU pins of the
reference at these shapes), tests/test_gpu_stream_shapes.py and tools/guard_stream_steps.py.

The f32 GRU kernel of cruse_amd/csrc/stream.hip (step, packet projection, packet recurrent step) is a template on KQ, the number of 64-lane
slices of a group's row a lane holds in registers; kq_of restates the dispatcher's thresholds.  Every row names what it is there for:
  KQ 3 / 5 / 10 / 16 each at a width that is not a multiple of 64 (a partly masked slice) and at its upper edge, Hg < 64 (one wave
  holds a whole row), odd channel counts (layout padding, odd LDS row strides), g = 3 and 5, the widest rows the layout accepts,
  and a model whose packet bound is small enough to run packets at exactly that bound.
"""
from __future__ import annotations

SHAPES = {
    "hg320_g2": dict(rnn_groups=2),                                   # <5> exact upper edge, the default ch
    "hg196_g5_odd": dict(ch=(1, 5, 7, 9, 98), rnn_groups=5),          # <5> first width above 192, partial slice, odd channels
    "hg200_odd": dict(ch=(1, 3, 5, 7, 20), rnn_groups=1),             # <5> partial slice with a channel count that admits packets
    "hg192_g5": dict(ch=(1, 4, 8, 16, 96), rnn_groups=5),             # <3> upper edge
    "hg100_odd": dict(ch=(1, 3, 6, 5, 10), rnn_groups=1),             # <3> partial slice, odd channels throughout
    "hg20_g1": dict(ch=(1, 2, 2, 2, 2), rnn_groups=1),                # Hg < 64
    "hg20_g3": dict(ch=(1, 4, 8, 16, 6), rnn_groups=3),               # Hg < 64, three groups
    "hg400_bound": dict(ch=(1, 12, 24, 48, 80), rnn_groups=2),        # <10> partial; packet bound 2..4: packets AT the bound
    "hg660": dict(ch=(1, 4, 8, 16, 66), rnn_groups=1),                # <16> partial, first slices
    "hg900": dict(ch=(1, 4, 8, 16, 90), rnn_groups=1),                # <16> partial, 15 slices, the widest that admits packets
    "hg1020": dict(ch=(1, 4, 8, 16, 102), rnn_groups=1),              # <16> near the limit (no packets: the skip weights fill LDS)
    "widest": dict(ch=(1, 25, 51, 102, 204), rnn_groups=2),           # rows of 2000 / 2040 floats, Hg 1020 (no packets)
}
DEFAULT_CH = (1, 8, 16, 32, 64)


def geometry(cfg):
    """(ch, groups, H, Hg) of a unet_2 configuration at 160 input bins"""
    ch, g = tuple(cfg.get("ch", DEFAULT_CH)), cfg.get("rnn_groups", 4)
    H = ch[4] * 10
    return ch, g, H, H // g


def kq_of(Hg: int) -> int:
    """the KQ instantiation cruse_stream_gru / _gru_proj_n / _gru_rec_n dispatch a group width to"""
    assert 0 < Hg <= 1024 and Hg % 4 == 0, Hg
    return 3 if Hg <= 192 else 5 if Hg <= 320 else 10 if Hg <= 640 else 16


def gru_grids(S: int, H: int, hops: int = 0):
    """{launch: (ntiles, grid_x)} of the GRU launches for S slots: tiles of 8 slots (8 (slot, frame) rows in the packet projection,
    hops + 1 rows per slot), grid_x = min(ntiles, ceil(2048 / (H / 4))) workgroup columns that stride over the tiles"""
    units = H // 4
    cap = (2048 + units - 1) // units
    tiles = {"stream_gru": (S + 7) // 8}
    if hops:
        tiles["stream_gru_proj_n"] = (S * (hops + 1) + 7) // 8
        tiles["stream_gru_rec_n"] = (S + 7) // 8
    return {k: (n, max(1, min(n, cap))) for k, n in tiles.items()}
