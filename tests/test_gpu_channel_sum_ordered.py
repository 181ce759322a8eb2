"""MI355X: cruse_channel_sum at few rows (<= 64: a training step of a few short clips) runs as one ordered workgroup, so the bias gradient
it forms has the same bits from run to run -- tests/test_gpu_mask_head.py::test_whole_step_on_and_off compares conv1_t.bias of three
runs bit for bit at 34 rows.  Above 64 rows the sum keeps its f32 atomics, whose order is free.

Bar against float64: an f32 sum of n terms in any order is within n * 2^-24 * sum |x|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (rows, C, F): the mask head's bias at B = 2, T = 17; the row bound with channels that straddle the 256-column chunks; one channel per
# column over several chunks; the first row count of the atomic form
SHAPES = [(34, 1, 160), (64, 8, 80), (7, 600, 1), (1, 3, 5), (65, 8, 80)]


@pytest.mark.parametrize("rows,C,F", SHAPES)
def test_channel_sum_few_rows_is_reproducible_and_right(rows, C, F):
    from cruse_amd import ops
    rng = np.random.default_rng(rows * 1000 + C)
    x = rng.standard_normal((rows, C, F)).astype(np.float32)
    start = rng.standard_normal(C).astype(np.float32)                           # out[c] += : the sum lands on what the buffer held
    g = torch.from_numpy(x).cuda()
    outs = []
    for _ in range(20):
        out = torch.from_numpy(start).cuda()
        ops.channel_sum(g, rows, C, F, out)
        outs.append(out.cpu())
    want = start.astype(np.float64) + x.astype(np.float64).sum(axis=(0, 2))
    bound = (rows * F + 1) * 2.0 ** -24 * (np.abs(start).astype(np.float64) + np.abs(x).astype(np.float64).sum(axis=(0, 2)))
    err = np.abs(outs[0].numpy().astype(np.float64) - want)
    print(f"rows {rows} C {C} F {F}: max error {err.max():.2e} (bound {bound.min():.2e} .. {bound.max():.2e})")
    assert (err <= bound).all()
    if rows <= 64:
        assert all(torch.equal(o.view(torch.int32), outs[0].view(torch.int32)) for o in outs[1:])
