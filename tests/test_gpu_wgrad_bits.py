"""GPU: cruse_conv_wgrad gives the BITS the library gave before its host path was gathered onto one call descriptor.

tests/golden/wgrad_bits_parent.npz holds dw as a build of the parent commit computed it on an MI355X, from dw = 0 and the seeded CPU inputs
of inputs() below, for the cases of cases(): the ragged shapes of test_gpu_kernels.py::test_conv_wgrad_register_direct_kernel except
(5, 21, ...), plus one odd-width shape that only the VALU kernel takes, at prec -1 / 0 / 1 / 2 -- and, on five of them, prec 2 with the
register-direct kernel switched off, which is how the LDS-staged kernel is reached in the bf16 mode.  Every case writes at most 16 slabs
(asserted from the plan): one chunk of the reduce, so one atomic per output onto zero and a fixed summation order.
Not in the file: the three calls the library refuses (REFUSED: the VALU kernel's channel rules at prec -1), and the seven prec -1 cases
of NOT_REPRODUCIBLE, where the parent itself gave different bits in two runs.  Those are VALU launches with fewer than 128 output tiles:
conv_wgrad_kernel sums the 256 / NT threads of an output tile with f32 atomics in LDS, and three or more addends land in a free order.
With 128 or 256 tiles (Ca = 64) there are two or one, so the VALU cases that remain -- three at prec -1 and the odd-width shape at every
prec -- have a fixed order; the parent gave the same bits in two runs of every case recorded.
Kernels reached: VALU at every prec, LDS-staged MFMA at 0 / 1 / 2, register-direct at 2 (asserted from the plans)."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_bits_parent.npz")
# (B, T, Ca, Fa, Cb, KT, S, pad); Fb = S * Fa
SHAPES = [(2, 5, 8, 8, 1, 2, 2, 1), (3, 1, 16, 12, 8, 2, 2, 1), (1, 2, 32, 20, 16, 2, 2, 1), (2, 7, 64, 10, 32, 2, 2, 1), (2, 9, 24, 10, 12, 2, 2, 1),
          (2, 5, 8, 40, 1, 1, 2, 0), (3, 3, 16, 12, 8, 1, 2, 0), (2, 4, 64, 10, 32, 1, 2, 0), (1, 6, 40, 20, 24, 1, 2, 0),
          (2, 5, 8, 16, 8, 1, 1, 1), (3, 3, 32, 20, 32, 1, 1, 1), (2, 4, 64, 10, 64, 1, 1, 1), (1, 11, 12, 12, 40, 1, 1, 1),
          (2, 5, 64, 9, 64, 1, 1, 1)]                   # (last: Fa = 9, odd -- the VALU kernel at every prec; 256 output tiles)
STAGED_AT_BF16 = (0, 1, 5, 6, 9)                       # shapes that also run prec 2 with wg_rd = 0
REFUSED = {"s4_p0", "s8_p0", "s12_p0"}
NOT_REPRODUCIBLE = {"s0_p0", "s1_p0", "s2_p0", "s5_p0", "s6_p0", "s9_p0", "s10_p0"}
EXPECTED = {-1: {"valu"}, 0: {"valu", "mfma"}, 1: {"valu", "mfma"}, 2: {"valu", "mfma", "rd"}}


def cases(i):
    """(prec, wg_rd) of shape i"""
    return [(-1, None), (0, None), (1, None), (2, None)] + ([(2, 0)] if i in STAGED_AT_BF16 else [])


def name(i, prec, wg_rd):
    return "s%d_p%d%s" % (i, prec + 1, "" if wg_rd is None else "_staged")


def inputs(i):
    B, T, Ca, Fa, Cb, KT, S, pad = SHAPES[i]
    gen = torch.Generator().manual_seed(4100 + i)
    return torch.randn(B, T, Ca, Fa, generator=gen), torch.randn(B, T, Cb, S * Fa, generator=gen)


def run(ops, i, prec, wg_rd):
    """dw from zero on the device, or None where the library refuses the call"""
    B, T, Ca, Fa, Cb, KT, S, pad = SHAPES[i]
    a, bt = inputs(i)
    dw = torch.zeros(Ca, Cb, KT, 3).cuda()
    with (ops.options() if wg_rd is None else ops.options(wg_rd=wg_rd)):
        try:
            ops.conv_wgrad(a.cuda(), bt.cuda(), dw, B, T, Ca, Fa, Cb, S * Fa, KT=KT, S=S, pad=pad, prec=prec)
        except RuntimeError:
            return None
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.fixture(scope="module")
def ops():
    from cruse_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def test_the_recorded_file_reaches_every_kernel_at_every_prec(ops, golden):
    reached = {p: set() for p in EXPECTED}
    for i, (B, T, Ca, Fa, Cb, KT, S, pad) in enumerate(SHAPES):
        for prec, wg_rd in cases(i):
            if name(i, prec, wg_rd) in golden:
                with (ops.options() if wg_rd is None else ops.options(wg_rd=wg_rd)):
                    reached[prec].add(ops.conv_wgrad_plan(B, T, Ca, Fa, Cb, S * Fa, KT, S, pad, prec)["kernel"])
    assert reached == EXPECTED, reached
    every = {name(i, p, w) for i in range(len(SHAPES)) for p, w in cases(i)}
    assert set(golden) == every - REFUSED - NOT_REPRODUCIBLE and all(n.endswith("_p0") for n in REFUSED | NOT_REPRODUCIBLE)     # prec -1 only


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=lambda i: "-".join(map(str, SHAPES[i])))
def test_conv_wgrad_bits_are_the_parents(ops, golden, i):
    B, T, Ca, Fa, Cb, KT, S, pad = SHAPES[i]
    for prec, wg_rd in cases(i):
        if name(i, prec, wg_rd) in NOT_REPRODUCIBLE:
            continue
        if name(i, prec, wg_rd) in REFUSED:
            assert run(ops, i, prec, wg_rd) is None
            continue
        want = golden[name(i, prec, wg_rd)]
        with (ops.options() if wg_rd is None else ops.options(wg_rd=wg_rd)):
            plan = ops.conv_wgrad_plan(B, T, Ca, Fa, Cb, S * Fa, KT, S, pad, prec)
        assert plan["slabs"] <= 16 and plan["reduce_grid"][1] == 1, plan
        got = run(ops, i, prec, wg_rd)
        assert got is not None and torch.equal(got, want), (prec, wg_rd, plan)
