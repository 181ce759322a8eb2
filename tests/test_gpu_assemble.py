"""GPU: cruse_assemble_clips (ops.assemble_clips) against the numpy plan executor of tests/filepairs_ref.py.  A copy:
compared with torch.equal.  The output is pre-filled with NaN, so a sample the kernel does not write shows, and sits between sentinels.
The graph replay of the same cases is tests/test_gpu_file_graphs.py (see there why it is a file of its own)."""
import numpy as np
import pytest
import torch

import filepairs_ref as R

pytestmark = pytest.mark.gpu

SENT = 12345.678
PAD = 64
POOL = np.random.default_rng(5).standard_normal(20000).astype(np.float32)


def assemble(seg, first, L, graph=False):
    from cruse_amd import ops
    seg, first = np.asarray(seg, dtype=np.int64).reshape(-1, 3), np.asarray(first, dtype=np.int32)
    B = len(first) - 1
    pool = torch.from_numpy(POOL).cuda()
    buf = torch.full((PAD + B * L + PAD,), SENT, device="cuda")
    out = buf[PAD:PAD + B * L].view(B, L)
    out.fill_(float("nan"))
    if graph:
        sd, fd = torch.from_numpy(seg).cuda(), torch.from_numpy(first).cuda()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.assemble_clips(pool, seg, first, L, out=out, seg_dev=sd, first_dev=fd)
        out.fill_(float("nan"))
        g.replay()
    else:
        assert ops.assemble_clips(pool, seg, first, L, out=out) is out
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.all(b[:PAD] == np.float32(SENT)) and np.all(b[-PAD:] == np.float32(SENT))
    want = torch.from_numpy(R.execute_segs(seg, first, POOL, L))
    got = out.cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got, want)
    return got


CASES = {
    "one cropped segment": ([[137, 0, 1000]], [0, 1], 1000),
    "utterance, gap, utterance": ([[0, 0, 300], [5000, 460, 540]], [0, 2], 1000),
    "all silence": ([], [0, 0], 1000),
    "odd edges": ([[1, 3, 5], [77, 9, 1], [1001, 11, 1013], [3, 1025, 1023], [19999, 4098, 1]], [0, 5], 4099),
    "three clips of 1000": ([[0, 0, 1000], [11, 1, 333], [3000, 500, 499], [7, 999, 1]], [0, 1, 1, 4], 1000),
    "three clips of 4099": ([[0, 0, 4099], [5000, 1023, 2], [6000, 1025, 2047], [9000, 3072, 1027], [123, 4000, 99]], [0, 1, 4, 5], 4099),
}


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_plan_executor(name):
    seg, first, L = CASES[name]
    got = assemble(seg, first, L)
    if name == "all silence":
        assert not got.any()
    if name == "three clips of 1000":
        assert not got[1].any() and got[0].any()                           # the middle clip has no segment


def test_a_planned_batch():
    """plans as the dataset makes them: plan_clip over a table of utterance lengths, B = 3"""
    from cruse_amd.filepairs import plan_clip
    lens = np.array([300, 1200, 50, 777, 4000, 2500])
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rng = np.random.default_rng(11)
    for L in (1000, 4099):
        segs, first = [], [0]
        for b in range(3):
            p = plan_clip(b if b < 2 else None, lens, L, 160, rng)
            segs.append(np.stack([start[p[:, 0]] + p[:, 1], p[:, 2], p[:, 3]], axis=1))
            first.append(first[-1] + p.shape[0])
        assemble(np.concatenate(segs), first, L)


def test_refusals():
    from cruse_amd import ops
    pool = torch.from_numpy(POOL).cuda()
    with pytest.raises(ValueError, match="overlap"):
        ops.assemble_clips(pool, np.array([[0, 0, 10], [50, 9, 5]], dtype=np.int64), [0, 2], 100)
    with pytest.raises(ValueError, match="pool"):
        ops.assemble_clips(pool, np.array([[19995, 0, 10]], dtype=np.int64), [0, 1], 100)
    with pytest.raises(RuntimeError, match="cruse_hip error -1"):
        ops.assemble_clips(pool, np.zeros((0, 3), dtype=np.int64), [0], 100)                  # B = 0
