"""MI355X: StreamingInferencer(precision="f16") -- the GRU layers of the streaming chains on f16-operand MFMA kernels
(cruse_stream_gru_f16 / _gru_proj_n_f16 / _gru_rec_n_f16).

References, both on the CPU from the oracle's modules: the FLOAT64 per-frame restatement (tests/stream_ref.py) and the EMULATION
(tests/stream_ref_f16.py: the same restatement with x, h, W_ih, W_hh of every GRU cell rounded through torch.float16).  Bars:
  stages in front of the GRU in a frame (spectrum, e1..e4, skip1..4)   1e-5 rel-L2 per frame, as in f32 mode
  gru1, gru2, mask                                                     1e-3 rel-L2 per frame, the project's reduced-precision bar
  whole clip                                                           2 x the emulation's own distance from float64 for that clip
The factor 2: kernel and emulation sum in different orders, so an operand near an f16 rounding boundary can round the other way; they are
two draws of one error process.  tests/test_stream_f16_host.py shows the emulation alone inside 1e-3 on the same models and clips."""
import os
import subprocess
import sys

import pytest
import torch

from tests import stream_ref_f16 as R
from tests.stream_shapes import SHAPES, geometry
from tests.test_gpu_stream_packets import _serve_packets, even_sizes, run_packets
from tests.test_gpu_streaming import _chain, _serve, stage_errors, stream_all

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _inf(m, S, **kw):
    from cruse_amd.inferencer import StreamingInferencer
    return StreamingInferencer(m, S, precision="f16", **kw)


def _bound(ch):
    from cruse_amd import ops
    return ops.stream_packet_layout(ch)["max_hops"]


def _push_frames(m, x):
    """the clip through the single-hop f16 chain, eager: [(stages, output block, frame index)] of frames 0..nb"""
    from cruse_amd import ops
    nb = x.numel() // 160
    inf = _inf(m, 1, use_graph=False)
    blocks = x.view(nb, 160).cuda()
    res = []
    inf.blocks.copy_(blocks[0:1])
    _chain(inf, 1, [ops.STREAM_STORE])
    inf.blocks.copy_(blocks[1:2])
    st, out, _ = _chain(inf, 0, [ops.STREAM_FRAME0])
    res.append((st, out, 0))
    st, out, _ = _chain(inf, 1, [ops.STREAM_FRAME])
    res.append((st, out, 1))
    for b in range(2, nb):
        inf.blocks.copy_(blocks[b:b + 1])
        st, out, _ = _chain(inf, 1, [ops.STREAM_FRAME])
        res.append((st, out, b))
    st, out, _ = _chain(inf, 1, [ops.STREAM_END])
    res.append((st, out, nb))
    return res


def _packet_frames(m, x, K, sizes):
    """the clip through f16 push_packet calls of the given sizes ("p": a single push), eager: every frame computed inside a packet and
    the frame a push leaves in the single-hop work row, then the end frame.  The push that follows block 0 computes frames 0 and 1 in
    two chains and leaves frame 1 alone to be seen; frame 0 is then not in the result."""
    from cruse_amd import ops
    nb = x.numel() // 160
    inf = _inf(m, 1, use_graph=False, max_hops=K)
    blocks = x.view(1, nb, 160).cuda()
    res, b, t = [], 0, 0
    for c in sizes:
        if c == "p":
            out, valid = inf.push(blocks[:, b])
            torch.cuda.synchronize()
            b += 1
            if b == 1:                                                      # block 0: stored, no frame
                continue
            if b == 2:                                                      # frames 0 and 1
                t = 1
            st = {k: v.cpu().clone() for k, v in inf.stage(0).items()}
            assert bool(valid[0])
            res.append((st, out[0].cpu(), t))
            t += 1
            continue
        inf.push_packet(blocks[:, b:b + c])
        torch.cuda.synchronize()
        b += c
        for f in range(int(inf._last_frames[0])):
            st = {k: v.cpu().clone() for k, v in inf.stage(0, f).items()}
            res.append((st, st.get("block"), t))
            t += 1
    assert b == nb and t == nb, (b, t)
    inf._last_frames[:] = 0
    st, out, _ = _chain(inf, 1, [ops.STREAM_END])
    res.append((st, out, nb))
    return res


def _check_frames(tag, got, frames64):
    """print the worst error of each class of stages (before anything is asserted), then hold every frame to the two per-stage bars"""
    worst32, worst16 = (0.0, None, None), (0.0, None, None)
    errs = []
    for st, out, t in got:
        e = stage_errors(st, out, frames64[t], t)
        errs.append((t, e))
        for k, v in e.items():
            if k in R.STAGES_F16:
                worst16 = max(worst16, (v, k, t))
            elif k != "block":
                worst32 = max(worst32, (v, k, t))
    print(f"{tag}: {len(got)} frames; in front of the GRU worst {worst32[0]:.2e} ({worst32[1]}, frame {worst32[2]}); "
          f"gru1 / gru2 / mask worst {worst16[0]:.2e} ({worst16[1]}, frame {worst16[2]})")
    for t, e in errs:
        for k, v in e.items():
            if k in R.STAGES_F16:
                assert v <= R.BAR_F16, (tag, t, k, v)
            elif k != "block":
                assert v <= R.BAR_F32, (tag, t, k, v)
    return worst16[0]


def _check_clip(tag, y, ref64, e_emu):
    err = R.rel(y, ref64)
    print(f"{tag}: whole clip vs float64 {err:.2e}; emulation vs float64 {e_emu:.2e}; ratio {err / e_emu:.2f}")
    assert y.shape == ref64.shape, tag
    assert err <= 2 * e_emu, (tag, err, e_emu)
    assert err > 4e-7, (tag, err, "this is the f32 path's error: the f16 kernels did not run")


# ---- 1. accuracy against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_accuracy_against_float64(name):
    cfg = R.CONFIGS[name]
    o = R.oracle_model(cfg)
    m = R.gpu_model(o, cfg)
    x = R.clip(R.ACC_BLOCKS, R.ACC_SEED)
    ref64, frames64, _, _, e_emu = R.references(o, x)
    _check_frames(f"{name} push + flush", _push_frames(m, x), frames64)
    _check_clip(f"{name} push + flush (graph)", stream_all(_inf(m, 1), x.view(1, -1))[0], ref64, e_emu)
    for K in (2, 4, 8):
        sizes = even_sizes(R.ACC_BLOCKS, K)
        _check_frames(f"{name} packets of {K}", _packet_frames(m, x, K, sizes), frames64)
        _check_clip(f"{name} packets of {K} (graph)", run_packets(_inf(m, 1, max_hops=K), x.view(1, -1), sizes)[0], ref64, e_emu)


# ---- 2. every instantiation -------------------------------------------------------------------------------------------------------
def test_matrix_has_widths_that_need_padding():
    hgs = [geometry(c)[3] for c in SHAPES.values()]
    assert any(h % 32 for h in hgs) and any(h % 16 for h in hgs), hgs     # K padded to 32, units padded to 16
    assert min(hgs) <= 20 and max(hgs) >= 1020


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_matrix(name):
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    x = R.clip(R.SHAPE_BLOCKS, R.SHAPE_SEED)
    o, seed = R.alive_model(cfg, x)                                        # the reference alone picks the model (see alive_model)
    m = R.gpu_model(o, cfg)
    assert (m.hidden_size, m.rnn_groups) == (H, g)
    ref64, frames64, _, _, e_emu = R.references(o, x)
    bound = _bound(ch)
    print(f"{name}: model seed {seed} ch {ch} g {g} H {H} Hg {Hg} (K padded to {(Hg + 31) // 32 * 32}, units to {(Hg + 15) // 16 * 16}) packet bound {bound}")
    _check_frames(f"{name} push + flush", _push_frames(m, x), frames64)
    _check_clip(f"{name} push + flush (graph)", stream_all(_inf(m, 1), x.view(1, -1))[0], ref64, e_emu)
    if bound >= 2:
        K = min(bound, 4)
        sizes = even_sizes(R.SHAPE_BLOCKS, K)
        _check_frames(f"{name} packets of {K}", _packet_frames(m, x, K, sizes), frames64)
        _check_frames(f"{name} a push, then packets of {K}", _packet_frames(m, x, K, ["p"] + even_sizes(R.SHAPE_BLOCKS - 1, K)), frames64)
        _check_clip(f"{name} packets of {K} (graph)", run_packets(_inf(m, 1, max_hops=K), x.view(1, -1), sizes)[0], ref64, e_emu)


# ---- 3. slot tilings --------------------------------------------------------------------------------------------------------------
# The kernels walk tiles of 16 rows (32 where S > 16 and the padded K is <= 512), rows = slots, or (slot, frame) pairs with hops + 1 rows
# per slot in the packet projection, on grid_x = min(ntiles, ceil(512 / (g * ceil(ceil(Hg / 16) / 4)))) workgroup columns that stride.
#   widest: g 2, Hg 1020: 32 workgroup rows, 16 columns of 16 slots; S = 260 is 17 tiles: the columns stride (no packets at this shape)
#   hg320_g2: g 2, Hg 320 (two tiles of 16 rows per pass): 10 workgroup rows, 52 columns of 32 rows; S = 333, K = 4: the projection has
#           1665 rows = 53 tiles: the two-tile instantiation strides, its last tile holds one row
#   hg900:  g 1, Hg 900: 15 workgroup rows, 35 columns; S = 141, K = 3 (its packet bound): the projection has 564 rows = 36 tiles and strides
def f16_grid(S, g, Hg, rows_per_slot=1):
    R_ = S * rows_per_slot
    kp, ut = (Hg + 31) // 32 * 32, (Hg + 15) // 16
    rt = 32 if R_ > 16 and kp <= 512 else 16
    by = g * ((ut + 3) // 4)
    ntiles = (R_ + rt - 1) // rt
    return ntiles, max(1, min(ntiles, (512 + by - 1) // by))


TILINGS = [("hg100_odd", 15, 4), ("hg100_odd", 16, 4), ("hg100_odd", 17, 4), ("hg100_odd", 33, 2), ("widest", 260, 0), ("hg900", 141, 3),
           ("hg320_g2", 333, 4)]


@pytest.mark.parametrize("name,S,K", TILINGS, ids=[f"{n}-S{s}-K{k}" for n, s, k in TILINGS])
def test_slot_tilings_every_slot_compared(name, S, K):
    cfg = SHAPES[name]
    ch, g, H, Hg = geometry(cfg)
    o = R.oracle_model(cfg)
    m = R.gpu_model(o, cfg)
    big = S > 100
    step, proj = f16_grid(S, g, Hg), f16_grid(S, g, Hg, K + 1)
    print(f"{name} S {S} K {K}: Hg {Hg}; (ntiles, grid_x) step {step}, projection {proj}")
    if name == "widest":
        assert step[0] > step[1]                                            # the stride loop of the step kernel iterates
    if name in ("hg900", "hg320_g2"):
        assert proj[0] > proj[1]                                            # and that of the packet projection
        assert (((Hg + 31) // 32 * 32) <= 512) == (name == "hg320_g2")      # hg320_g2: with two row tiles per pass
    clips = {s: R.clip(4 + s % 2 if big else 8 + s % 5, 1000 + s) for s in range(S)}
    refs = {s: R.references(o, c) for s, c in clips.items()}
    probe = S // 2 + 1

    def compare(tag, res):
        compared, ratios = set(), []
        for s in range(S):
            y = res[(s, 0)]
            assert y.shape == clips[s].shape, (tag, s)
            ratios.append(R.rel(y, refs[s][0]) / refs[s][4])
            compared.add(s)
        print(f"{tag}: {len(compared)} slots compared; whole clip vs float64 / emulation's distance: "
              f"min {min(ratios):.2f}, max {max(ratios):.2f} (slot {ratios.index(max(ratios))})")
        bad = [(s, r) for s, r in enumerate(ratios) if r > 2.0 or R.rel(res[(s, 0)], refs[s][0]) < 4e-7]
        assert not bad, (tag, bad[:8])
        assert len(compared) == S

    if name not in ("hg900", "hg320_g2"):
        plan = {s: [(s % 4, clips[s], [s % 4 + 2 + s % 3] if s % 2 else [])] for s in range(S)}
        res = _serve(_inf(m, S), plan, 20)
        compare(f"{name} S {S} pushes", res)
        alone = _serve(_inf(m, 1), {0: plan[probe]}, 20)
        assert torch.equal(alone[(0, 0)], res[(probe, 0)]), "a slot's output depends on its neighbours (pushes)"
    if K:
        assert K <= _bound(ch)
        plan = {s: [(s % 4, clips[s])] for s in range(S)}
        res = _serve_packets(_inf(m, S, max_hops=K), plan, 60, K, seed=5)
        compare(f"{name} S {S} packets of up to {K}", res)
        alone = _serve_packets(_inf(m, 1, max_hops=K), {0: plan[probe]}, 60, K, seed=5 + 100 * probe)
        assert torch.equal(alone[(0, 0)], res[(probe, 0)]), "a slot's output depends on its neighbours (packets)"


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_runs_repeat():
    cfg = R.CONFIGS["small_g2"]
    m = R.gpu_model(R.oracle_model(cfg), cfg)
    clips = torch.stack([R.clip(30, 40 + i) for i in range(20)])              # 20 slots: two row tiles in one pass
    a = stream_all(_inf(m, 20, use_graph=True), clips)
    b = stream_all(_inf(m, 20, use_graph=False), clips)
    c = stream_all(_inf(m, 20, use_graph=True), clips)
    assert torch.equal(a, b) and torch.equal(a, c)
    sizes = even_sizes(30, 4)
    pa = run_packets(_inf(m, 20, use_graph=True, max_hops=4), clips, sizes)
    pb = run_packets(_inf(m, 20, use_graph=False, max_hops=4), clips, sizes)
    pc = run_packets(_inf(m, 20, use_graph=True, max_hops=4), clips, sizes)
    assert torch.equal(pa, pb) and torch.equal(pa, pc)


# ---- 5. f32 untouched --------------------------------------------------------------------------------------------------------------
def test_f32_mode_is_todays_and_the_modes_coexist():
    from cruse_amd.inferencer import StreamingInferencer
    cfg = R.CONFIGS["g4"]
    m = R.gpu_model(R.oracle_model(cfg), cfg)
    clips = torch.stack([R.clip(24, 70 + i) for i in range(3)])
    blocks = clips.view(3, 24, 160).cuda()
    plain = StreamingInferencer(m, 3, max_hops=4)
    named = StreamingInferencer(m, 3, max_hops=4, precision="f32")
    assert plain.precision == "f32" and named.precision == "f32"
    assert not hasattr(named, "gru_pack1_f16") and not hasattr(plain, "gru_pack1_f16")    # nothing new is allocated
    half = _inf(m, 3, max_hops=4)
    half_alone = _inf(m, 3, max_hops=4)
    assert half.precision == "f16"
    for b in range(0, 12):                                                  # pushes, the two modes interleaved in one process
        oa, va = plain.push(blocks[:, b])
        oh, _ = half.push(blocks[:, b])
        ob, vb = named.push(blocks[:, b])
        oh2, _ = half_alone.push(blocks[:, b])
        assert torch.equal(oa, ob) and torch.equal(va, vb) and torch.equal(oh, oh2)
        assert torch.equal(plain.state, named.state) and torch.equal(plain.work, named.work)
    for b in range(12, 24, 4):                                              # then packets
        oa, na = plain.push_packet(blocks[:, b:b + 4])
        oh, _ = half.push_packet(blocks[:, b:b + 4])
        ob, nb = named.push_packet(blocks[:, b:b + 4])
        oh2, _ = half_alone.push_packet(blocks[:, b:b + 4])
        assert torch.equal(oa, ob) and torch.equal(na, nb) and torch.equal(oh, oh2)
        assert torch.equal(plain.state, named.state) and torch.equal(plain.pwork, named.pwork) and torch.equal(plain.gi, named.gi)
        assert not torch.equal(oa, oh)                                      # and the f16 instance really computes something else
    assert torch.equal(plain.flush([0, 1, 2]), named.flush([0, 1, 2]))
    assert torch.equal(half.flush([0, 1, 2]), half_alone.flush([0, 1, 2]))


# ---- 6. mixing, refresh --------------------------------------------------------------------------------------------------------------
def test_push_packet_flush_mixed_on_a_slot():
    cfg = R.CONFIGS["g4"]
    o = R.oracle_model(cfg)
    m = R.gpu_model(o, cfg)
    x = R.clip(90, 21)
    ref64, frames64, _, _, e_emu = R.references(o, x)
    mix = [1, "p", 8, 3, "p", "p", 5, 2, 7, 1, 6, "p", 4, 8, 8, "p", 3, 5, 7, 2, 6, "p", 4, 4]
    assert sum(1 if c == "p" else c for c in mix) == 90
    got = _packet_frames(m, x, 8, mix)                                       # eager: every frame of the mixture but frame 0
    assert [t for _, _, t in got] == list(range(1, 91))
    _check_frames("g4 mixture of push / push_packet", got, frames64)
    inf = _inf(m, 1, max_hops=8)
    _check_clip("g4 mixture of push / push_packet", run_packets(inf, x.view(1, -1), mix)[0], ref64, e_emu)
    _check_clip("g4 the same server, pushes only", stream_all(inf, x.view(1, -1))[0], ref64, e_emu)


def test_refresh_reaches_captured_graphs():
    cfg = R.CONFIGS["small_g2"]
    o = R.oracle_model(cfg)
    m = R.gpu_model(o, cfg)
    x = R.clip(16, 3).view(1, -1)
    inf = _inf(m, 1, max_hops=4)
    before = (stream_all(inf, x), run_packets(inf, x, even_sizes(16, 4)))   # the graphs are captured now
    ptrs = (inf.gru_pack1_f16.data_ptr(), inf.gru_pack2_f16.data_ptr())
    with torch.no_grad():
        for lst in (m.gru.gru_list1, m.gru.gru_list2):
            for gr in lst:
                gr.weight_hh_l0.mul_(0.5)
                gr.weight_ih_l0.mul_(1.25)
    inf.refresh()
    assert ptrs == (inf.gru_pack1_f16.data_ptr(), inf.gru_pack2_f16.data_ptr())           # updated in place
    after = (stream_all(inf, x), run_packets(inf, x, even_sizes(16, 4)))
    fresh = _inf(m, 1, max_hops=4)
    want = (stream_all(fresh, x), run_packets(fresh, x, even_sizes(16, 4)))
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    assert torch.equal(after[0], want[0]) and torch.equal(after[1], want[1])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from cruse_amd import _lib
    from cruse_amd.inferencer import StreamingInferencer
    cfg = R.CONFIGS["small_g2"]
    m = R.gpu_model(R.oracle_model(cfg), cfg)
    with pytest.raises(ValueError, match=r"f32.*f16"):
        StreamingInferencer(m, 1, precision="bf16")
    lib = _lib.lib
    buf = torch.zeros(1 << 16, device="cuda")
    ctl = torch.zeros(64, device="cuda", dtype=torch.int32)
    p16 = torch.zeros(1 << 16, device="cuda", dtype=torch.float16)
    f, i, h = buf.data_ptr(), ctl.data_ptr(), p16.data_ptr()
    for S, Hg in ((1, 18), (1, 1028), (0, 16)):
        rc = lib.cruse_stream_gru_f16(i, S, 1, 1, Hg, f, 4096, 0, None, None, 1e-5, f, 4096, 0, f, h, f, 4096, 0, None)
        assert rc == -1 and b"stream_gru_f16" in lib.cruse_last_error(), (S, Hg, rc)
        rc = lib.cruse_stream_gru_proj_n_f16(i, S, 2, 3, 1, 1, Hg, f, 4096, 0, None, None, 1e-5, f, h, f, None)
        assert rc == -1 and b"stream_gru_proj_n_f16" in lib.cruse_last_error(), (S, Hg, rc)
        rc = lib.cruse_stream_gru_rec_n_f16(i, S, 2, 3, 0, 1, Hg, f, f, 4096, 0, f, h, f, 4096, 0, None)
        assert rc == -1 and b"stream_gru_rec_n_f16" in lib.cruse_last_error(), (S, Hg, rc)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                    # nothing was launched


def test_offsets_that_leave_a_row_are_refused():
    """f32 and f16 forms alike: S = 1, g = 1, Hg = 4 in rows of 8 floats; an offset of 6 leaves the row"""
    from cruse_amd import _lib
    lib = _lib.lib
    buf = torch.zeros(1 << 12, device="cuda")
    ctl = torch.zeros(64, device="cuda", dtype=torch.int32)
    p16 = torch.zeros(1 << 12, device="cuda", dtype=torch.float16)
    f, i, h = buf.data_ptr(), ctl.data_ptr(), p16.data_ptr()
    for p16_arg, who in (((), b"stream_gru"), ((h,), b"stream_gru_f16")):
        step = lib.cruse_stream_gru_f16 if p16_arg else lib.cruse_stream_gru
        rec = lib.cruse_stream_gru_rec_n_f16 if p16_arg else lib.cruse_stream_gru_rec_n
        for x_off, h_off, o_off in ((6, 0, 0), (0, 6, 0), (0, 0, 6)):
            rc = step(i, 1, 1, 1, 4, f, 8, x_off, None, None, 1e-5, f, 8, h_off, f, *p16_arg, f, 8, o_off, None)
            msg = lib.cruse_last_error()
            assert rc == -1 and who + b":" in msg and b"outside rows of 8 / 8 / 8" in msg, (who, x_off, h_off, o_off, rc, msg)
        rc = rec(i, 1, 1, 2, 0, 1, 4, f, f, 8, 0, f, *p16_arg, f, 8, 6, None)          # h_off past the work row
        msg = lib.cruse_last_error()
        assert rc == -1 and who.replace(b"gru", b"gru_rec_n") + b":" in msg and b"outside a state row of 8 / work row of 8" in msg, (who, rc, msg)
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                    # refused before any launch


# ---- 8. bounds --------------------------------------------------------------------------------------------------------------------------
def test_f16_chains_under_the_guard_allocator():
    """tools/engine_guard_run.py tools/guard_stream_f16.py, once, in a subprocess under a time limit: the f16 chains at one and three slots
    for three models with every tensor end-aligned in its own allocation, outputs compared with the emulation"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "engine_guard_run.py"), os.path.join(ROOT, "tools", "guard_stream_f16.py")],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode(errors="replace")
    lines = out.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1].startswith("guard stream f16 ok"), out[-3000:]
