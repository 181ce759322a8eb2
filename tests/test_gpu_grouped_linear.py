"""GPU: the grouped-linear and band kernels against float64 einsum / dense products, the modules on them against
the reference's own outputs (fixture G24, tests/golden/make_golden_squeezed.py) and, for gradients, against tests/squeezed_ref.py.

Bars (rel-L2), the project's own for the exact-f32 MFMA route (tests/test_gpu_extras.py, GroupGRU): forward and states < 1e-5, input
gradient < 5e-4, parameter gradients < 2e-3; band_pool / band_expand do f32 adds and one multiply: < 1e-6."""
import numpy as np
import pytest
import torch
from torch import nn

import squeezed_ref as R

pytestmark = pytest.mark.gpu

FWD, DX, DW, BAND = 1e-5, 5e-4, 2e-3, 1e-6
DEV = "cuda"

# (rows, G, Ig, Hg): widths below and off the 16-wide tile; equal widths over more than one 64-row block; one column per group;
# Hg above one 64-wide tile with a partial last row tile and a weight gradient split over 5 row parts; a single row
SHAPES = {"odd": (21, 8, 12, 5), "equal": (130, 8, 8, 8), "one_col": (67, 4, 1, 3), "wide": (1100, 1, 96, 80), "row1": (1, 2, 20, 36)}


@pytest.fixture(scope="module")
def g24(golden):
    return golden("g24_squeezed.npz")


def _case(name):
    rows, G, Ig, Hg = SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(rows, G * Ig, generator=g, dtype=torch.float64)
    w = torch.randn(G, Ig, Hg, generator=g, dtype=torch.float64) / Ig ** 0.5
    b = torch.randn(G * Hg, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, G * Hg, generator=g, dtype=torch.float64)
    return x, w, b, dy


@pytest.mark.parametrize("layout", ("gih", "ghi"))
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernels_against_einsum(name, layout):
    from cruse_amd import ops
    x, w, b, dy = _case(name)
    G = w.shape[0]
    xd, dyd = x.float().to(DEV), dy.float().to(DEV)
    wd = (w if layout == "gih" else w.transpose(1, 2)).float().contiguous().to(DEV)
    for bias in (True, False):
        for relu in (True, False):
            for shuffle in (True, False):
                tag = f"{name} {layout} bias={bias} relu={relu} shuffle={shuffle}"
                xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
                yr = R.grouped_linear(xr, wr, br if bias else None, relu, shuffle)
                yr.backward(dy)
                bd = b.float().to(DEV) if bias else None
                y = ops.grouped_linear(xd, wd, layout, bd, relu, shuffle)
                dx = ops.grouped_linear_bwd_dx(dyd, wd, layout, y if relu else None, shuffle)
                dw, db = ops.grouped_linear_bwd_dw(dyd, xd, tuple(wd.shape), layout, y if relu else None, shuffle, want_db=bias)
                torch.cuda.synchronize()
                if layout == "ghi":
                    dw = dw.transpose(1, 2)
                errs = {"y": R.rel_l2(y, yr), "dx": R.rel_l2(dx, xr.grad), "dw": R.rel_l2(dw, wr.grad)}
                if bias:
                    errs["db"] = R.rel_l2(db, br.grad)
                print(tag, errs)
                assert tuple(y.shape) == tuple(yr.shape) and tuple(dw.shape) == tuple(w.shape)
                assert errs["y"] < FWD and errs["dx"] < DX and errs["dw"] < DW and errs.get("db", 0.0) < DW, (tag, errs)
                assert (db is None) == (not bias)
    assert G == SHAPES[name][1]


def test_autograd_function_saves_nothing_without_grad():
    from cruse_amd import ops
    x, w, b, _ = _case("odd")
    xd, wd, bd = x.float().to(DEV), w.float().to(DEV), b.float().to(DEV)
    y = ops.GroupedLinearFn.apply(xd, wd, bd, "gih", True, False)
    assert y.grad_fn is None and not y.requires_grad
    wq = wd.clone().requires_grad_()
    y = ops.GroupedLinearFn.apply(xd, wq, bd, "gih", False, False)
    x_s, w_s, y_s = y.grad_fn.saved_tensors
    assert x_s is not None and w_s is None and y_s is None          # weight gradient alone: x, neither w nor the ReLU mask


def test_guard_placement_gives_the_same_values():
    """every operand and result is the tail of its own buffer (its last element is the buffer's last, its base is off the 16-byte grid):
    values must be those of the normal placement, bit for bit"""
    from cruse_amd import ops
    from cruse_amd._lib import check, lib
    x, w, b, dy = _case("odd")
    rows, G, Ig, Hg = SHAPES["odd"]

    def tail(t, extra):
        buf = torch.full((t.numel() + extra,), float("nan"), device=DEV, dtype=torch.float32)
        v = buf[extra:].view(t.shape)
        v.copy_(t)
        return v

    xd, wd, bd, dyd = (t.float().to(DEV) for t in (x, w, b, dy))
    y0 = ops.grouped_linear(xd, wd, "gih", bd, True, True)
    dx0 = ops.grouped_linear_bwd_dx(dyd, wd, "gih", y0, True)
    dw0, db0 = ops.grouped_linear_bwd_dw(dyd, xd, tuple(wd.shape), "gih", y0, True, want_db=True)
    xt, wt, bt, dyt = tail(xd, 3), tail(wd, 1), tail(bd, 5), tail(dyd, 7)
    yt, dxt, dwt, dbt = tail(torch.zeros_like(y0), 1), tail(torch.zeros_like(dx0), 3), tail(torch.zeros_like(dw0), 5), tail(torch.zeros_like(db0), 7)
    s = torch.cuda.current_stream().cuda_stream
    sg, si, so = Ig * Hg, Hg, 1
    check(lib.cruse_grouped_linear_fwd(xt.data_ptr(), wt.data_ptr(), sg, si, so, bt.data_ptr(), rows, G, Ig, Hg, 1, 1, yt.data_ptr(), s))
    check(lib.cruse_grouped_linear_bwd_dx(dyt.data_ptr(), yt.data_ptr(), wt.data_ptr(), sg, si, so, rows, G, Ig, Hg, 1, 1, dxt.data_ptr(), s))
    check(lib.cruse_grouped_linear_bwd_dw(dyt.data_ptr(), yt.data_ptr(), xt.data_ptr(), rows, G, Ig, Hg, 1, 1, dwt.data_ptr(), sg, si, so,
                                          dbt.data_ptr(), None, 0, s))
    torch.cuda.synchronize()
    for a, c in ((yt, y0), (dxt, dx0), (dwt, dw0), (dbt, db0)):
        assert torch.equal(a, c)


# ---- modules against the reference's outputs --------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def test_grouped_linear_einsum_module(g24):
    from model.based_model.cust_conv import GroupedLinearEinsum
    m = GroupedLinearEinsum(96, 64, 8).to(DEV)
    m.load_state_dict({"weight": _t(g24["gle/weight"])})
    y = m(_t(g24["x"]))
    assert tuple(y.shape) == (3, 7, 64) and R.rel_l2(y, torch.from_numpy(g24["gle/y"])) < FWD


@pytest.mark.parametrize("name", ("gl_shuffle", "gl_cat"))
def test_grouped_linear_module(g24, name):
    from model.based_model.cust_conv import GroupedLinear
    m = GroupedLinear(96, 40, 8, shuffle=name == "gl_shuffle").to(DEV)
    sd = {}
    for i in range(8):
        sd[f"layers.{i}.weight"], sd[f"layers.{i}.bias"] = _t(g24[f"{name}/weight"][i]), _t(g24[f"{name}/bias"][i])
    m.load_state_dict(sd)
    x = _t(g24["x"]).requires_grad_()
    y = m(x)
    y4 = m(_t(g24["x4"]))                                             # 4-D input [2, 3, 5, 96]
    assert tuple(y4.shape) == (2, 3, 5, 40)
    assert R.rel_l2(y, torch.from_numpy(g24[f"{name}/y"])) < FWD and R.rel_l2(y4, torch.from_numpy(g24[f"{name}/y4"])) < FWD
    # gradients reach the nn.Linear parameters: against stock torch on the CPU
    ref = nn.ModuleList(nn.Linear(12, 5) for _ in range(8)).double()
    ref.load_state_dict({k[len("layers."):]: v.double().cpu() for k, v in sd.items()})
    xr = torch.from_numpy(g24["x"]).double().requires_grad_()
    yr = torch.cat([l(xr[..., 12 * i:12 * (i + 1)]) for i, l in enumerate(ref)], dim=-1)
    if m.shuffle:
        yr = R.shuffle_columns(yr, 8)
    dy = torch.randn(3, 7, 40, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    yr.backward(dy)
    y.backward(dy.float().to(DEV))
    assert R.rel_l2(x.grad, xr.grad) < DX
    for i in range(8):
        assert R.rel_l2(m.layers[i].weight.grad, ref[i].weight.grad) < DW and R.rel_l2(m.layers[i].bias.grad, ref[i].bias.grad) < DW


def _squeezed(name):
    from model.based_model.cust_conv import SqueezedGRU, SqueezedGRU_S
    kw = {
        "sq2": dict(output_size=40, num_layers=2, linear_groups=8, gru_skip_op=nn.Identity, linear_act_layer=nn.ReLU),
        "sqs": dict(output_size=96, num_layers=1, gru_skip_op=nn.Identity),
        "sq_noout": dict(output_size=None),
        "sq_tmajor": dict(output_size=40, num_layers=2, linear_groups=8, batch_first=False, gru_skip_op=nn.Identity, linear_act_layer=nn.ReLU),
        "sq_tanh": dict(output_size=40, gru_skip_op=nn.Identity, linear_act_layer=nn.Tanh),
    }[name]
    late = name == "sqs"
    return (SqueezedGRU_S if late else SqueezedGRU)(96, 64, **kw), R.Squeezed(96, 64, late_skip=late, **kw).double()


@pytest.mark.parametrize("name", ("sq2", "sqs", "sq_noout", "sq_tmajor", "sq_tanh"))
def test_squeezed_gru(g24, name):
    m, ref = _squeezed(name)
    src = "sq2" if name == "sq_tmajor" else name
    sd = {k[len(src) + 4:]: torch.from_numpy(g24[k]) for k in g24.files if k.startswith(src + "/sd/")}
    m.load_state_dict(sd)
    ref.load_state_dict({k: v.double() for k, v in sd.items()})
    m = m.to(DEV)
    x = torch.from_numpy(g24["x"])
    if name == "sq_tmajor":
        x = x.transpose(0, 1).contiguous()
    h0 = torch.from_numpy(g24[f"{name}/h0"])
    L = h0.shape[0]
    want = {k: torch.from_numpy(g24[f"{name}/{k}"]) for k in ("y", "h", "y_h0", "h_h0")}
    # no state, a zero state, a non-zero state: outputs and final states against the reference's own
    for state, ky, kh in ((None, "y", "h"), (torch.zeros_like(h0), "y", "h"), (h0, "y_h0", "h_h0")):
        y, h = m(x.to(DEV), None if state is None else state.to(DEV))
        assert tuple(y.shape) == tuple(want[ky].shape) and tuple(h.shape) == (L, 3, 64)
        ey, eh = R.rel_l2(y, want[ky]), R.rel_l2(h, want[kh])
        print(name, "state", None if state is None else float(state.abs().max()), ey, eh)
        assert ey < FWD and eh < FWD, (name, ey, eh)
    # gradients from the non-zero state, against stock torch (float64) -- the state itself gets none here (it is detached)
    xg = x.to(DEV).requires_grad_()
    hg = h0.to(DEV).requires_grad_()
    y, h = m(xg, hg)
    g = torch.Generator().manual_seed(9)
    dy, dh = torch.randn(y.shape, generator=g, dtype=torch.float64), torch.randn(h.shape, generator=g, dtype=torch.float64)
    (y * dy.float().to(DEV)).sum().add((h * dh.float().to(DEV)).sum()).backward()
    xr = x.double().requires_grad_()
    yr, hr = ref(xr, h0.double())
    ((yr * dy).sum() + (hr * dh).sum()).backward()
    assert hg.grad is None
    assert R.rel_l2(xg.grad, xr.grad) < DX, R.rel_l2(xg.grad, xr.grad)
    grads = dict(ref.named_parameters())
    for k, p in m.named_parameters():
        e = R.rel_l2(p.grad, grads[k].grad)
        print(name, k, e)
        assert e < DW, (name, k, e)


def test_squeezed_gru_refuses_hidden_48():
    from model.based_model.cust_conv import SqueezedGRU
    with pytest.raises(RuntimeError, match="multiple of 32"):
        SqueezedGRU(96, 48)


def _sq2_on_device(g24):
    m, _ = _squeezed("sq2")
    m.load_state_dict({k[len("sq2/sd/"):]: torch.from_numpy(g24[k]) for k in g24.files if k.startswith("sq2/sd/")})
    return m.to(DEV), torch.from_numpy(g24["x"]).to(DEV), torch.from_numpy(g24["sq2/h0"]).to(DEV)


def test_squeezed_gru_is_deterministic(g24):
    m, x, h0 = _sq2_on_device(g24)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_()
        y, h = m(xg, h0)
        (y.square().sum() + h.sum()).backward()
        runs.append([y.detach(), h.detach(), xg.grad] + [p.grad.clone() for p in m.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_squeezed_gru_forward_captures_into_a_graph(g24):
    m, x, h0 = _sq2_on_device(g24)
    with torch.no_grad():
        y0, hn0 = m(x, h0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x, h0)                                                  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y, hn = m(x, h0)
        for _ in range(2):
            y.zero_(); hn.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, y0) and torch.equal(hn, hn0)


# ---- ERB bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (1, 5, 403))
@pytest.mark.parametrize("i", range(3))
def test_erb_apply_against_the_dense_product(g24, i, rows):
    from model.based_model.cust_conv import erb_apply, erb_apply_inverse
    width = g24[f"erb/{i}/width"].astype(int)
    F, nb = int(width.sum()), len(width)
    g = torch.Generator().manual_seed(100 * i + rows)
    x = torch.randn(rows, F, generator=g, dtype=torch.float64)
    mb = torch.randn(rows, nb, generator=g, dtype=torch.float64)
    for normalized in (True, False):
        fb = torch.from_numpy(g24[f"erb/{i}/fb_n{int(normalized)}_i0"]).double()
        fbi = torch.from_numpy(g24[f"erb/{i}/fb_n{int(normalized)}_i1"]).double()
        xr, mr = x.clone().requires_grad_(), mb.clone().requires_grad_()
        yr, zr = xr @ fb, mr @ fbi
        dy, dz = torch.randn(yr.shape, generator=g, dtype=torch.float64), torch.randn(zr.shape, generator=g, dtype=torch.float64)
        yr.backward(dy); zr.backward(dz)
        xd, md = x.float().to(DEV).requires_grad_(), mb.float().to(DEV).requires_grad_()
        y, z = erb_apply(xd, width, normalized), erb_apply_inverse(md, width, normalized)
        y.backward(dy.float().to(DEV)); z.backward(dz.float().to(DEV))
        errs = [R.rel_l2(y, yr), R.rel_l2(z, zr), R.rel_l2(xd.grad, xr.grad), R.rel_l2(md.grad, mr.grad)]
        print(i, rows, normalized, errs)
        assert tuple(y.shape) == (rows, nb) and tuple(z.shape) == (rows, F) and max(errs) < BAND, errs
    # inverse(apply(x)) at normalized=True: every bin holds the mean of its band
    xd = x.float().to(DEV)
    back = erb_apply_inverse(erb_apply(xd, width, True), width, True).cpu().double()
    edges = np.concatenate([[0], np.cumsum(width)])
    means = torch.cat([x[:, a:b].mean(dim=1, keepdim=True).expand(-1, b - a) for a, b in zip(edges[:-1], edges[1:])], dim=1)
    assert R.rel_l2(back, means) < BAND


def test_erb_apply_keeps_leading_dimensions(g24):
    from model.based_model.cust_conv import erb_apply, erb_apply_inverse
    width = g24["erb/0/width"].astype(int)
    x = torch.randn(2, 3, 5, 161, device=DEV)
    y = erb_apply(x, width)
    assert tuple(y.shape) == (2, 3, 5, 32) and tuple(erb_apply_inverse(y, width).shape) == (2, 3, 5, 161)
    with pytest.raises(RuntimeError):
        erb_apply(x[..., :160].contiguous(), width)
