"""Launch traces of the training step: every call the host makes into libcruse_hip.so, written down without addresses.

record(fn) runs fn() with every entry point of `_lib.SIGNATURES` wrapped on `ops.lib` and returns one record per call:
[name, arg, arg, ...] where an integer or string argument stands verbatim, a float as "f" + repr, a pointer as "p" + the position of the
first pointer argument of THIS call holding the same address ("p-1": null) and the trailing stream as "s" + the ordinal of that stream's
first appearance in the trace.  Addresses are not compared across calls: the caching allocator may hand out other blocks once the lifetime
of a temporary moves.  CASES is the matrix tests/test_gpu_step_trace.py pins against tests/golden/step_trace_parent.json; run_case(name)
-> the records, the sha256 of the returned mask's bytes and the loss as a hex float.  Besides the public engine / module API the file
touches three privates, all present on the commit the golden is recorded from, where it runs unchanged (python tests/step_trace.py OUT.json):
ops._CONV_FN (the conv entry points bound at import), TrainEngine._last_mask, and -- module cases only -- torch.zeros_like, patched while the
step runs (see run_case).  A refused step (narrow_ch) leaves its queued leaves in that case's OWN engine scheduler: no other case sees them.
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

CH, F0, B0, L0 = (1, 8, 16, 32, 64), 160, 8, 3200          # the narrowest net on which the MFMA and fused paths are eligible; T = 21


def _addr(a) -> int:
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, ctypes._SimpleCData):
        return a.value or 0
    try:
        return ctypes.addressof(a)
    except TypeError:
        return id(a)                      # byref(...): some host address, non-null and its own


def record(fn) -> list:
    from cruse_amd import _lib, ops
    trace, streams = [], {}

    def spy(name, kinds, real):
        def call(*args):
            rec, first = [name], {}
            stream_at = len(args) - 1 if kinds.endswith("p") and _addr(args[-1]) == (torch.cuda.current_stream().cuda_stream or 0) else -1
            for i, (k, a) in enumerate(zip(kinds, args)):
                if i == stream_at:
                    rec.append(f"s{streams.setdefault(_addr(a), len(streams))}")
                elif k == "p":
                    v = _addr(a)
                    rec.append(f"p{first.setdefault(v, i) if v else -1}")
                elif k in "fd":
                    rec.append("f" + repr(float(a)))
                elif k == "c":
                    rec.append(a.decode() if isinstance(a, bytes) else str(a))
                else:
                    rec.append(int(a))
            trace.append(rec)
            return real(*args)
        return call

    with pytest.MonkeyPatch.context() as mp:
        wrapped = {}
        for name, (kinds, _) in _lib.SIGNATURES.items():
            real = getattr(ops.lib, name)
            wrapped[id(real)] = spy(name, kinds, real)
            mp.setattr(ops.lib, name, wrapped[id(real)])
        # (the conv wrappers of ops.py hold their entry points in a table bound at import)
        mp.setattr(ops, "_CONV_FN", tuple(tuple(wrapped.get(id(f), f) for f in row) for row in ops._CONV_FN))
        fn()
        torch.cuda.synchronize()
    return trace


def _gi16_batch() -> int:
    """a batch the f16-gi recurrence serves (chains of 8 clips): B0 if it does, else the smallest"""
    from cruse_amd import ops
    for B in [B0] + list(range(1, 65)):
        if ops.gru_plan(B, 1, 640, "bf16")["clips_per_chain"] == 8:
            return B
    raise RuntimeError("no batch up to 64 runs chains of 8 clips")


def _cases() -> dict:
    c = {}
    for g in (1, 2, 4):
        c[f"bf16_g{g}"] = dict(groups=g)
    for prec in ("f32", "bf16x3"):
        for g in (1, 4):
            c[f"{prec}_g{g}"] = dict(groups=g, prec=prec)
    for knob in ("fuse_bn_fwd", "fuse_bn_stats", "fuse_bn_bwd_stats", "fuse_bn_bwd_apply", "bf16_dy", "bf16_de", "dx_atr", "fuse_mask_head",
                 "overlap"):
        c[f"{knob}_off"] = dict(cfg={knob: False})
    for knob, values in (("gi_f16", (0, 3)), ("gi_x3", (0, 7)), ("defer_mask", (0,)), ("inline_mask", (0, 31))):
        for v in values:
            c[f"{knob}_{v}"] = dict(cfg={knob: v})
    c["gi_store_f16"] = dict(cfg={"gi_store_f16": True}, B="gi16")
    for loss in ("si_snr", "sdnr", "wo_male_df"):
        c[f"loss_{loss}"] = dict(loss=loss)
    c["eval_loss"] = dict(kind="eval")
    c["bucketed"] = dict(bucketed=True)
    c["upsample_module"] = dict(kind="upsample")
    c["narrow_ch"] = dict(ch=(1, 3, 5, 6, 8))           # Hg = 80: the recurrence refuses it (Hg % 32 != 0) -- the calls up to the refusal and its text
    c["odd_ch"] = dict(ch=(1, 3, 5, 6, 32))             # ... and a whole step on the VALU convs and weight gradients (all_mfma false), Hg = 320
    c["unet_2_module"] = dict(kind="module")
    c["ggru_module"] = dict(kind="ggru")
    return c


CASES = _cases()


def run_case(name: str):
    """-> dict(trace, mask_sha256 of the mask / module output, loss / output sum as a hex float, error) of the SECOND step: the first one
    sets up workspaces, LDS attributes and the side-stream choice, whose own launches are no part of a step.  A step the library refuses
    (RuntimeError) leaves the calls up to the refusal and its message in `error`."""
    from cruse_amd.config import EngineConfig
    from cruse_amd.data import synth_batch
    from cruse_amd.engine import TrainEngine
    from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
    from cruse_amd.model.cruse_net import GGRU, unet_2
    spec = CASES[name]
    kind, prec, g, ch = spec.get("kind", "step"), spec.get("prec", "bf16"), spec.get("groups", 1), spec.get("ch", CH)
    B = _gi16_batch() if spec.get("B") == "gi16" else B0
    torch.manual_seed(3)
    out = {}
    if kind in ("step", "eval"):
        eng = TrainEngine(unet_2(ch=ch, rnn_groups=g, precision=prec).cuda(), use_graph=False, lr=0.0, loss=spec.get("loss", "wo_male"),
                          bucketed=spec.get("bucketed"), config=EngineConfig(**spec.get("cfg", {})))
        noisy, clean = synth_batch(B, L0, "cuda", 50)

        def fn():
            if kind == "eval":
                out["loss"] = eng.eval_loss(noisy, clean)
            else:
                out["loss"] = eng.loss_value(eng.step(noisy, clean))
            out["mask"] = eng._last_mask
    else:
        T = L0 // 160 + 1
        if kind == "ggru":
            mod = GGRU(hidden_size=640, groups=1, precision=prec).cuda()
            x = torch.randn(B, 64, T, 10, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_()
        else:
            mod = (CRUSE4MagAddSkipUpsample if kind == "upsample" else unet_2)(ch=ch, rnn_groups=g, precision=prec).cuda()
            x = torch.rand(B, 1, T, F0, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_()

        n_par, zeros_like = sum(p.numel() for p in mod.parameters()), torch.zeros_like

        def fn():
            # The backward pass tests whether dW_hh follows dW_ih in memory (one concatenated launch if so).  The autograd glue makes its
            # gradient tensors with zeros_like, so where they land is the caching allocator's business: here they are carved from ONE
            # buffer in the order they are asked for (as FlatParams lays out the engine's), so that the test does not depend on it.
            flat, used = torch.zeros(n_par, device="cuda"), [0]

            def carve(t, **kw):
                o, n = used[0], t.numel()
                if kw or not t.is_cuda or t.dtype != torch.float32 or o + n > n_par:
                    return zeros_like(t, **kw)
                used[0] = o + n
                return flat[o:o + n].view(t.shape)
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(torch, "zeros_like", carve)
                mod.zero_grad()
                y = mod(x)
                y.sum().backward()
            out["mask"], out["loss"] = y.detach(), float(y.detach().double().sum())

    def guarded():
        out.clear()
        try:
            fn()
        except RuntimeError as ex:
            out["error"] = str(ex)
    guarded()
    torch.cuda.synchronize()
    trace = record(guarded)
    if "error" in out:
        return dict(trace=trace, mask_sha256=None, loss=None, error=out["error"])
    return dict(trace=trace, mask_sha256=hashlib.sha256(out["mask"].detach().contiguous().float().cpu().numpy().tobytes()).hexdigest(),
                loss=float(out["loss"]).hex(), error=None)


def pack(results: dict) -> dict:
    """{case: run_case result} -> distinct records once, one index list per case"""
    index, records, cases = {}, [], {}
    for name, res in results.items():
        idx = []
        for rec in res["trace"]:
            key = json.dumps(rec)
            if key not in index:
                index[key] = len(records)
                records.append(rec)
            idx.append(index[key])
        cases[name] = dict(res, trace=idx)
    return dict(records=records, cases=cases)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    results = {name: run_case(name) for name in CASES}
    again = {name: run_case(name) for name in CASES}             # the recording is only worth pinning if the commit repeats itself
    unstable = [name for name in CASES if results[name] != again[name]]
    with open(sys.argv[1], "w") as f:
        json.dump(pack(results), f, separators=(",", ":"))
    calls = sum(len(r["trace"]) for r in results.values())
    print(f"{len(CASES)} cases, {calls} calls; not repeatable: {unstable}")
    sys.exit(1 if unstable else 0)
