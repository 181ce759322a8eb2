"""MI355X: cruse_stream_boundary_plan and the launches agree about acceptance on a real device.  A short clip goes through StreamingInferencer
in each of the eight decode forms ({transposed, upsample} x {plain, pcm_out + atten_lim, post_filter, all three}), pushes and packets mixed; every
call the server makes to a boundary entry point is written down with its arguments, must be accepted by the entry point (the launch included:
cruse_ensure_dyn_lds raised no objection) and by ops.stream_boundary_plan with the same arguments, and the plan's instance must be the one the form
asks for.  The numerical bars of these forms are where they were, in the test files of each form."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(ch=(1, 3, 5, 6, 8), rnn_groups=1)
S, K, HOP = 3, 2, 160
FORMS = {"plain": {}, "pcm_lim": dict(pcm_out=True, atten_lim=True), "pf": dict(post_filter="iam"),
         "all": dict(pcm_out=True, atten_lim=True, post_filter="iam")}
SUFFIX = {"plain": "", "pcm_lim": "_io", "pf": "_pf", "all": "_pf"}


@functools.lru_cache(maxsize=None)
def model(decoder):
    """the product module with its initial weights (nothing here depends on their values) -- built once, shared, never modified"""
    from cruse_amd.model.cruse import CRUSE4MagAddSkipUpsample
    from cruse_amd.model.cruse_net import unet_2
    torch.manual_seed(3)
    return (CRUSE4MagAddSkipUpsample if decoder == "upsample" else unet_2)(precision="f32", **CFG).cuda().eval()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("decoder", ["transposed", "upsample"])
def test_plan_accepts_what_the_server_launches(decoder, form, monkeypatch):
    from cruse_amd import ops
    from cruse_amd.inferencer import StreamingInferencer
    calls = []

    def spy(entry):
        fn = getattr(ops.lib, f"cruse_stream_{entry}")

        def call(*args):
            rc = fn(*args)
            calls.append((entry, args[:-1], rc))
            return rc
        return call

    for entry in ops.STREAM_BOUNDARY_ENTRIES:
        monkeypatch.setattr(ops.lib, f"cruse_stream_{entry}", spy(entry))
    kw = FORMS[form]
    inf = StreamingInferencer(model(decoder), S, decoder=decoder, use_graph=False, max_hops=K, **kw)
    if "atten_lim" in kw:
        inf.set_atten_lim(12.0)
    if "post_filter" in kw:
        inf.set_post_filter(0.02)
    x = 0.1 * torch.randn(S, 4 * HOP, generator=torch.Generator().manual_seed(1)).cuda()
    inf.push(x[:, :HOP])                                   # block 0: stored
    inf.push(x[:, HOP:2 * HOP])                            # frame 0 and frame 1: two chains
    inf.push_packet(x[:, 2 * HOP:].reshape(S, K, HOP))     # two frames in one packet
    inf.flush(list(range(S)))                              # the end frame
    torch.cuda.synchronize()
    suffix = "_up" if decoder == "upsample" else SUFFIX[form]
    assert {c[0] for c in calls} == {"encode", "encode_n", "decode" + suffix, "decode_n" + suffix}, {c[0] for c in calls}
    # the device's LDS limit is known to the library only as cruse_ensure_dyn_lds's refusal: rc == 0 of the real call says that the bytes
    # it asked for -- plan["lds_bytes"], computed by the same function from the same arguments -- were within it
    for entry, args, rc in calls:
        assert rc == 0, (entry, rc, ops.lib.cruse_last_error())
        plan = ops.stream_boundary_plan(entry, *args)       # raises where the plan refuses
        assert plan["grid"] == S and 0 < plan["lds_bytes"], (entry, plan)
        if entry.startswith("decode"):
            assert (plan["dec"], plan["s16"], plan["lim"], plan["pf"]) == (int(decoder == "upsample"), int("pcm_out" in kw), int("atten_lim" in kw),
                                                                           int("post_filter" in kw)), (entry, plan)
            assert plan["family"] == (3 if "_n" in entry else 2)
        else:
            assert plan["raw"][:5] == [int("_n" in entry), 0, 0, 0, 0], (entry, plan)
