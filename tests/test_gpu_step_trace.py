"""MI355X: the training step makes the calls into libcruse_hip.so that the commit before the step plan (cruse_amd/model/step_plan.py) made.

For every case of tests/step_trace.py -- the default bf16 step at 1 / 2 / 4 GRU groups, f32 and bf16x3, every EngineConfig switch of the step
alone, the f16 gi rows, the other losses, eval_loss, the bucketed schedule, the upsample decoder, odd channel counts and the nn.Module
surfaces -- one eager step (TrainEngine(use_graph=False, lr=0.0), or module(x).sum().backward()) runs with every entry point of
_lib.SIGNATURES wrapped, and the whole list of records (entry, scalar arguments verbatim, null / equality pattern of the pointer arguments,
ordinal of the stream) must equal the recorded one: no record is skipped.  The mask's sha256 and the loss as a hex float are pinned with it
(both are bit-stable; gradients are not hashed, BatchNorm-sum atomics reorder from run to run).  The narrow_ch case (Hg = 80) is a step
the recurrence refuses: its calls up to the refusal and the message are what is pinned.

tests/golden/step_trace_parent.json was recorded from the PARENT of the commit that added the plan, never from the code under test: check
that parent out into a scratch worktree, build it, copy tests/step_trace.py there (its docstring names the three privates it touches besides the public API)
and run `python tests/step_trace.py step_trace_parent.json` on an MI355X; it runs the case list twice and fails unless both passes agree.
The file holds each distinct record once and one index list per case.  A change that moves a launch on purpose re-records it the same way,
from the commit before that change plus the intended difference reviewed by hand."""
import functools
import json
import os

import pytest

from step_trace import CASES, run_case

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_trace_parent.json")) as f:
        return json.load(f)


def test_golden_holds_exactly_the_case_list():
    assert list(golden()["cases"]) == list(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_step_makes_the_parents_calls(name):
    want = golden()["cases"][name]
    got = run_case(name)
    print(name, len(got["trace"]), "calls", got["mask_sha256"], got["loss"], got["error"])
    records = golden()["records"]
    want_trace = [records[i] for i in want["trace"]]
    for n, (a, b) in enumerate(zip(got["trace"], want_trace)):
        assert a == b, f"{name}: call {n} is {a}, the parent made {b}"
    assert len(got["trace"]) == len(want_trace), (name, len(got["trace"]), len(want_trace))
    assert got["error"] == want["error"]
    assert got["mask_sha256"] == want["mask_sha256"]
    assert got["loss"] == want["loss"]
