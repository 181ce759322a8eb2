"""GPU: cruse_assemble_clips captured into a HIP graph and replayed equals the eager call.

A file of its own, sorted behind tests/test_gpu_engines_coexist.py on purpose.  Instantiating a graph makes the runtime create streams
of its own, which moves every later stream of the process to another hardware queue; that test times six engines against each other
across exactly such shifts with a 10 % bound, and with one more instantiation in front of it its fourth graph-form engine came out
12 % slow, twice in two whole-suite runs, and within 2 % when the file ran without it.  The engine's choice of a launch stream
(TrainEngine._pick_launch_stream) is what that test guards and is not touched here; this capture simply happens after it, as the
captures of tests/test_gpu_fftconv.py and tests/test_gpu_resample.py do."""
import pytest
import torch

from test_gpu_assemble import CASES, assemble

pytestmark = pytest.mark.gpu


def test_graph_replay_equals_eager():
    seg, first, L = CASES["three clips of 4099"]
    assert torch.equal(assemble(seg, first, L, graph=True), assemble(seg, first, L))
