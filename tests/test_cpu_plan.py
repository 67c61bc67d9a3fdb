"""premvos_amd.plan: the launch-plan bookkeeping the four nets share (host logic; descriptors and packed weights on CPU tensors,
the launch functions replaced by recording fakes -- the HIP library is never loaded)."""
import pytest
import torch

from premvos_amd import _lib, arena, ops
from premvos_amd.ops import ACT_RELU, NHWC
from premvos_amd.plan import LaunchPlan

CPU = torch.device("cpu")


@pytest.fixture
def launches(monkeypatch):
    """Record every conv launch instead of running it; loading the library fails the test."""
    calls = []

    def no_lib():
        raise AssertionError("the plan bookkeeping must not load the HIP library")

    monkeypatch.setattr(_lib, "load", no_lib)
    monkeypatch.setattr(ops, "run_desc", lambda d, stream=None: calls.append(("fp32", d)))
    monkeypatch.setattr(ops, "run_s8", lambda d, x, pk, out_s8, tile=None, stream=None, res_s8=None:
                        calls.append(("s8", d, x, pk, out_s8, res_s8)))
    return calls


def _weights(cout, cin, k, seed=0):
    return torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(seed))


def test_fp32_conv_is_tuned_and_s8_conv_is_not(launches):
    pk = ops.pack_conv(_weights(32, 16, 3), None, CPU)
    pk8 = ops.pack_conv_s8(_weights(64, 32, 1, 1), None, CPU)
    x, y = NHWC.alloc(2, 8, 12, 16, CPU), NHWC.alloc(2, 8, 12, 32, CPU)
    x8, y8, r8 = (NHWC.alloc_s8(2, 8, 12, c, CPU) for c in (32, 64, 64))
    p = LaunchPlan()
    d = p.conv("a", x, pk, y, pad=(1, 1), act=ACT_RELU)
    assert p.descs == [d] and p.tune_descs == [d] and p.split_layers == 0 and d.tile_hint == 0
    d8 = p.conv("b", x8, pk8, None, out_s8=y8, res_s8=r8)
    assert p.descs == [d, d8] and p.tune_descs == [d] and p.split_layers == 1
    assert d8.tile_hint == ops.S8_HINT and d8.precision == _lib.PREC_BF16X3
    with pytest.raises(AssertionError):              # an fp32 input has no S8 output or residual
        p.conv("c", x, pk, y, out_s8=y8, pad=(1, 1))
    assert len(p.steps) == 2
    p.run()
    assert launches == [("fp32", d), ("s8", d8, x8, pk8, y8, r8)]


def test_step_names_order_and_flops(launches):
    pk = ops.pack_conv(_weights(32, 16, 3), None, CPU)
    pk8 = ops.pack_conv_s8(_weights(64, 32, 1, 2), None, CPU)
    x, y = NHWC.alloc(1, 8, 8, 16, CPU), NHWC.alloc(1, 4, 4, 32, CPU)
    x8, y8 = NHWC.alloc_s8(1, 8, 8, 32, CPU), NHWC.alloc_s8(1, 8, 8, 64, CPU)
    p = LaunchPlan()
    p.add("pre", lambda: launches.append("pre"))
    p.conv("s2", x, pk, y, stride=(2, 2), pad=(1, 1))
    p.conv("ps", x, pk, y, stride=(2, 2), pad=(1, 1), flops=1234.0)
    p.conv("pw8", x8, pk8, None, out_s8=y8)
    p.add("post", lambda: launches.append("post"))
    assert [n for n, _ in p.steps] == ["pre", "conv:s2", "conv:ps", "conv:pw8", "post"]
    assert p.flops == {"conv:s2": 2.0 * 1 * 4 * 4 * 3 * 3 * 16 * 32,     # over the written output, true cin / cout
                       "conv:ps": 1234.0,
                       "conv:pw8": 2.0 * 1 * 8 * 8 * 1 * 1 * 32 * 64}
    p.run()
    assert [c if isinstance(c, str) else c[0] for c in launches] == ["pre", "fp32", "fp32", "s8", "post"]
    launches.clear()
    p.run(p.steps[1:2])                               # a sub-list of the steps
    assert launches == [("fp32", p.descs[0])]


def test_launch_replays_the_capture_of_the_steps_it_is_given(launches):
    class Graph:
        def __init__(self):
            self.replays = 0

        def replay(self):
            self.replays += 1

    p = LaunchPlan()
    p.add("net", lambda: launches.append("net"))
    stage = [("pre", lambda: launches.append("pre"))] + p.steps
    p.launch()
    p.launch(stage)
    assert launches == ["net", "pre", "net"]          # nothing captured: eager
    launches.clear()
    own, other = Graph(), Graph()
    p.graph = own
    p.launch()
    p.launch(stage)                                   # another owner's list without a capture of its own: eager, not the plan's graph
    p.launch(stage, other)
    assert (own.replays, other.replays, launches) == (1, 1, ["pre", "net"])


class _TwoPassPlan(LaunchPlan):
    """The shape of the proposal / refinement plans: the builder runs twice through ``arena.two_pass``."""

    def __init__(self, pk, pk8):
        self.passes = []
        self.arena = arena.two_pass(CPU, lambda A: self._build(A, pk, pk8))

    def _build(self, A, pk, pk8):
        self.reset()
        x = NHWC(A.alloc(1, 8, 8, 16, "f32"), c=16)
        y = NHWC(A.alloc(1, 8, 8, 32, "f32"), c=32)
        self.conv("a", x, pk, y, pad=(1, 1))
        A.release(x)
        y8 = NHWC(A.alloc(1, 8, 8, 32, "s8"), c=32, layout="s8")
        self.add("split8", lambda: None)
        z8 = NHWC(A.alloc(1, 8, 8, 64, "s8"), c=64, layout="s8")
        self.conv("b", y8, pk8, None, out_s8=z8)
        self.passes.append((len(self.steps), len(self.descs), len(self.tune_descs), len(self.flops), self.split_layers))


def test_a_second_build_pass_starts_empty(launches):
    p = _TwoPassPlan(ops.pack_conv(_weights(32, 16, 3), None, CPU), ops.pack_conv_s8(_weights(64, 32, 1), None, CPU))
    assert p.passes == [(3, 2, 1, 2, 1)] * 2
    assert [n for n, _ in p.steps] == ["conv:a", "split8", "conv:b"] and p.graph is None
    assert p.descs[0].inp and p.descs[0].out          # the descriptors of the real pass, not the shape-only one
