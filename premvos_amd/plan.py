"""The launch plan the four networks share: a fixed list of named kernel launches built once per input shape, its conv
descriptors tuned once, captured into a HIP graph and replayed.

A conv step is recorded in one way for every net: the step is named ``"conv:" + key``, its descriptor goes into ``descs`` (in step
order -- ``pipeline.conv_steps`` and bench.py's roofline pair the two lists) and its algorithmic FLOPs into ``flops``.  An input in
the resident split layout S8 (bf16x3 mode) runs on csrc/conv_bf16x3_s8.hip: its descriptor is marked ``tile_hint = ops.S8_HINT``
and stays out of ``tune_descs`` (that kernel has one configuration); every fp32 conv runs on premvos_conv2d_f32 and is configured
by ``ops.autotune``.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from . import ops


class LaunchPlan:
    """``steps``: [(name, launch fn)] in launch order.  ``descs`` / ``flops``: per conv step its descriptor and its algorithmic
    FLOPs (2 x MACs with the true cin / cout, keyed by step name); ``tune_descs``: the fp32 ones; ``split_layers``: how many convs
    run on the S8 kernel.  ``graph``: the capture of the whole list (None: launched eagerly)."""

    def __init__(self):
        self.reset()

    def reset(self):
        """Empty bookkeeping.  A builder that runs twice (``arena.two_pass``) calls this at the start of each pass."""
        self.steps: List = []
        self.flops: Dict[str, float] = {}
        self.descs: List = []
        self.tune_descs: List = []
        self.split_layers = 0
        self.graph: Optional[torch.cuda.CUDAGraph] = None

    def add(self, name: str, fn: Callable[[], None]):
        self.steps.append((name, fn))

    def conv(self, key: str, x: ops.NHWC, pk, out: Optional[ops.NHWC], out_s8: Optional[ops.NHWC] = None,
             res_s8: Optional[ops.NHWC] = None, flops: Optional[float] = None, **kw):
        """Append the step ``"conv:" + key``.  ``x`` in S8 -> the S8 kernel (fp32 ``out`` and / or S8 ``out_s8``; ``res_s8``: the
        residual read from an S8 tensor); fp32 ``x`` -> premvos_conv2d_f32.  ``flops`` overrides the count over the written output
        (a transposed conv's taps are not those of the conv it runs as).  Returns the descriptor."""
        name = "conv:" + key
        if x.layout == "s8":
            d = ops.conv_s8_desc(x, pk, out, out_s8, **kw)
            d.tile_hint = ops.S8_HINT
            self.add(name, lambda d=d, x=x, pk=pk, o8=out_s8, r8=res_s8: ops.run_s8(d, x, pk, o8, res_s8=r8))
            self.split_layers += 1
        else:
            assert out_s8 is None and res_s8 is None
            d = ops.conv_desc(x, pk, out, **kw)
            self.tune_descs.append(d)
            self.add(name, lambda d=d: ops.run_desc(d))
        self.descs.append(d)
        o = out if out is not None else out_s8
        self.flops[name] = 2.0 * o.n * o.h * o.w * pk.kh * pk.kw * pk.cin * pk.cout if flops is None else flops
        return d

    def tune(self, device):
        """Freeze a configuration into every fp32 conv; one split-K scratch buffer serves the whole (stream-ordered) list."""
        self.ws_splitk = ops.assign_workspace(ops.autotune(self.tune_descs, device) or self.tune_descs, device)

    def run(self, steps=None):
        for _, fn in (self.steps if steps is None else steps):
            fn()

    def capture(self, steps=None) -> "torch.cuda.CUDAGraph":
        """Record a launch list into a HIP graph (launch-bound layers replay as one submit); the plan's own list becomes ``graph``."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.run(steps)     # warm-up outside capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):      # other host threads (IO lanes) keep using the GPU
            self.run(steps)
        if steps is None:
            self.graph = g
        return g

    def launch(self, steps=None, graph: Optional["torch.cuda.CUDAGraph"] = None):
        """Replay the capture of ``steps`` if there is one, else launch them eagerly.  ``steps`` None: the plan's own list and
        ``graph``; a list of another owner (a stage's pre- / post-processing around the net) comes with that owner's capture."""
        g = self.graph if steps is None else graph
        if g is not None:
            g.replay()
        else:
            self.run(steps)
