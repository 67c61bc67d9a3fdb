"""The case table of the bf16 / bf16x3 implicit-GEMM tests (csrc/conv_igemm_bf16.hip): the shapes tests/test_gpu_conv_bf16.py runs, the
inputs for which the kernel has to be EXACT, and the float64 value it has to return for them.  A plain module without a GPU:
tests/test_cpu_conv_bf16_cases.py proves on the CPU that the exactness condition below holds for every case.

The kernel is one template with 6 tiles x 2 stage depths x NPASS 1 / 3 x {plain, pixel-shuffle, split-K} = 72 instances, and in the
bf16 modes the plan-time tuner times all of them against each other.  `python tests/conv_bf16_cases.py` prints, per instance, the
cases that launch it.

Exactness.  bf16x3 adds hi(a)hi(b) + hi(a)lo(b) + lo(a)hi(b) with hi = bf16(x), lo = bf16(x - hi), round to nearest even (what
torch.Tensor.to(torch.bfloat16) does); bf16 adds hi(a)hi(b).  Activations and weights come from the lattice
    x = h + l,   h in +-{1 .. hmax},   l = j * 2^-11,  j in {-3 .. 3}
so that hi(x) = h and lo(x) = l exactly (3 * 2^-11 is less than half a bf16 ulp just below 1).  h * h' is an integer, h * l' a multiple
of 2^-11; bias and residual are multiples of 2^-11 with magnitude <= 8.  Every partial sum of an output element, in ANY order, is then
a multiple of 2^-11 of magnitude at most
    S_abs = sum(|hi hi| + |hi lo| + |lo hi|) + |bias| + |residual|
and while S_abs < 2^13 it fits the 24 bits of a float: nothing is rounded anywhere (MFMA accumulators, split-K workspace, its reduce)
and the output equals the float64 value of the sum bit for bit, whatever the tile, stage depth, wave layout or k-slicing.  Leaky ReLU
rounds once, v * float32(0.1) in float32, which `expected` does the same way; sigmoid is left to the kernels' other tests."""
import functools
from collections import namedtuple

import torch

import conv_exact as K
from conv_exact import SLOPE, Data, cin_pad, gemm_cout, gemm_extent, hi_lo, igemm_shapes, out_extent, product_terms, split  # noqa: F401
from conv_exact import round_up as _r

TILES = [(128, 128), (128, 64), (128, 32), (64, 128), (64, 64), (64, 32)]      # BM x BN of csrc/conv_igemm_bf16.hip's dispatch_kb
STAGES = [16, 32]                                                                # KB: k depth of one LDS stage
PRECISIONS = ["bf16", "bf16x3"]
NPASS = {"bf16": 1, "bf16x3": 3}
S_ABS_LIMIT = 2.0 ** 13
QUANTUM = 2.0 ** -11                         # of the operands' lattice, of bias and residual

# pad = (top, left, bottom, right); act in "none" / "relu" / "leaky"; res: a residual is added; hmax: the lattice's largest |h|;
# deconv: ConvTranspose2d(4, stride 2, pad 1) as a 3x3 conv with 4 * cout phase outputs and a pixel-shuffle store (pack_deconv4x4s2);
# split_k: the case is launched a second time cut into that many k-slices; win_in / win_out: (pixel stride, first channel) of the
# channel window the map occupies in a wider buffer, None = a buffer of its own.
Case = namedtuple("Case", "id n h w cin cout k stride dil pad act res hmax deconv split_k win_in win_out")


def _c(id, n, h, w, cin, cout, k, stride=1, dil=1, pad=(0, 0, 0, 0), act="none", res=False, hmax=3, deconv=False, split_k=None,
       win_in=None, win_out=None):
    return Case(id, n, h, w, cin, cout, k, stride, dil, pad, act, res, hmax, deconv, split_k, win_in, win_out)


# The smallest shapes at which each mechanism of the kernel is exercised (M = output pixels = GEMM rows, k_pad = GEMM depth):
CASES = [
    # M = 198: a ragged last row tile for 64 and for 128 rows.  Two column tiles at BN 128, the second holding 8 real columns of
    # cout_pad 160 (weight rows beyond cout_pad are zero-filled by the kernel).  cin_pad 20 is a multiple of neither stage depth, so
    # the tap changes inside a stage.  k_pad 192.
    _c("k3-c20", 2, 9, 11, 20, 136, 3, pad=(1, 1, 1, 1), act="leaky", res=True, win_in=(28, 4), win_out=(144, 4)),
    # cin_pad 4: one 32-deep stage walks eight taps (the `while (c >= cin_pad)` carry).  k_pad 224 = 7 stages at KB 32 (odd), 14 at
    # 16.  Asymmetric padding.  A k tail of zero taps (kh >= p.kh).
    _c("k7-c3", 1, 19, 23, 3, 64, 7, stride=2, pad=(2, 2, 3, 3), act="relu"),
    # k_pad 32: a single stage at KB 32 -- the pipelined loop runs only its epilogue -- and two at KB 16.  M = 35: smaller than any tile.
    _c("pw-c32", 1, 5, 7, 32, 32, 1),
    # 23 stages at KB 32, 46 at 16.  With split_k = 4 the last slice is short: 5 of 6 stages at KB 32, 10 of 12 at KB 16.
    _c("pw-c728", 1, 13, 13, 728, 168, 1, act="relu", res=True, hmax=2, split_k=4),
    # cout_pad 64 inside 128-wide tiles.  The dilated taps reach outside the map on every side.  Batch boundaries inside a row tile.
    _c("atrous", 3, 8, 9, 36, 40, 3, dil=2, pad=(2, 2, 2, 2), act="leaky"),
    # stride with padding at the bottom and on the right only
    _c("s2-pad01", 1, 10, 10, 64, 96, 3, stride=2, pad=(0, 0, 1, 1), act="relu"),
    # the pixel-shuffle store, and with split_k = 2 the pixel-shuffle form of the reduce; the output is a window of a wider buffer
    _c("deconv", 2, 6, 5, 37, 2, 4, deconv=True, split_k=2, win_out=(8, 4)),
    # ... with a longer k
    _c("deconv-c132", 1, 4, 7, 132, 2, 4, hmax=2, deconv=True),
]
BY_ID = {c.id: c for c in CASES}
GAUSSIAN = ["k3-c20", "pw-c728", "atrous", "deconv"]        # the layers of the Gaussian-data tests

def k_pad(case):
    return _r((9 if case.deconv else case.k * case.k) * cin_pad(case), 32)


def launches(case):
    """(kernel form, split_k) of every launch of the case; -1 = no k-slices."""
    return [("pixshuf" if case.deconv else "plain", -1)] + ([("splitk", case.split_k)] if case.split_k else [])


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The lattice inputs of the case (float32, on the host; the same tensors on every call: do not write to them)."""
    return K.lattice_inputs(igemm_shapes(case), K.generator(case.id), case.hmax, QUANTUM, QUANTUM, res="quanta" if case.res else None)


@functools.lru_cache(maxsize=None)
def gaussian_inputs(case):
    """Full-mantissa data on the same layer: the hi / lo rounding of arbitrary values."""
    return K.gaussian_inputs(igemm_shapes(case), K.generator(case.id, 1), case.cin * (4 if case.deconv else case.k * case.k), res=case.res)


def conv(case, x, w):
    """The layer's convolution without bias, residual or activation, in the dtype of its operands."""
    return K.conv(x, w, case.pad, case.stride, case.dil, case.deconv)


def magnitude(case, terms, data):
    """sum |a| |b| over the product terms + |bias| + |residual|, float64."""
    return K.magnitude(functools.partial(conv, case), terms, data.b, data.res)


def product_sum(case, prec, data, dtype=torch.float64):
    """-> (the sum of the product convolutions + bias + residual evaluated in ``dtype``, S_abs in float64)."""
    terms = product_terms(prec, data.x, data.w)
    return K.pre_activation(functools.partial(conv, case), terms, data.b, data.res, dtype), magnitude(case, terms, data)


def activate(case, v):
    return K.activate(case.act, v)


@functools.lru_cache(maxsize=None)
def expected(case, prec):
    """-> (what the kernel must return for the lattice inputs, float64 NCHW; S_abs).  The activation is applied in float32 to the exact
    pre-activation: the single rounding the kernel makes (tests/test_cpu_conv_bf16_cases.py asserts that .float() loses nothing)."""
    pre, s_abs = product_sum(case, prec, inputs(case))
    return K.exact(case.act, pre), s_abs


def true_conv(case, data):
    """-> (the layer on the unsplit operands in float64, S_true = conv(|x|, |w|) + |b| + |res|)."""
    return K.true_conv(functools.partial(conv, case), case.act, data)


if __name__ == "__main__":                   # python tests/conv_bf16_cases.py: per kernel instance, the cases that launch it
    for prec in PRECISIONS:
        for form in ("plain", "pixshuf", "splitk"):
            ids = [c.id + (f" (split_k {sk})" if sk > 0 else "") for c in CASES for f, sk in launches(c) if f == form]
            for bm, bn in TILES:
                for st in STAGES:
                    print(f"<{bm}, {bn}, NPASS {NPASS[prec]}, {form}, KB {st}>  {', '.join(ids)}")
