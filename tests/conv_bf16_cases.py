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
import torch.nn.functional as F

TILES = [(128, 128), (128, 64), (128, 32), (64, 128), (64, 64), (64, 32)]      # BM x BN of csrc/conv_igemm_bf16.hip's dispatch_kb
STAGES = [16, 32]                                                                # KB: k depth of one LDS stage
PRECISIONS = ["bf16", "bf16x3"]
NPASS = {"bf16": 1, "bf16x3": 3}
S_ABS_LIMIT = 2.0 ** 13
QUANTUM = 2.0 ** -11
SLOPE = 0.1

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

Data = namedtuple("Data", "x w b res")                      # x [n][cin][h][w]; w OIHW, for a deconv [cin][cout][4][4]; res NCHW like the output


def _r(v, m):
    return (v + m - 1) // m * m


def cin_pad(case):
    return _r(case.cin, 4)


def gemm_cout(case):
    return 4 * case.cout if case.deconv else case.cout


def k_pad(case):
    return _r((9 if case.deconv else case.k * case.k) * cin_pad(case), 32)


def gemm_extent(case):
    """Rows and columns of output pixels the GEMM walks (a deconv: the input's; its store doubles both)."""
    if case.deconv:
        return case.h, case.w
    pt, pl, pb, pr = case.pad
    span = case.dil * (case.k - 1) + 1
    return (case.h + pt + pb - span) // case.stride + 1, (case.w + pl + pr - span) // case.stride + 1


def out_extent(case):
    ho, wo = gemm_extent(case)
    return (2 * ho, 2 * wo) if case.deconv else (ho, wo)


def launches(case):
    """(kernel form, split_k) of every launch of the case; -1 = no k-slices."""
    return [("pixshuf" if case.deconv else "plain", -1)] + ([("splitk", case.split_k)] if case.split_k else [])


def _generator(case, salt=0):
    return torch.Generator().manual_seed(sum(map(ord, case.id)) + salt)


def lattice(shape, generator, hmax):
    h = torch.randint(1, hmax + 1, shape, generator=generator).float()
    sign = torch.randint(0, 2, shape, generator=generator).float() * 2 - 1
    j = torch.randint(-3, 4, shape, generator=generator).float()
    return sign * h + j * QUANTUM


def _quanta(shape, generator):
    """Multiples of 2^-11 in [-8, 8]."""
    return torch.randint(-8 * 2048, 8 * 2048 + 1, shape, generator=generator).float() * QUANTUM


def _shapes(case):
    w = (case.cin, case.cout, 4, 4) if case.deconv else (case.cout, case.cin, case.k, case.k)
    return (case.n, case.cin, case.h, case.w), w, (case.cout,), (case.n, case.cout) + out_extent(case)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The lattice inputs of the case (float32, on the host; the same tensors on every call: do not write to them)."""
    g = _generator(case)
    xs, ws, bs, rs = _shapes(case)
    return Data(lattice(xs, g, case.hmax), lattice(ws, g, case.hmax), _quanta(bs, g), _quanta(rs, g) if case.res else None)


@functools.lru_cache(maxsize=None)
def gaussian_inputs(case):
    """Full-mantissa data on the same layer: the hi / lo rounding of arbitrary values."""
    g = _generator(case, 1)
    xs, ws, bs, rs = _shapes(case)
    fan_in = case.cin * (4 if case.deconv else case.k * case.k)
    return Data(torch.randn(xs, generator=g), torch.randn(ws, generator=g) * (2.0 / fan_in) ** 0.5, torch.randn(bs, generator=g) * 0.1,
                torch.randn(rs, generator=g) if case.res else None)


def hi_lo(x):
    """The split the kernel makes of a float32 tensor, as float32: hi = bf16(x), lo = bf16(x - hi)."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def split(x):
    """hi_lo of lattice data, where the two parts hold all of x."""
    hi, lo = hi_lo(x)
    assert torch.equal(hi + lo, x) and torch.equal((hi.double() + lo.double()).float(), x)
    return hi, lo


def product_terms(prec, x, w):
    """The (activation part, weight part) pairs the kernel multiplies, in the order it adds them."""
    (xh, xl), (wh, wl) = hi_lo(x), hi_lo(w)
    return [(xh, wh)] if prec == "bf16" else [(xl, wh), (xh, wl), (xh, wh)]


def conv(case, x, w):
    """The layer's convolution without bias, residual or activation, in the dtype of its operands."""
    if case.deconv:
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    pt, pl, pb, pr = case.pad
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, stride=case.stride, dilation=case.dil)


def magnitude(case, terms, data):
    """sum |a| |b| over the product terms + |bias| + |residual|, float64."""
    s = sum(conv(case, a.double().abs(), b.double().abs()) for a, b in terms) + data.b.double().abs().view(1, -1, 1, 1)
    return s + data.res.double().abs() if data.res is not None else s


def product_sum(case, prec, data, dtype=torch.float64):
    """-> (the sum of the product convolutions + bias + residual evaluated in ``dtype``, S_abs in float64)."""
    terms = product_terms(prec, data.x, data.w)
    pre = sum(conv(case, a.to(dtype), b.to(dtype)) for a, b in terms) + data.b.to(dtype).view(1, -1, 1, 1)
    if data.res is not None:
        pre = pre + data.res.to(dtype)
    return pre, magnitude(case, terms, data)


def activate(case, v):
    """apply_act of csrc/common.h in the dtype of ``v``; the slope is the float32 the kernel is handed."""
    slope = torch.tensor(SLOPE, dtype=torch.float32).to(v.dtype)
    return v if case.act == "none" else v.clamp_min(0) if case.act == "relu" else torch.where(v > 0, v, v * slope)


@functools.lru_cache(maxsize=None)
def expected(case, prec):
    """-> (what the kernel must return for the lattice inputs, float64 NCHW; S_abs).  The activation is applied in float32 to the exact
    pre-activation: the single rounding the kernel makes (tests/test_cpu_conv_bf16_cases.py asserts that .float() loses nothing)."""
    pre, s_abs = product_sum(case, prec, inputs(case))
    return activate(case, pre.float()).double(), s_abs


def true_conv(case, data):
    """-> (the layer on the unsplit operands in float64, S_true = conv(|x|, |w|) + |b| + |res|)."""
    pre = conv(case, data.x.double(), data.w.double()) + data.b.double().view(1, -1, 1, 1)
    if data.res is not None:
        pre = pre + data.res.double()
    return activate(case, pre), magnitude(case, [(data.x, data.w)], data)


if __name__ == "__main__":                   # python tests/conv_bf16_cases.py: per kernel instance, the cases that launch it
    for prec in PRECISIONS:
        for form in ("plain", "pixshuf", "splitk"):
            ids = [c.id + (f" (split_k {sk})" if sk > 0 else "") for c in CASES for f, sk in launches(c) if f == form]
            for bm, bn in TILES:
                for st in STAGES:
                    print(f"<{bm}, {bn}, NPASS {NPASS[prec]}, {form}, KB {st}>  {', '.join(ids)}")
