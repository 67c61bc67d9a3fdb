"""What the case tables of the exact conv tests share (tests/conv_*_cases.py): how a case's data is drawn, the float64 reference of a
padded / strided / dilated / transposed convolution, the bf16 hi / lo split, and the sums `expected` and the bounds are made of.  Pure
torch on the host.  A table keeps its exactness argument, its constants, its cases and the geometry of its own kernels, and binds the
functions below to its constants.

The order and kind of the random draws is part of every table's data: x, w, bias, residual, from one generator."""
from collections import namedtuple

import torch
import torch.nn.functional as F

SLOPE = 0.1
Data = namedtuple("Data", "x w b res")       # x [n][cin][h][w]; w OIHW, transposed [cin][cout][kh][kw]; b [cout] or None; res NCHW like the output or None


def round_up(v, m):
    return (v + m - 1) // m * m


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous()


# ---- geometry --------------------------------------------------------------------------------------------------------------------------

def extent(h, w, kh, kw, pad, stride=1, dil=1):
    """Output rows and columns of a convolution; pad = (top, left, bottom, right)."""
    pt, pl, pb, pr = pad
    return (h + pt + pb - dil * (kh - 1) - 1) // stride + 1, (w + pl + pr - dil * (kw - 1) - 1) // stride + 1


def shapes(case, kernel, out_hw, transposed=False):
    """-> the shapes of (x, w, bias, residual) of a case with the fields n, cin, h, w, cout."""
    w = (case.cin, case.cout) if transposed else (case.cout, case.cin)
    return (case.n, case.cin, case.h, case.w), w + tuple(kernel), (case.cout,), (case.n, case.cout) + tuple(out_hw)


# The implicit-GEMM tables' cases have a square kernel `k` and `deconv`: ConvTranspose2d(4, stride 2, pad 1) run as a 3x3 conv with
# 4 * cout phase outputs and a pixel-shuffle store.
def cin_pad(case):
    return round_up(case.cin, 4)


def gemm_cout(case):
    return 4 * case.cout if case.deconv else case.cout


def gemm_extent(case):
    """Rows and columns of output pixels the GEMM walks (a deconv: the input's; its store doubles both)."""
    return (case.h, case.w) if case.deconv else extent(case.h, case.w, case.k, case.k, case.pad, case.stride, case.dil)


def out_extent(case):
    ho, wo = gemm_extent(case)
    return (2 * ho, 2 * wo) if case.deconv else (ho, wo)


def igemm_shapes(case):
    return shapes(case, (4, 4) if case.deconv else (case.k, case.k), out_extent(case), case.deconv)


# ---- data ------------------------------------------------------------------------------------------------------------------------------

def generator(case_id, offset=0):
    return torch.Generator().manual_seed(sum(map(ord, case_id)) + offset)


def lattice(shape, g, hmax, step):
    """+-h + j * step,  h in {1 .. hmax},  j in {-3 .. 3}."""
    h = torch.randint(1, hmax + 1, shape, generator=g).float()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    j = torch.randint(-3, 4, shape, generator=g).float()
    return sign * h + j * step


def quanta(shape, g, quantum):
    """Whole multiples of ``quantum`` (a power of two) in [-8, 8]."""
    n = round(8 / quantum)
    return torch.randint(-n, n + 1, shape, generator=g).float() * quantum


def lattice_inputs(shp, g, hmax, step, quantum, bias=True, res=None):
    """Lattice activations and weights, a bias of quanta, and a residual of quanta (res "quanta") or from the lattice ("lattice")."""
    xs, ws, bs, rs = shp
    x, w = lattice(xs, g, hmax, step), lattice(ws, g, hmax, step)
    b = quanta(bs, g, quantum) if bias else None
    return Data(x, w, b, quanta(rs, g, quantum) if res == "quanta" else lattice(rs, g, hmax, step) if res == "lattice" else None)


def gaussian_inputs(shp, g, fan_in, bias=True, res=False):
    """Full-mantissa data: He-scaled weights, a small bias, a unit residual."""
    xs, ws, bs, rs = shp
    return Data(torch.randn(xs, generator=g), torch.randn(ws, generator=g) * (2.0 / fan_in) ** 0.5,
                torch.randn(bs, generator=g) * 0.1 if bias else None, torch.randn(rs, generator=g) if res else None)


# ---- the bf16 split --------------------------------------------------------------------------------------------------------------------

def hi_lo(x):
    """The split the kernels make of a float32 tensor, as float32: hi = bf16(x), lo = bf16(x - hi)."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def split(x):
    """hi_lo of lattice data, where the two parts hold all of x."""
    hi, lo = hi_lo(x)
    assert torch.equal(hi + lo, x) and torch.equal((hi.double() + lo.double()).float(), x)
    return hi, lo


def product_terms(prec, x, w):
    """The (activation part, weight part) pairs a kernel multiplies, in the order it adds them; fp32 is the one-term case."""
    if prec == "fp32":
        return [(x, w)]
    (xh, xl), (wh, wl) = hi_lo(x), hi_lo(w)
    return [(xh, wh)] if prec == "bf16" else [(xl, wh), (xh, wl), (xh, wh)]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def conv(x, w, pad=(0, 0, 0, 0), stride=1, dil=1, transposed=False):
    """The convolution without bias, residual or activation, in the dtype of its operands; pad = (top, left, bottom, right).
    transposed: ConvTranspose2d(4, stride 2, pad 1)."""
    if transposed:
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    pt, pl, pb, pr = pad
    return F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, stride=stride, dilation=dil)


def pre_activation(conv_fn, terms, bias, res, dtype=torch.float64):
    """The sum over the product terms of conv_fn(a, b), + bias + residual, evaluated in ``dtype``."""
    pre = sum(conv_fn(a.to(dtype), b.to(dtype)) for a, b in terms)
    if bias is not None:
        pre = pre + bias.to(dtype).view(1, -1, 1, 1)
    return pre + res.to(dtype) if res is not None else pre


def magnitude(conv_fn, terms, bias, res):
    """sum |a| |b| over the product terms + |bias| + |residual|, float64: the bound of every partial sum."""
    return pre_activation(conv_fn, [(a.double().abs(), b.double().abs()) for a, b in terms], None if bias is None else bias.double().abs(),
                          None if res is None else res.double().abs())


def activate(act, v):
    """apply_act of csrc/common.h in the dtype of ``v``; the slope is the float32 the kernel is handed."""
    slope = torch.tensor(SLOPE, dtype=torch.float32).to(v.dtype)
    return v if act == "none" else v.clamp_min(0) if act == "relu" else torch.where(v > 0, v, v * slope)


def exact(act, pre):
    """What a kernel must return where ``pre`` (float64) is exact: the activation applied in float32, the one rounding it makes."""
    return activate(act, pre.float()).double()


def true_conv(conv_fn, act, data):
    """-> (the layer on the unsplit operands in float64, S_true = conv(|x|, |w|) + |b| + |res|)."""
    terms = [(data.x, data.w)]
    return activate(act, pre_activation(conv_fn, terms, data.b, data.res)), magnitude(conv_fn, terms, data.b, data.res)
