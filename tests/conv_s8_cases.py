"""The case table of the exact tests of csrc/conv_bf16x3_s8.hip (tests/test_gpu_conv_s8_exact.py): the LDS-DMA implicit GEMM on the resident
split layout S8 -- 12 tile configurations, each instantiated as a pointwise (PW) and as a general kernel --, the ping-pong pointwise
kernel and split8_kernel.  A plain module without a GPU: tests/test_cpu_conv_s8_cases.py proves on the CPU that the premises below
hold for every case.  `python tests/conv_s8_cases.py` prints, per kernel instance, the cases that launch it.

Exactness is that of tests/conv_bf16_cases.py, whose lattice this module imports: activations and weights x = h + l with h in
+-{1 .. hmax} and l = j * 2^-11, |j| <= 3, split into hi = h and lo = l without remainder, so the S8 image of an input holds all of it.
The kernel adds lo.hi + hi.lo + hi.hi per 16-deep step; bias and fp32 residual are multiples of 2^-11 of magnitude <= 8, an S8
residual is hi + lo of a lattice tensor, which the epilogue's float32 addition restores exactly.  While
    S_abs = sum(|lo hi| + |hi lo| + |hi hi|) + |bias| + |residual| < 2^13
every partial sum, in any order, is a multiple of 2^-11 that fits a float: the fp32 output equals the float64 value of the sum bit
for bit, whatever the tile, stage count or wave layout, and the S8 output is hi = bf16(v), lo = bf16(v - hi) of it, bit for bit.

Windows.  Production runs the kernel on channel windows of wider arena buffers.  A windowed input lies in a buffer otherwise filled
with NaN bf16 words: a chunk fetched from beyond the layer's channels poisons its sum instead of meeting a zero weight.  Such a
window has ps >= coff + roundup(cin, 32), so a kernel that wrongly fetched an absent chunk would still read inside the buffer."""
import functools
from collections import namedtuple

import torch

import conv_exact as K
from conv_bf16_cases import QUANTUM, S_ABS_LIMIT  # noqa: F401  (the lattice is the bf16 table's)
from conv_exact import SLOPE, Data, hi_lo, nhwc, product_terms, split  # noqa: F401
from conv_exact import round_up as _r

# (BM, BN, waves, NSTAGE, KC) of the `switch (tile)` of premvos_conv_bf16x3_s8_f32; tile 10 is the ping-pong kernel where
# pingpong(case) holds and tile 0's instance otherwise
TILES = [(256, 256, 8, 2, 32), (256, 128, 4, 3, 32), (256, 128, 4, 2, 32), (256, 128, 8, 3, 32), (128, 128, 4, 3, 32), (128, 128, 4, 2, 32),
         (256, 128, 4, 3, 16), (256, 128, 4, 2, 16), (128, 256, 4, 3, 16), (256, 64, 4, 3, 32), (256, 256, 8, 2, 32), (256, 256, 4, 2, 32)]
PINGPONG_TILE = 10
NAN_WORD = 0x7FC07FC0                        # two bf16 NaNs: what lies around a windowed input

# pad = (top, left, bottom, right); act in "none" / "relu" / "leaky"; res in None / "f32" / "s8"; hmax: the lattice's largest |h|;
# win_*: (pixel stride in floats, first channel) of the channel window in a wider buffer, None = a buffer of the layer's own width.
# win_in, win_out8 and win_res8 are S8 windows: they start on a multiple of 8 channels, which is a 32-byte boundary.
Case = namedtuple("Case", "id n h w cin cout kh kw stride dil pad act bias res hmax win_in win_out win_out8 win_res8")


def _c(id, n, h, w, cin, cout, kh=1, kw=1, stride=1, dil=1, pad=(0, 0, 0, 0), act="none", bias=True, res=None, hmax=3, win_in=None,
       win_out=None, win_out8=None, win_res8=None):
    return Case(id, n, h, w, cin, cout, kh, kw, stride, dil, pad, act, bias, res, hmax, win_in, win_out, win_out8, win_res8)


# The smallest shapes that reach each mechanism (M = output pixels = GEMM rows, KT = K stages = taps x ceil(cin / 32) x 32 / KC):
CASES = [
    # KT = 1 at 32-deep stages: the prologue is shorter than NSTAGE - 1, ping-pong takes `else wait_vm(0)`.  At KC 16 the second
    # half-stage is wholly absent (lim <= 0).  M = 35 is less than any tile.  cout 40 is no multiple of 32 (col_ok).  No bias.
    _c("pw-c8", 1, 5, 7, 8, 40, bias=False),
    # KT = 2: ping-pong issues both stages before the loop and none inside
    _c("pw-c64", 1, 9, 11, 64, 72, act="relu", res="f32"),
    # KT = 3: the first steady-state iteration of NSTAGE 3, the first in-loop `issue` of ping-pong
    _c("pw-c96", 1, 6, 5, 96, 128, act="leaky"),
    # A partial last 32-block (5 groups).  M = 1150: 5 row tiles of 256 and 9 of 128, the last ragged, a batch boundary inside a
    # row tile.  cout 264: the last column tile holds 8 real columns at BN 256, 128 and 64.  10 to 27 work-groups, nwg % 8 != 0.
    # Input, fp32 output, S8 output and S8 residual are all windows.
    _c("pw-c40", 2, 23, 25, 40, 264, act="relu", res="s8", win_in=(80, 8), win_out=(272, 4), win_out8=(280, 8), win_res8=(288, 16)),
    # 23 stages (odd), the last block 3 groups: the middle-flow / conv3 shape
    _c("pw-c728", 2, 13, 13, 728, 264, act="relu", res="s8", hmax=2),
    # A strided 1x1 (the convshortcut form): output 5 x 6 taken from the output tensor, reads pixel (2 oy, 2 ox), the last row and
    # column unused.  The general kernel, not PW.
    _c("pw-s2", 2, 10, 12, 64, 128, stride=2),
    # The tap changes every stage and every stage has a partial block
    _c("k3-c24", 2, 9, 11, 24, 136, 3, 3, pad=(1, 1, 1, 1), act="leaky", res="f32", win_in=(48, 8)),
    # kc32 = 3, 27 stages.  M = 272 is one row more than a 256 tile.  Tile 9's natural shape.
    _c("k3-c72", 1, 17, 16, 72, 64, 3, 3, pad=(1, 1, 1, 1), act="relu"),
    # Output 5 x 5 from the output tensor: the implicit bottom / right padding, reached only through the unsigned range test
    _c("s2-pad01", 1, 10, 10, 64, 96, 3, 3, stride=2, pad=(0, 0, 1, 1), act="relu"),
    # Taps leave the map on every side.  Batch boundaries inside a tile.
    _c("atrous", 3, 8, 9, 40, 48, 3, 3, dil=2, pad=(2, 2, 2, 2), act="leaky", res="s8"),
    # 49 taps (the entry's maximum), one group per stage
    _c("k7-c8", 1, 19, 23, 8, 64, 7, 7, stride=2, pad=(3, 3, 3, 3), act="relu"),
    # kh != kw: the `++i_kx == p.kw` carry
    _c("k1x3", 1, 6, 20, 16, 32, 1, 3, pad=(0, 1, 0, 1)),
]
BY_ID = {c.id: c for c in CASES}
GAUSSIAN = ["pw-c40", "k3-c24", "atrous", "k3-c72"]        # the layers of the Gaussian-data tests

# ---- the launcher's geometry, restated
def out_extent(case):
    return K.extent(case.h, case.w, case.kh, case.kw, case.pad, case.stride, case.dil)


def rows(case):
    """M: output pixels = GEMM rows."""
    ho, wo = out_extent(case)
    return case.n * ho * wo


def taps(case):
    return case.kh * case.kw


def kc32(case):
    return -(-case.cin // 32)


def k_pad(case):
    return taps(case) * 32 * kc32(case)


def cout_pad(case):
    """ops.pack_conv_s8: whole 256-row tiles."""
    return _r(case.cout, 256)


def kt(case, tile):
    """K stages: every tap is padded to whole 32-channel blocks, a KC-16 tile walks each in two halves."""
    return taps(case) * kc32(case) * (32 // TILES[tile][4])


def row_tiles(case, tile):
    return -(-rows(case) // TILES[tile][0])


def col_tiles(case, tile):
    return -(-case.cout // TILES[tile][1])


def work_groups(case, tile):
    return row_tiles(case, tile) * col_tiles(case, tile)


def last_tile_columns(case, tile):
    """Real columns of the last column tile."""
    return case.cout - (col_tiles(case, tile) - 1) * TILES[tile][1]


def is_pw(case):
    """The launcher's `pw`: the PW instantiation (no tap offsets, no range test) instead of the general one."""
    return taps(case) == 1 and case.stride == 1 and case.pad[:2] == (0, 0) and out_extent(case) == (case.h, case.w)


def pingpong(case):
    """The three conditions under which tile 10 takes the ping-pong kernel: a pointwise layer, both operands span less than 4 GB
    (32-bit byte offsets; in_ps of the buffer the test builds), weight rows padded to whole 256-row tiles."""
    in_ps = case.win_in[0] if case.win_in else case.cin
    small = rows(case) * in_ps * 4 < 2 ** 32 and cout_pad(case) * kc32(case) * 128 < 2 ** 32
    return is_pw(case) and small and cout_pad(case) % 256 == 0


def absent_half_stage(case):
    """At KC 16 the second half of the layer's last 32-channel block holds no channel group at all (`lim <= 0`)."""
    return case.cin // 8 - (kc32(case) * 2 - 1) * 2 <= 0


def instance(case, tile):
    """The kernel a launch of the case with this tile runs."""
    if tile == PINGPONG_TILE and pingpong(case):
        return "pingpong"
    bm, bn, waves, nstage, kc = TILES[tile]
    return f"<{bm}, {bn}, {waves} waves, NSTAGE {nstage}, KC {kc}, {'PW' if is_pw(case) else 'general'}>"


# ---- data
def _shapes(case):
    return K.shapes(case, (case.kh, case.kw), out_extent(case))


def _generator(case, salt=0):
    return K.generator(case.id, 1000 * salt + 7)                               # this table's own offsets: 7 and 1007


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The lattice inputs of the case (float32, on the host; the same tensors on every call: do not write to them).  An fp32 residual
    is made of quanta, an S8 residual is a lattice tensor: its S8 image holds all of it."""
    return K.lattice_inputs(_shapes(case), _generator(case), case.hmax, QUANTUM, QUANTUM, bias=case.bias,
                            res={None: None, "f32": "quanta", "s8": "lattice"}[case.res])


@functools.lru_cache(maxsize=None)
def gaussian_inputs(case):
    """Full-mantissa data on the same layer: the hi / lo rounding of arbitrary values."""
    return K.gaussian_inputs(_shapes(case), _generator(case, 1), case.cin * taps(case), bias=case.bias, res=case.res)


def residual_value(case, data):
    """What the epilogue adds: an fp32 residual as it is, an S8 residual as hi + lo (float32; exact for lattice data)."""
    if case.res != "s8":
        return data.res
    hi, lo = hi_lo(data.res)
    return hi + lo


# ---- the reference
def conv(case, x, w):
    """The layer's convolution without bias, residual or activation, in the dtype of its operands."""
    return K.conv(x, w, case.pad, case.stride, case.dil)


def activate(case, v):
    return K.activate(case.act, v)


def magnitude(case, terms, data):
    """sum |a| |b| over the product terms + |bias| + |residual| (an S8 residual as hi + lo), float64."""
    return K.magnitude(functools.partial(conv, case), terms, data.b, residual_value(case, data))


def product_sum(case, data, dtype=torch.float64):
    """-> (sum(lo.hi + hi.lo + hi.hi) + bias + residual evaluated in ``dtype``, S_abs in float64)."""
    terms = product_terms("bf16x3", data.x, data.w)
    return K.pre_activation(functools.partial(conv, case), terms, data.b, residual_value(case, data), dtype), magnitude(case, terms, data)


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> (what the kernel must write as fp32 for the lattice inputs, float64 NCHW; expected_s8 = (hi, lo) of it, what the S8 output
    must hold, as two bf16 tensors).  The activation is applied in float32 to the exact pre-activation: the single rounding the
    kernel makes (tests/test_cpu_conv_s8_cases.py asserts that .float() loses nothing)."""
    ref = K.exact(case.act, product_sum(case, inputs(case))[0])
    hi, lo = hi_lo(ref.float())
    return ref, (hi.to(torch.bfloat16), lo.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def s_abs(case):
    return product_sum(case, inputs(case))[1]


def true_conv(case, data):
    """-> (the layer on the unsplit operands and the unsplit residual in float64, S_true = conv(|x|, |w|) + |b| + |res|)."""
    return K.true_conv(functools.partial(conv, case), case.act, data)


# ---- the S8 layout on the host, from the comment in csrc/common.h: every group of EIGHT channels of a pixel is the 32 bytes
# {hi(8 x bf16), lo(8 x bf16)}, stored in place of its eight floats; hi = bf16(x) (round to nearest even), lo = bf16(x - hi)
def encode_s8(x_nhwc):
    """float32 [..., c] with c % 8 == 0 -> int32 [..., c]: the words of the 32-byte groups."""
    assert x_nhwc.dtype == torch.float32 and x_nhwc.shape[-1] % 8 == 0
    hi, lo = hi_lo(x_nhwc)
    lead = x_nhwc.shape[:-1]
    halves = torch.stack([hi.to(torch.bfloat16).reshape(*lead, -1, 8), lo.to(torch.bfloat16).reshape(*lead, -1, 8)], dim=-2)   # [..., group, hi | lo, 8]
    return halves.contiguous().view(torch.int16).reshape(*lead, -1).view(torch.int32)


def decode_s8(words):
    """int32 [..., c] -> float32 [..., c]: hi + lo, the value a consumer multiplies."""
    assert words.dtype == torch.int32 and words.shape[-1] % 8 == 0
    lead = words.shape[:-1]
    halves = words.contiguous().view(torch.bfloat16).reshape(*lead, -1, 2, 8).float()
    return (halves[..., 0, :] + halves[..., 1, :]).reshape(*lead, -1)


def window(case, which):
    """(pixel stride in floats, first channel) of the buffer that holds the input / fp32 output / S8 output / S8 residual."""
    win, c = {"in": (case.win_in, case.cin), "out": (case.win_out, case.cout), "out8": (case.win_out8, case.cout),
              "res8": (case.win_res8, case.cout)}[which]
    return win or (c, 0)


if __name__ == "__main__":                   # python tests/conv_s8_cases.py: per kernel instance, the cases that launch it
    table = {}
    for tile in range(len(TILES)):
        for c in CASES:
            table.setdefault((tile, instance(c, tile)), []).append(f"{c.id} (KT {kt(c, tile)}, {work_groups(c, tile)} wg)")
    for (tile, name), ids in table.items():
        print(f"tile {tile:2d} {name}:  {', '.join(ids)}")
    print("split8_kernel:  test_split8_is_the_bf16_split_bit_for_bit")
