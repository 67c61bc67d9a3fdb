"""The case table of the fp32 implicit-GEMM tests (csrc/conv_igemm_f32.hip): the shapes tests/test_gpu_conv_f32.py runs, the inputs for
which the kernel has to be EXACT, and the float64 value it has to return for them.  A plain module without a GPU:
tests/test_cpu_conv_f32_cases.py proves on the CPU that the exactness condition below holds for every case and that the table reaches
every mechanism its comments name.

conv_igemm_f32_kernel is one template <BM, BN, WM, WN, PIXSHUF, SPLITK, KB, PW>: 9 tiles at KB 16, four of them at KB 32 too, each in
five forms {plain, plain-PW, split-K, split-K-PW, pixel-shuffle} = 65 kernels, plus splitk_reduce_kernel<false / true>.
`python tests/conv_f32_cases.py` prints, per instance, the cases that launch it.

Exactness.  The fp32 MFMA multiplies and accumulates in float32.  Activations and weights come from the lattice
    x = +-h + j * 2^-4,   h in {1 .. hmax},   j in {-3 .. 3}
so every product is a multiple of 2^-8; bias and residual are multiples of 2^-8 with magnitude <= 8.  Every partial sum of an output
element, in ANY order, is then a multiple of 2^-8 of magnitude at most
    S_abs = conv(|x|, |w|) + |bias| + |residual|
and while S_abs < 2^16 = 2^24 * 2^-8 it fits the 24 bits of a float: nothing is rounded anywhere (MFMA accumulators, split-K slabs, their
reduce) and the output equals the float64 value of the sum bit for bit, whatever the tile, stage depth, wave layout or k-slicing.
Leaky ReLU rounds once, v * float32(0.1) in float32, which `expected` does the same way; sigmoid is left to the kernels' other tests.
The kernel promises "the same sums up to the sign of an exact zero", so the comparison is torch.equal on floats (-0 == +0)."""
import functools
from collections import namedtuple

import torch

import conv_exact as K
from conv_exact import SLOPE, Data, cin_pad, gemm_cout, gemm_extent, igemm_shapes, out_extent, round_up as _r  # noqa: F401

# hint (BM << 16 | BN) of premvos_conv2d_f32's dispatch -> waves (WM, WN).  (256, 129) is the 256x128 tile with four 128x64 waves.
WAVES = {(256, 128): (4, 2), (256, 129): (2, 2), (128, 128): (2, 2), (128, 96): (4, 1), (128, 64): (2, 2), (128, 32): (4, 1),
         (64, 128): (2, 2), (64, 64): (2, 2), (64, 32): (2, 1)}
TILES = list(WAVES)
TILES_KB32 = [(256, 128), (128, 128), (128, 64), (64, 128)]
PAIRS = [(t, 16) for t in TILES] + [(t, 32) for t in TILES_KB32]              # the 13 (tile, stage depth) pairs that are instantiated
FORMS = ["plain", "plain-pw", "splitk", "splitk-pw", "pixshuf"]                # launch_cfg's five instantiations of a pair
S_ABS_LIMIT = 2.0 ** 16
QUANTUM = 2.0 ** -8                          # of products, bias and residual
STEP = 2.0 ** -4                             # of the operands' lattice

# pad = (top, left, bottom, right); act in "none" / "relu" / "leaky"; res: a residual is added; hmax: the lattice's largest |h|;
# deconv: ConvTranspose2d(4, stride 2, pad 1) as a 3x3 conv with 4 * cout phase outputs and a pixel-shuffle store (pack_deconv4x4s2);
# split_k: the case is launched a second time cut into that many k-slices; tail: (tail_m_tiles, tail_split_k) of a further launch whose
# last rows of tiles run as k-slices; hints: (tile_hint, stage_k) of the other kernels that promise the same products on this layer;
# win_in / win_out: (pixel stride, first channel) of the channel window the map occupies in a wider buffer, None = a buffer of its own.
Case = namedtuple("Case", "id n h w cin cout k stride dil pad act res hmax deconv split_k tail hints win_in win_out")


def _c(id, n, h, w, cin, cout, k, stride=1, dil=1, pad=(0, 0, 0, 0), act="none", res=False, hmax=3, deconv=False, split_k=None,
       tail=None, hints=(), win_in=None, win_out=None):
    return Case(id, n, h, w, cin, cout, k, stride, dil, pad, act, res, hmax, deconv, split_k, tail, hints, win_in, win_out)


# The smallest shapes at which each mechanism of the kernel is exercised (M = output pixels = GEMM rows, k_pad = GEMM depth):
CASES = [
    # M = 198: a ragged last row tile for 64, 128 and 256 rows.  Two column tiles at BN 128, the second holding 8 real columns of
    # cout_pad 160: NARROW with one live block at 128x128, skipped column blocks (nvalid) in every BN.  cin_pad 20: the tap changes inside
    # a stage.  k_pad 192, kreal 180: the last 16-deep stage holds one real 8-deep group (h_last 1), the last 32-deep stage three.
    _c("k3-c20", 2, 9, 11, 20, 136, 3, pad=(1, 1, 1, 1), act="leaky", res=True, win_in=(28, 4), win_out=(144, 4)),
    # cin_pad 4: a 16-deep stage walks four taps, a 32-deep one eight (the `while (c >= cin_pad)` carry).  k_pad 208 = 13 stages of 16,
    # 6.5 of 32 (k_pad % 32 == 16 on the general path: the last half stage is zero taps, kh >= p.kh).  Asymmetric padding.
    _c("k7-c3", 1, 19, 23, 3, 64, 7, stride=2, pad=(2, 2, 3, 3), act="relu"),
    # k_pad 32: a single stage at KB 32 -- the pipelined loop runs only its epilogue -- and two at KB 16.  M = 35: smaller than any tile.
    _c("pw-c32", 1, 5, 7, 32, 32, 1),
    # k_pad 736 = 46 stages of 16 (728 = 45.5: a half-real last stage) and 23 of 32.  Interior tiles for 64 and 128 rows.  The second
    # 128-wide column tile holds 40 real columns: NARROW with two live blocks.  With split_k = 4 the last slice is short: 10 of 12
    # stages at KB 16, 5 of 6 at KB 32.  The LDS-DMA pointwise kernel (hint 6) promises the same sums.
    _c("pw-c728", 1, 13, 13, 728, 168, 1, act="relu", res=True, split_k=4, hints=((6, 0),)),
    # strided pointwise addressing (pw_unit false), three images so that M = 168 holds an interior 128-row tile.  k_pad 208 is 16 mod
    # 32 on the PW path; cin_pad 200 >= 12 * 16, so the interior loads run with a half-real last stage.  88 real columns in the second
    # 128-wide tile (the Xception case): NARROW with three live blocks.
    _c("pw-s2-c200", 3, 13, 15, 200, 216, 1, stride=2, act="leaky", hints=((6, 0),)),
    # cout_pad 64 inside 128-wide tiles.  The dilated taps reach outside the map on every side.  Batch boundaries inside a row tile.
    _c("atrous", 3, 8, 9, 36, 40, 3, dil=2, pad=(2, 2, 2, 2), act="leaky"),
    # stride with padding at the bottom and on the right only; cout 96 is the 128x96 tile's own width
    _c("s2-pad01", 1, 10, 10, 64, 96, 3, stride=2, pad=(0, 0, 1, 1), act="relu"),
    # cout % 4 != 0 and an odd channel offset of the output window: the scalar epilogue.  6 real columns in the second 128-wide tile,
    # where NARROW must NOT engage (its store is the wide one).
    _c("scalar-c134", 2, 7, 9, 24, 134, 1, act="leaky", res=True, win_out=(140, 3)),
    # the pixel-shuffle store, and with split_k = 2 the pixel-shuffle form of the reduce; the output is a window of a wider buffer.
    # k_pad 368 is 16 mod 32.
    _c("deconv", 2, 6, 5, 37, 2, 4, deconv=True, split_k=2, win_out=(8, 4)),
    # ... with a longer k
    _c("deconv-c132", 1, 4, 7, 132, 2, 4, deconv=True),
    # Tail splits: M = 429 is two row tiles at BM 256, four at 128, seven at 64; the last one runs as three k-slices from row tile mt0 > 0
    # (slabs and reduce start at m_begin > 0).  1x1: k_pad 80 = 5 stages of 16 (slices of 2, 2, 1) or 2.5 of 32 (three single-stage
    # slices, the last half real); the first row tile is interior for BM 64, 128 and 256.
    _c("tail-pw", 3, 11, 13, 72, 160, 1, act="relu", res=True, tail=(1, 3)),
    # 3x3: k_pad 112 = 7 stages of 16 (3, 3, 1) or 3.5 of 32 (2, 2)
    _c("tail-k3", 3, 11, 13, 12, 100, 3, pad=(1, 1, 1, 1), act="leaky", tail=(1, 3)),
    # tail split combined with the pixel-shuffle store: M = 270, two row tiles at BM 256
    _c("tail-deconv", 3, 10, 9, 20, 3, 4, deconv=True, tail=(1, 3)),
    # the streaming pointwise kernel's layer (hint 5: cin = k_pad = 64, cout 128)
    _c("pw-c64", 2, 9, 10, 64, 128, 1, act="relu", res=True, hints=((5, 0),)),
    # a two-channel head on a 37x43 map (10 x 11 tiles of 4x4): the direct kernel's tiled form and, with stage_k 1, its per-pixel form
    _c("head-c36", 1, 37, 43, 36, 2, 3, pad=(1, 1, 1, 1), hints=((1, 0), (1, 1))),
]
BY_ID = {c.id: c for c in CASES}
GAUSSIAN = ["k3-c20", "pw-c728", "pw-s2-c200", "deconv", "tail-pw", "tail-k3"]       # the layers of the Gaussian-data tests

# name: what the launch is called in a failure; forms: the kernel instances it runs (of the tile and stage it is given); split_k: the
# descriptor's value (-1 = no k-slices); tail: (tail_m_tiles, tail_split_k); reduce: the form of splitk_reduce_kernel it ends with
Launch = namedtuple("Launch", "name forms split_k tail reduce")


def cout_pad(case):
    return _r(gemm_cout(case), 32)


def k_real(case):
    return (9 if case.deconv else case.k * case.k) * cin_pad(case)


def k_pad(case):
    return _r(k_real(case), 16)


def gemm_rows(case):
    ho, wo = gemm_extent(case)
    return case.n * ho * wo


def is_pw(case):
    """launch_cfg's `pw`: one tap and no padding above or to the left."""
    return not case.deconv and case.k == 1 and case.pad[:2] == (0, 0)


def pw_unit(case):
    return case.stride == 1 and gemm_extent(case) == (case.h, case.w)


def wide_ok(case):
    """The epilogue's condition for 16-byte stores (buffers of their own are 16-byte aligned and have pixel strides rounded up to 4)."""
    out_ps, off = case.win_out or (_r(case.cout, 4), 0)
    return not case.deconv and case.cout % 4 == 0 and out_ps % 4 == 0 and off % 4 == 0


def launches(case):
    """Every launch of the case in the implicit GEMM (the same-products kernels of case.hints are launched besides)."""
    base = "pixshuf" if case.deconv else "plain-pw" if is_pw(case) else "plain"
    sliced = "splitk-pw" if is_pw(case) else "splitk"
    reduce = "pixshuf" if case.deconv else "nhwc"
    out = [Launch("plain", (base,), -1, (0, 0), None)]
    if case.split_k:
        out.append(Launch(f"split_k {case.split_k}", (sliced,), case.split_k, (0, 0), reduce))
    if case.tail:
        out.append(Launch(f"tail {case.tail[0]}x{case.tail[1]}", (base, sliced), -1, case.tail, reduce))
    return out


def tile_bn(tile):
    return 128 if tile == (256, 129) else tile[1]


def grid(case, tile):
    """(row tiles, column tiles) of the whole layer."""
    return -(-gemm_rows(case) // tile[0]), -(-gemm_cout(case) // tile_bn(tile))


def slices(case, stage, n):
    """The library cuts the KT stages into ceil(KT / ceil(KT / n)) slices of whole stages -> (stages per slice, slices, stages of the last)."""
    kt = -(-k_pad(case) // stage)
    per = -(-kt // n)
    count = -(-kt // per)
    return per, count, kt - (count - 1) * per


def m_begin(case, tile, launch):
    """First GEMM row of the launch's k-sliced part (0: all of it), None without k-slices."""
    if launch.split_k > 1:
        return 0
    if launch.tail[0]:
        assert 0 < launch.tail[0] < grid(case, tile)[0], (case.id, tile)
        return (grid(case, tile)[0] - launch.tail[0]) * tile[0]
    return None


def workspace_need(case, tile, stage, launch):
    """Bytes of slabs the launch needs (premvos_conv2d_workspace_bytes): slices x k-sliced rows x padded columns x 4."""
    mb = m_begin(case, tile, launch)
    if mb is None:
        return 0
    count = slices(case, stage, launch.split_k if launch.split_k > 1 else launch.tail[1])[1]
    assert count > 1, (case.id, tile, stage)
    return count * (gemm_rows(case) - mb) * grid(case, tile)[1] * tile_bn(tile) * 4


def workgroups(case, tile, launch):
    """Workgroups of each GEMM kernel launch (the XCD swizzle works on gridDim.x * gridDim.y, per k-slice)."""
    mt, nt = grid(case, tile)
    if launch.split_k > 1:
        return [mt * nt]
    return [(mt - launch.tail[0]) * nt] + ([launch.tail[0] * nt] if launch.tail[0] else [])


def narrow_blocks(case, tile, launch):
    """Live 32-column blocks (nvn) of the column tiles that the launch computes in the NARROW 4x1 wave layout: the 128x128 tile, not
    pixel-shuffle, not split-K, a store that can be wide, at most 96 real columns."""
    if tile != (128, 128) or not wide_ok(case) or launch.forms[0] not in ("plain", "plain-pw"):
        return []
    real = [gemm_cout(case) - n0 for n0 in range(0, gemm_cout(case), 128)]
    return [-(-r // 32) for r in real if r <= 96]


def skipped_blocks(case, tile):
    """True where some wave of the tile has a 32-column block of its own that lies wholly beyond cout (nvalid < NTL)."""
    bn = tile_bn(tile)
    wtn = bn // WAVES[tile][1]
    cols = grid(case, tile)[1] * bn
    return any(wtn > 32 and min(wtn // 32, max(0, -(-(gemm_cout(case) - wn0) // 32))) < wtn // 32 for wn0 in range(0, cols, wtn))


def interior_tiles(case, tile, stage):
    """Output tiles whose stages (all but the matrix's last) are loaded unpredicated: a pointwise layer at KB 16, a tile whose staging
    units divide evenly among the threads, all BM rows < M, all BN weight rows < cout_pad."""
    bm, bn = tile[0], tile_bn(tile)
    nt = 64 * WAVES[tile][0] * WAVES[tile][1]
    kt = -(-k_pad(case) // stage)
    if not is_pw(case) or stage != 16 or (bm * 4) % nt or (bn * 4) % nt or (kt - 1) * stage > cin_pad(case) or kt < 3:
        return 0
    return (gemm_rows(case) // bm) * (cout_pad(case) // bn)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The lattice inputs of the case (float32, on the host; the same tensors on every call: do not write to them)."""
    return K.lattice_inputs(igemm_shapes(case), K.generator(case.id), case.hmax, STEP, QUANTUM, res="quanta" if case.res else None)


@functools.lru_cache(maxsize=None)
def gaussian_inputs(case):
    """Full-mantissa data on the same layer: sums that do round."""
    return K.gaussian_inputs(igemm_shapes(case), K.generator(case.id, 1), case.cin * (4 if case.deconv else case.k * case.k), res=case.res)


def conv(case, x, w):
    """The layer's convolution without bias, residual or activation, in the dtype of its operands."""
    return K.conv(x, w, case.pad, case.stride, case.dil, case.deconv)


def magnitude(case, data):
    """S = conv(|x|, |w|) + |bias| + |residual|, float64."""
    return K.magnitude(functools.partial(conv, case), [(data.x, data.w)], data.b, data.res)


def pre_activation(case, data, dtype=torch.float64):
    """conv + bias + residual evaluated in ``dtype``."""
    return K.pre_activation(functools.partial(conv, case), [(data.x, data.w)], data.b, data.res, dtype)


def activate(case, v):
    return K.activate(case.act, v)


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> (what the kernel must return for the lattice inputs, float64 NCHW; S_abs).  The activation is applied in float32 to the exact
    pre-activation: the single rounding the kernel makes (tests/test_cpu_conv_f32_cases.py asserts that .float() loses nothing)."""
    data = inputs(case)
    return K.exact(case.act, pre_activation(case, data)), magnitude(case, data)


def true_conv(case, data):
    """-> (the layer in float64, S_true = conv(|x|, |w|) + |b| + |res|)."""
    return K.true_conv(functools.partial(conv, case), case.act, data)


def instances():
    """(case id + launch name) lists per kernel instance (tile, stage, form), and per reduce form."""
    per_form = {f: [f"{c.id} ({l.name})" if l.name != "plain" else c.id for c in CASES for l in launches(c) if f in l.forms] for f in FORMS}
    return {(t, st, f): per_form[f] for t, st in PAIRS for f in FORMS}


if __name__ == "__main__":                   # python tests/conv_f32_cases.py: per kernel instance, the cases that launch it
    for (t, st, f), ids in instances().items():
        wm, wn = WAVES[t]
        print(f"<{t[0]}, {tile_bn(t)}, {wm}, {wn}, {f}, KB {st}>  {', '.join(ids) if ids else 'NOTHING'}")
    for kind in ("nhwc", "pixshuf"):
        ids = [f"{c.id} ({l.name})" for c in CASES for l in launches(c) if l.reduce == kind]
        print(f"splitk_reduce_kernel<{'true' if kind == 'pixshuf' else 'false'}>  {', '.join(ids)}")
