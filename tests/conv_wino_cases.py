"""The case table of the exact Winograd tests (csrc/conv_wino_f32.hip, csrc/conv_wino4_f32.hip): the shapes
tests/test_gpu_conv_wino_exact.py runs, the inputs for which every Winograd kernel has to be EXACT, and the float64 value it has to
return for them.  A plain module without a GPU: tests/test_cpu_conv_wino_cases.py proves on the CPU that the exactness condition below
holds for every case and that the table reaches every kernel and every mechanism its comments name.

The two files hold 24 kernels.  F(2x2,3x3): wino_gemm_kernel<128,32,4,1>, <128,64,2,2>, <64,64,2,2>, <128,128,2,2>, <64,128,2,2> and
wino_output_kernel (tile_hint 2, stage_k 0 / 64), and the six blocks of wino_fused_kernel (tile_hint 3, stage_k 0, 2 .. 6).
F(4x4,3x3): wino4_input_kernel, nine wino4_gemm_kernel instances and wino4_output_kernel<true / false> (tile_hint 4, stage_k 0 / 16 /
64 / 80), also behind the kept-slab entry premvos_conv_wino4_slab_f32.  `python tests/conv_wino_cases.py` prints, per kernel, the
(case, hint, stage_k) that launch it.

Exactness.  Activations are integers from {-1, 0, 1}; weights are 576 * 2^-S * {-1, 0, 1}; every entry is non-zero with probability
`density` (1/2).  576 is the common denominator of G g G^T for F(4x4,3x3) and a multiple of the 4 that F(2x2,3x3) needs, so both
filter transforms are whole multiples of QUANTUM = 2^-S, rounded nowhere; the input transforms are integers.  In quanta, per case and
per family (F(2x2): both hints 2 and 3):
    V_abs = |B^T| |d| |B|                       (the intermediates of the input transform are at most 100 x the data: exact)
    U_abs = |G| |g| |G^T|
    M_abs = sum_k V_abs * U_abs  < 2^24         every partial sum of every component GEMM is exact in ANY order, whatever the block,
                                                stage depth or wave layout
    Y_abs = |A^T| |M| |A| + |bias| + |res| < 2^24, with the true M: both passes of the output transform (the slab-free kernel: its
                                                running sums over the components) and the epilogue are exact
Bias and residual are whole multiples of QUANTUM of magnitude <= 8.  When both caps hold, every Winograd kernel has to return the
float64 value of conv + bias + residual bit for bit.  Leaky ReLU rounds once, v * float32(0.1) in float32, which `expected` does the
same way; sigmoid is left to the kernels' other tests.  The caps are caps: a case that misses one gets sparser data, never a wider cap.

Roundings (the derived bound of the Gaussian-data test), counted in the code, one per float32 operation on the longest path:
    F(4x4), hint 4:  bt6 twice -- t[0] = 4 d0 - 5 d2 + d4: the multiply by 5, the subtraction, the addition (4 d0 is exact) = 3 per pass
                     -> 6;  U rounded once by pack_winograd4 -> 1;  at6 twice -- s[3] = d12 + 8 d34 + m5 through m1: d12, + 8 d34,
                     + m5 = 3 per pass -> 6.                                                                            T = 13
    F(2x2), hint 2:  lstore's (d11 + sj d12) + si (d21 + sj d22), si, sj = +-1: the inner and the outer addition -> 2;  U -> 1;
                     wino_output_kernel: a + b + c twice -> 4.                                                          T = 7
    F(2x2), hint 3:  the same lstore -> 2;  U -> 1;  Y[ya][yb] += c * M, c = +-1, for the nine components with a non-zero
                     A^T (x) A^T weight -> 9 (the first, to a zero accumulator, counted as well).                        T = 12
The Kp accumulations of the GEMM and the two additions of the epilogue (bias, residual) are the `Kp` and the `+ 2` of the bound."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import conv_exact as K
from conv_exact import SLOPE, Data, cin_pad  # noqa: F401
from conv_exact import round_up as _r

S = 9
QUANTUM = 2.0 ** -S
WEIGHT = 576 * QUANTUM                       # |w| of a non-zero weight
LIMIT = 2.0 ** 24                            # of M_abs and Y_abs, in quanta
ROUNDINGS = {2: 7, 3: 12, 4: 13}            # T of the derived bound per hint (module docstring)
WINO4_MIN_C = 16                             # the tests pack F(4x4) filters with pack_conv(..., wino4_min_c=16)
WINO4_MIN_COUT = 32                          # ops.WINO4_MIN_COUT: why every cout is at least 32

HINTS = {2: (0, 64), 3: (0, 2, 3, 4, 5, 6), 4: (0, 16, 64, 80)}                # tile_hint -> its block ids (stage_k)
BLOCKS = [(h, b) for h, bs in HINTS.items() for b in bs]                       # the 12 (family, block) ids
FAMILY = {2: 2, 3: 2, 4: 4}                                                    # hint -> m of F(m x m, 3x3)
WINO_GEMM = {(128, 32): (4, 1), (128, 64): (2, 2), (64, 64): (2, 2), (128, 128): (2, 2), (64, 128): (2, 2)}     # (BM, BN) -> (WM, WN)
FUSED = {0: (128, 128, 2, 4, 16), 2: (64, 128, 2, 2, 16), 3: (64, 64, 2, 2, 16), 4: (64, 128, 2, 2, 32), 5: (64, 64, 2, 2, 32),
         6: (128, 128, 2, 4, 32)}                                              # block id -> <BM, BN, WM, WN, KB>
WINO4_GEMM = [(128, 32, 4, 1, 32)] + [(bm, bn, 2, 2, kb) for bm in (128, 64) for bn in (64, 128) for kb in (32, 16)]
SLAB_ENTRY = "premvos_conv_wino4_slab_f32"

# pad = (top, left), the same at the bottom and on the right; act in "none" / "relu" / "leaky"; res: a residual is added;
# win_in / win_out: (pixel stride, first channel) of the channel window the map occupies in a wider buffer, None = a buffer of its own;
# density: the probability of a non-zero entry in activations and weights.
Case = namedtuple("Case", "id n h w cin cout pad dil act res win_in win_out density")


def _c(id, n, h, w, cin, cout, pad=(1, 1), dil=1, act="none", res=False, win_in=None, win_out=None, density=0.5):
    return Case(id, n, h, w, cin, cout, pad, dil, act, res, win_in, win_out, density)


# The smallest shapes at which each mechanism is reached (Kp = cin_pad rounded up to 16 = GEMM depth, tiles = GEMM rows):
CASES = [
    # cin_pad 20 inside Kp 32: the pad channels [20, 32) lie in the input buffer (sentinels) and must be selected away.  60 F(2x2) and
    # 18 F(4x4) tiles: fewer than any block has rows.  Two 128-wide column tiles, the second with 8 real columns of cout_pad 160:
    # weight rows clamped or masked.  A 9 x 11 map: no multiple of 2 or 4.  Input and output are windows of wider buffers.
    _c("c20-n136", 2, 9, 11, 20, 136, act="leaky", res=True, win_in=(28, 4), win_out=(144, 4)),
    # Kp 48 = 16 mod 32: hint 4 stage_k 0 / 64 fall to the 16-deep instances with KT = 3, the fused blocks 4, 5, 6 zero-fill half a
    # stage.  168 F(4x4) tiles (128 + 40, 2 x 64 + 40) and 585 F(2x2) tiles: interior row tiles and a ragged last one.  bn 64
    # everywhere, 40 real columns of 64.
    _c("ragged-m", 3, 26, 30, 48, 40, act="relu"),
    # Kp % 32 == 0 and cout <= 32: the only way into wino4_gemm_kernel<128,32,4,1,32> (stage_k 0 / 64), with two row tiles; stage_k
    # 16 / 80 take bn 64.  The F(2x2) slab kernel is <128,32,4,1>.
    _c("c64-n32", 4, 22, 25, 64, 32, res=True),
    # PWC conv*_4 in miniature: cin_pad 536, Kp 544 = 17 stages of 32 or 34 of 16, the longest sum the exactness condition carries
    _c("long-k", 1, 9, 14, 533, 32, act="leaky"),
    # the 2 x 2 phases are of unequal size (rows 7 / 6, columns 5 / 5); output rows and columns past the map inside a tile; hint 2
    # must refuse it
    _c("atrous-2", 2, 13, 10, 36, 64, pad=(2, 2), dil=2, act="leaky", res=True),
    # the map is smaller than 4 d in both directions, one phase has a single column.  Kp 16: one 16-deep stage (the prefetching loop
    # runs only its epilogue), half a 32-deep one.  96 real columns in a 128-wide block.
    _c("atrous-4-small", 1, 9, 7, 16, 96, pad=(4, 4), dil=4, act="leaky"),
    # ho 12, wo 11: the taps reach two pixels above the map and none to its left -- pt != pl, neither is "same"
    _c("pad-2-0", 1, 10, 13, 32, 64, pad=(2, 0), act="relu"),
    # out_ps % 4 != 0 and an odd channel offset: wino4_output_kernel<false> and the scalar epilogue of the slab-free kernel
    _c("scalar-store", 1, 7, 6, 24, 68, act="leaky", res=True, win_out=(75, 3)),
]
BY_ID = {c.id: c for c in CASES}
GAUSSIAN = ["c20-n136", "ragged-m", "long-k", "atrous-2"]                      # the layers of the Gaussian-data tests

# The kept-slab entry on a DenseNet block in miniature: a concat buffer of 112 channels on a 9 x 11 map.  Layer 0 reads channels
# [64, 112) and writes [32, 64); layer 1 reads [32, 112) and writes [0, 32): it transforms only the 32 new channels and takes the
# other 48 from the slab layer 0 left.  Kp 48 and 80: 16-deep stages, bn 64.
DENSE_PS = 112
DENSE = [_c("dense-block-0", 1, 9, 11, 48, 32, win_in=(DENSE_PS, 64), win_out=(DENSE_PS, 32)),
         _c("dense-block-1", 1, 9, 11, 80, 32, win_in=(DENSE_PS, 32), win_out=(DENSE_PS, 0))]
DENSE_PLAN = [(DENSE_PS, 64, 48), (DENSE_PS, 32, 32)]                          # (pitch, v_c0, t_cn) of ops.wino4_slab_plan

def _cdiv(a, b):
    return -(-a // b)


def cout_pad(case):
    return _r(case.cout, 32)


def kp(case):
    """Depth of every component GEMM: the transformed filters are packed with k = cin_pad rounded up to 16."""
    return _r(cin_pad(case), 16)


def out_extent(case):
    return case.h + 2 * case.pad[0] - 2 * case.dil, case.w + 2 * case.pad[1] - 2 * case.dil


def takes(case, hint):
    """Whether the family runs the case: hint 2 no atrous layer; hint 3 an atrous layer only with pad = dilation
    (conv_wino_fused_applicable); hint 4 where pack_conv(..., wino4_min_c=16) packs F(4x4) filters."""
    if hint == 2:
        return case.dil == 1
    if hint == 3:
        return case.dil == 1 or case.pad == (case.dil, case.dil)
    return case.cin >= WINO4_MIN_C and case.cout >= WINO4_MIN_COUT


def phase_tiles(case, m):
    """(tile rows, tile columns) of ONE of the dil x dil phases of F(m x m, 3x3); every phase is given the same count."""
    ho, wo = out_extent(case)
    return _cdiv(_cdiv(ho, case.dil), m), _cdiv(_cdiv(wo, case.dil), m)


def tiles(case, m):
    """GEMM rows: images x phases x tiles of a phase."""
    ty, tx = phase_tiles(case, m)
    return case.n * case.dil * case.dil * ty * tx


def phase_sizes(case):
    """(rows of each row phase, columns of each column phase) of the output map."""
    ho, wo = out_extent(case)
    return [_cdiv(ho - p, case.dil) for p in range(case.dil)], [_cdiv(wo - p, case.dil) for p in range(case.dil)]


def block(case, hint, stage_k):
    """-> (BM, BN, KB) of the GEMM the (hint, stage_k) launches on the case: wino_bn / conv_wino, conv_wino_fused, wino4_bn / wino4_run."""
    if hint == 2:
        bn = 32 if case.cout <= 32 else 64 if case.cout <= 64 else 128
        return (64 if stage_k == 64 and bn > 32 else 128), bn, 16
    if hint == 3:
        bm, bn, _, _, kb = FUSED[stage_k]
        return bm, bn, kb
    k32 = kp(case) % 32 == 0 and not stage_k & 16
    if case.cout <= 32 and k32:
        return 128, 32, 32
    return (64 if stage_k & 64 else 128), (64 if case.cout <= 64 else 128), (32 if k32 else 16)


def grid(case, hint, stage_k):
    """(row tiles, column tiles) of the GEMM."""
    bm, bn, _ = block(case, hint, stage_k)
    return _cdiv(tiles(case, FAMILY[hint]), bm), _cdiv(case.cout, bn)


def wide_ok(case):
    """The 16-byte epilogue's condition (buffers of their own are 16-byte aligned with pixel strides rounded up to 4; the residual is
    always a buffer of its own)."""
    out_ps, off = case.win_out or (_r(case.cout, 4), 0)
    return out_ps % 4 == 0 and off % 4 == 0


def kernels(case, hint, stage_k):
    """The kernels the launch runs."""
    bm, bn, kb = block(case, hint, stage_k)
    if hint == 2:
        return ["wino_gemm_kernel<%d,%d,%d,%d>" % ((bm, bn) + WINO_GEMM[(bm, bn)]), "wino_output_kernel"]
    if hint == 3:
        return ["wino_fused_kernel<%d,%d,%d,%d,%d>" % FUSED[stage_k]]
    wm, wn = (4, 1) if bn == 32 else (2, 2)
    return ["wino4_input_kernel", "wino4_gemm_kernel<%d,%d,%d,%d,%d>" % (bm, bn, wm, wn, kb),
            "wino4_output_kernel<%s>" % ("true" if wide_ok(case) else "false")]


ALL_KERNELS = ["wino_gemm_kernel<%d,%d,%d,%d>" % (t + w) for t, w in WINO_GEMM.items()] + ["wino_output_kernel"] \
    + ["wino_fused_kernel<%d,%d,%d,%d,%d>" % v for v in FUSED.values()] + ["wino4_input_kernel"] \
    + ["wino4_gemm_kernel<%d,%d,%d,%d,%d>" % v for v in WINO4_GEMM] + ["wino4_output_kernel<true>", "wino4_output_kernel<false>"]


def workspace_need(case, hint, stage_k):
    """Bytes the launch asks for (premvos_conv2d_workspace_bytes): hint 2 the 16 raw component slabs, hint 4 the V and M slabs."""
    if hint == 3:
        return 0
    mt = tiles(case, FAMILY[hint])
    _, bn, _ = block(case, hint, stage_k)
    cols = _cdiv(case.cout, bn) * bn
    return 16 * mt * cols * 4 if hint == 2 else 36 * mt * (kp(case) + cols) * 4


def m_slab_need(case, stage_k):
    """Bytes of the M slab alone: what the kept-slab entry wants as the descriptor's workspace."""
    _, bn, _ = block(case, 4, stage_k)
    return 36 * tiles(case, 4) * _cdiv(case.cout, bn) * bn * 4


def half_stage(case, hint, stage_k):
    """True where the last stage of the launch's K loop is half real and zero-filled (a 32-deep stage on Kp = 16 mod 32)."""
    return block(case, hint, stage_k)[2] == 32 and kp(case) % 32 == 16


def instances():
    """kernel (or entry point) -> the "case hint/stage_k" that launch it."""
    out = {k: [] for k in ALL_KERNELS + [SLAB_ENTRY]}
    for c in CASES:
        for hint, sk in BLOCKS:
            if takes(c, hint):
                for k in kernels(c, hint, sk):
                    out[k].append(f"{c.id} {hint}/{sk}")
    for c in DENSE:
        for sk in HINTS[4]:
            for k in kernels(c, 4, sk) + [SLAB_ENTRY]:
                out[k].append(f"{c.id} slab/{sk}")
    return out


# ---- data --------------------------------------------------------------------------------------------------------------------------

def ternary(shape, generator, density):
    """{-1, 0, 1}, non-zero with probability `density`."""
    on = (torch.rand(shape, generator=generator) < density).float()
    return on * (torch.randint(0, 2, shape, generator=generator).float() * 2 - 1)


def _shapes(case):
    return K.shapes(case, (3, 3), out_extent(case))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The lattice inputs of the case (float32, on the host; the same tensors on every call: do not write to them).  The first layer
    of the dense block reads what the second one reads behind the 32 channels that are new to it: it draws no activations."""
    g = K.generator(case.id)
    xs, ws, bs, rs = _shapes(case)
    x = inputs(DENSE[1]).x[:, 32:].contiguous() if case.id == "dense-block-0" else ternary(xs, g, case.density)
    return Data(x, ternary(ws, g, case.density) * WEIGHT, K.quanta(bs, g, QUANTUM), K.quanta(rs, g, QUANTUM) if case.res else None)


@functools.lru_cache(maxsize=None)
def gaussian_inputs(case):
    """Full-mantissa data on the same layer: sums that do round."""
    return K.gaussian_inputs(_shapes(case), K.generator(case.id, 1), 9 * case.cin, res=case.res)


# ---- the direct convolution -----------------------------------------------------------------------------------------------------------

def conv(case, x, w):
    """The layer's convolution without bias, residual or activation, in the dtype of its operands."""
    return K.conv(x, w, case.pad + case.pad, 1, case.dil)


def pre_activation(case, data, dtype=torch.float64):
    return K.pre_activation(functools.partial(conv, case), [(data.x, data.w)], data.b, data.res, dtype)


def activate(case, v):
    return K.activate(case.act, v)


@functools.lru_cache(maxsize=None)
def expected(case):
    """What every kernel must return for the lattice inputs, float64 NCHW.  The activation is applied in float32 to the exact
    pre-activation: the single rounding the kernels make (tests/test_cpu_conv_wino_cases.py asserts that .float() loses nothing)."""
    return K.exact(case.act, pre_activation(case, inputs(case)))


def true_conv(case, data):
    """The layer in float64."""
    return K.true_conv(functools.partial(conv, case), case.act, data)[0]


# ---- both Winograd algorithms restated in float64 -------------------------------------------------------------------------------------

def _m64(rows):
    return torch.tensor(rows, dtype=torch.float64)


BT = {2: _m64([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
      4: _m64([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]])}
# G as (integer matrix, its denominator): the integer products keep the float64 evaluation exact on the lattice
G = {2: (_m64([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]]), 2.0),
     4: (_m64([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]]), 24.0)}
AT = {2: _m64([[1, 1, 1, 0], [0, 1, -1, -1]]),
      4: _m64([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]])}


def _mat(table, m, absolute):
    return table[m].abs() if absolute else table[m]


def input_transform(case, x, m, absolute=False):
    """V = B^T d B of every (m + 2)^2 patch -> [n][cin][phase][tile row][tile column][m + 2][m + 2].  An atrous layer is a dense
    3x3 problem on each of its dil x dil phases, whose pixels lie dil apart; every phase gets phase_tiles(case, m) tiles, zeros
    outside the map."""
    d, (pt, pl), (ty, tx) = case.dil, case.pad, phase_tiles(case, m)
    x = x.double().abs() if absolute else x.double()
    rows, cols = (ty * m + 2) * d, (tx * m + 2) * d                  # of the padded map: ty * m + 2 rows of every phase
    xp = F.pad(x, (pl, cols - pl - case.w, pt, rows - pt - case.h))
    bt = _mat(BT, m, absolute)
    out = []
    for py in range(d):
        for px in range(d):
            sub = xp[:, :, py::d, px::d]
            patches = sub.unfold(2, m + 2, m).unfold(3, m + 2, m)       # [n][cin][ty][tx][m + 2][m + 2]
            assert patches.shape[2:4] == (ty, tx)
            out.append(torch.einsum("ia,nctsab,jb->nctsij", bt, patches, bt))
    return torch.stack(out, 2)


def filter_transform(w, m, absolute=False):
    """U = G g G^T -> [cout][cin][m + 2][m + 2]."""
    g, den = G[m]
    g = g.abs() if absolute else g
    w = w.double().abs() if absolute else w.double()
    return torch.einsum("ia,ocab,jb->ocij", g, w, g) / (den * den)


def multiply(v, u):
    """M = sum over cin of V .* U -> [n][cout][phase][tile row][tile column][m + 2][m + 2]."""
    return torch.einsum("ncptsij,ocij->noptsij", v, u)


def tile_transform(case, mm, m, absolute=False):
    """A^T M A of every tile, the pixels past the map included -> [n][cout][phase][tile rows * m][tile columns * m]."""
    ty, tx = phase_tiles(case, m)
    at = _mat(AT, m, absolute)
    y = torch.einsum("ai,noptsij,bj->noptasb", at, mm.abs() if absolute else mm, at)      # [n][cout][phase][ty][m][tx][m]
    return y.reshape(y.shape[0], y.shape[1], case.dil * case.dil, ty * m, tx * m)


def output_transform(case, mm, m, absolute=False):
    """Y = A^T M A, every tile's m x m pixels put back into the map of their phase -> NCHW [n][cout][ho][wo]."""
    d, (ho, wo) = case.dil, out_extent(case)
    y = tile_transform(case, mm, m, absolute)
    out = torch.zeros(y.shape[:2] + (ho, wo), dtype=torch.float64)
    for py in range(d):
        for px in range(d):
            rows, cols = _cdiv(ho - py, d), _cdiv(wo - px, d)
            out[:, :, py::d, px::d] = y[:, :, py * d + px, :rows, :cols]
    return out


def winograd(case, x, w, m):
    """The convolution by F(m x m, 3x3) in float64."""
    return output_transform(case, multiply(input_transform(case, x, m), filter_transform(w, m)), m)


def _extras(data):
    e = data.b.double().abs().view(1, -1, 1, 1)
    return e + data.res.double().abs() if data.res is not None else e


def magnitudes(case, data, m):
    """-> (M_abs = sum_k V_abs * U_abs per component, tile and cout;  Y_abs = |A^T| |M| |A| + |bias| + |res| with the true M, NCHW;
    the largest |A^T| |M| |A| of any tile pixel, those past the map included: the kernels compute them as well, and they bound the
    first pass of the output transform)."""
    m_abs = multiply(input_transform(case, data.x, m, True), filter_transform(data.w, m, True))
    m_true = multiply(input_transform(case, data.x, m), filter_transform(data.w, m))
    return m_abs, output_transform(case, m_true, m, True) + _extras(data), tile_transform(case, m_true, m, True).max().item()


def bound_scale(case, data, m):
    """S_w = |A^T| (sum_k V_abs * U_abs) |A| + |b| + |res| of the derived bound, NCHW."""
    m_abs = multiply(input_transform(case, data.x, m, True), filter_transform(data.w, m, True))
    return output_transform(case, m_abs, m, True) + _extras(data)


if __name__ == "__main__":                   # python tests/conv_wino_cases.py: per kernel, the launches that run it
    for kernel, ids in instances().items():
        print(f"{kernel}  {', '.join(ids) if ids else 'NOTHING'}")
