"""Every kernel instance behind premvos_dwconv3x3_f32 (csrc/refine_ops.hip), launched directly, against float64.

The cases are tests/dwconv_cases.py; tests/test_cpu_dwconv_cover.py proves that they reach every instance the dispatcher can pick, and
each case asserts here, through premvos_dwconv3x3_variant, that it launched the instance the table names.

Reference: F.conv2d in float64 (groups = c) on exactly the float32 wgt[9][c_pad] / bias[c_pad] the kernel is handed, explicit zero
padding from pt / pl.  Tolerance, derived and not tuned: the kernel adds the bias and nine products in fp32, ten roundings on the longest
path whether or not a product is fused into its add, so with u = 2^-24, element by element,
    |got - ref| <= 10u / (1 - 10u) * (|b| + sum |w| |x|),
the right side being the float64 conv of |x| with |w|; ReLU on either side is 1-Lipschitz and keeps the bound.

Also here: the S8 store of every instance against the bf16 hi + lo split of the same call's plain output (exact), the bits of the
instances against each other (exact), non-finite inputs, channel windows of wider buffers with a sentinel around them, and the three
small kernels of the same file / the ASPP head that had one toy shape each (bilinear resize, pixel broadcast, global average pool).

`python tests/dwconv_cases.py` prints, per variant code, the cases that launch it.

What the file found: dwconv3x3_kernel (per-pixel) added the bias after the nine taps while the row and tile kernels start from it, so
its bits differed from theirs wherever the last rounding fell differently; test_interior_bits_agree_across_tile_row_and_per_pixel_kernels
("per-pixel kernel" sub-map) and test_interior_bits_agree_between_dilated_tile_and_per_pixel_kernel compare exactly that, and the
kernel now starts from the bias too.

Mutations the file is meant to catch, each made by hand in a scratch copy of refine_ops.hip (none of them moves a load or a store
out of bounds), and the tests aimed at them:
  col_ok of the 5x5 tile bounded by w - 1 instead of w   -> test_case_matches_float64...[t55-*], the "5x5 tile" sub-maps of the
                                                            interior / border tests
  ox0 without its (tx % dil) residue                     -> test_case_matches_float64...[*-r2 / r3 / r4 / r5 / r6 / r12] (outputs of the
                                                            other residues keep the sentinel), the dilated interior test
  store_unit sending the other half (odd ? lo : h)       -> the S8 comparison of every case with an even number of 4-channel units
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dwconv_cases as D
from conv_exact import round_up as _r
from conv_exact_device import bits as _bits, ops as _lib_ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 12345678.0                        # exactly representable; compared bit for bit


def _inputs(case, seed=None, n=None):
    """x [n][h][w][c_pad], wgt [9][c_pad], bias [c_pad] in float32; channels c .. c_pad are zero, as the packer leaves them."""
    g = torch.Generator().manual_seed(sum(map(ord, case.id)) if seed is None else seed)
    cp = D.c_pad(case)
    n = case.n if n is None else n
    x = torch.randn((n, case.h, case.w, cp), generator=g)
    wgt = torch.randn((9, cp), generator=g) * 0.4
    bias = torch.randn((cp,), generator=g) * 0.5
    x[..., case.c:], wgt[:, case.c:], bias[case.c:] = 0, 0, 0
    return x, wgt, bias


def _reference(case, x, wgt, bias, act):
    """-> (ref, bound) float64 [n][ho][wo][c_pad]"""
    ho, wo = D.out_extent(case)
    s, r = case.stride, case.rate
    cp = x.shape[-1]
    pb = max(0, (ho - 1) * s + 2 * r + 1 - case.pt - case.h)
    pr = max(0, (wo - 1) * s + 2 * r + 1 - case.pl - case.w)
    xd = x.double().permute(0, 3, 1, 2)
    if case.pre_relu:
        xd = F.relu(xd)
    xd = F.pad(xd, (case.pl, pr, case.pt, pb))
    k = wgt.double().t().reshape(cp, 1, 3, 3)
    ref = F.conv2d(xd, k, bias.double(), stride=s, dilation=r, groups=cp)[:, :, :ho, :wo]
    mag = F.conv2d(xd.abs(), k.abs(), bias.double().abs(), stride=s, dilation=r, groups=cp)[:, :, :ho, :wo]
    if act & D.RELU:
        ref = F.relu(ref)
    return ref.permute(0, 2, 3, 1).contiguous(), (10 * U / (1 - 10 * U) * mag).permute(0, 2, 3, 1).contiguous()


def _run(case, x, wgt, bias, act, windows=True):
    """Launch the case on ``x``; -> (the output's channel window [n][ho][wo][c_pad] float32 on the host -- an S8 output decoded into
    (hi, lo) --, and asserts that everything around the window kept the sentinel and that the whole input buffer kept its bits)."""
    _lib, lib, ops = _lib_ops()
    n, cp = x.shape[0], x.shape[-1]
    ho, wo = D.out_extent(case)
    s8 = bool(act & D.S8)
    in_ps, in_off = (case.win_in if windows and case.win_in else (cp, 0))
    out_ps, out_off = (case.win_out if windows and case.win_out else (cp, 0))
    if s8:                                   # an S8 window starts on a group of 8 channels, in a pixel of whole groups
        out_off, width = _r(out_off, 8), _r(cp, 8)
        out_ps = width if out_ps == cp else _r(out_ps, 8) + 8
    else:
        width = cp
    xin = torch.full((n, case.h, case.w, in_ps), SENTINEL, device="cuda")
    xin[..., in_off:in_off + cp] = x.cuda()
    before = xin.clone()
    out = torch.full((n, ho, wo, out_ps), SENTINEL, device="cuda")
    wd, bd = wgt.cuda(), bias.cuda()
    _lib.check(lib.premvos_dwconv3x3_f32(xin.data_ptr() + 4 * in_off, in_ps, n, case.h, case.w, case.c, wd.data_ptr(), bd.data_ptr(), cp,
                                         out.data_ptr() + 4 * out_off, out_ps, ho, wo, case.stride, case.rate, case.pt, case.pl,
                                         case.pre_relu, act, _lib.current_stream()), "dwconv3x3")
    torch.cuda.synchronize()
    assert torch.equal(_bits(xin), _bits(before)), f"{case.id}: the input buffer was written"    # the window and the channels around it
    out = out.cpu()
    sent = _bits(torch.tensor([SENTINEL]))[0].item()
    outside = torch.cat([_bits(out[..., :out_off]), _bits(out[..., out_off + width:])], -1)
    assert torch.all(outside == sent), f"{case.id}: channels outside the output window were written"
    win = out[..., out_off:out_off + width].contiguous()
    if not s8:
        return win
    raw = win.view(torch.bfloat16).view(n, ho, wo, -1, 2, 8)
    if cp % 8:                               # an odd number of 4-channel units: the last unit owns half of its group, the other half stays
        keep = torch.full((1, 8), SENTINEL).view(torch.bfloat16).view(2, 8)[:, 4:]
        assert torch.equal(raw[..., -1, :, 4:].contiguous().view(torch.int16), keep.contiguous().view(torch.int16).expand(n, ho, wo, 2, 4)), case.id
    raw = raw.float()
    return raw[..., 0, :].reshape(n, ho, wo, -1)[..., :cp], raw[..., 1, :].reshape(n, ho, wo, -1)[..., :cp]


def _check_against_reference(case, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{case.id}: max |got - ref| = {err.max().item():.3e}, worst error / bound = {ratio:.3f}")
    bad = err > bound
    assert not bool(bad.any()), (case.id, D.describe(D.expected_code(case)), int(bad.sum()), bad.nonzero()[:4].tolist(), ratio)


@pytest.mark.parametrize("case", D.CASES, ids=[c.id for c in D.CASES])
def test_case_matches_float64_and_its_s8_store_is_the_split_of_the_plain_one(case):
    _lib, lib, ops = _lib_ops()
    plain_act = case.act & ~D.S8
    assert D.query(lib, case, plain_act) == D.expected_code(case, plain_act), D.describe(D.query(lib, case, plain_act))
    x, wgt, bias = _inputs(case)
    got = _run(case, x, wgt, bias, plain_act)
    ref, bound = _reference(case, x, wgt, bias, plain_act)
    assert got.shape == ref.shape
    _check_against_reference(case, got, ref, bound)
    if case.c % 4:                           # zero weights and bias: the pad channels of the window are written as zeros
        assert got[..., case.c:].abs().max().item() == 0
    if case.act & D.S8:
        assert D.query(lib, case) == D.expected_code(case), D.describe(D.query(lib, case))
        hi, lo = _run(case, x, wgt, bias, case.act)
        want_hi = got.to(torch.bfloat16).float()
        want_lo = (got - want_hi).to(torch.bfloat16).float()
        assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo), (case.id, D.describe(D.expected_code(case)))
        assert torch.equal(hi + lo, want_hi + want_lo)


SPECIAL = [c for c in D.CASES if not c.pre_relu and c.n * c.h * c.w * c.c <= 40_000_000]       # up to the 5 x 97 x 97 x 728 case of the 8x4 tile


@pytest.mark.parametrize("case", SPECIAL, ids=[c.id for c in SPECIAL])
def test_non_finite_inputs_propagate_like_the_reference(case):
    """Without pre-ReLU, +Inf / -Inf / NaN at border and interior pixels come out exactly where float64 puts them (the comment in
    dwconv3x3_tile_kernel promises it); a masked-off tap whose register holds anything must not reach an accumulator."""
    assert len(SPECIAL) >= 20 and "t48-97x97x728" in [c.id for c in SPECIAL]
    x, wgt, bias = _inputs(case, seed=7)
    h, w, c = case.h, case.w, case.c
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (0, w // 2), (h // 2, 0), (h - 1, w // 3), (h // 3, w - 1)]
    vals = [float("inf"), float("-inf"), float("nan")]
    for i, (y, xx) in enumerate(spots):
        x[i % x.shape[0], y, xx, (5 * i) % c] = vals[i % 3]
        x[(i + 1) % x.shape[0], y, xx, (3 * i + 1) % c] = vals[(i + 1) % 3]
    got = _run(case, x, wgt, bias, 0)
    ref, _ = _reference(case, x, wgt, bias, 0)
    assert bool(torch.isnan(ref).any()) or bool(torch.isinf(ref).any())
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), case.id
    assert torch.equal(torch.isposinf(got), torch.isposinf(ref)) and torch.equal(torch.isneginf(got), torch.isneginf(ref)), case.id
    fin = torch.isfinite(ref)
    _, bound = _reference(case, torch.where(torch.isfinite(x), x, torch.zeros(())), wgt, bias, 0)
    assert bool(((got.double() - ref).abs()[fin] <= bound[fin]).all())


# ------------------------------------------------------------------------------------------------ the instances against each other
def _shape(id, n, c, h, w, rate=1, pad=None, pre_relu=0, ho=None, wo=None):
    pad = rate if pad is None else pad
    return D.Case(id, n, c, h, w, 1, rate, pad, pad, pre_relu, 0, None, None, ho, wo, None)


@pytest.mark.parametrize("c,h,w,pre,small,large", [(2048, 9, 9, 0, 2, 86), (64, 193, 193, 1, 2, 16), (304, 97, 97, 0, 1, 20)])
def test_batch_invariance_across_the_4x4_and_8x4_tiles(c, h, w, pre, small, large):
    """The wide layers switch between 4x4 and 8x4 tiles with the number of crop slots in a launch; the byte-identical output tree at
    any rank count and chunking rests on the two writing the same bits: the leading images of a large launch equal the small launch."""
    _lib, lib, ops = _lib_ops()
    case = _shape(f"batch-{h}x{w}x{c}", large, c, h, w, pre_relu=pre)
    va, vb = D.query(lib, case, n=small), D.query(lib, case, n=large)
    assert (va, vb) == (D.code(D.TILE, 4, 4, 1, pre, 1, D.F32), D.code(D.TILE, 4, 8, 1, pre, 1, D.F32)), (D.describe(va), D.describe(vb))
    x, wgt, bias = _inputs(case)
    a = _run(case, x[:small].contiguous(), wgt, bias, 0)
    b = _run(case, x, wgt, bias, 0)
    assert torch.equal(a, b[:small])


@pytest.mark.parametrize("pre", [0, 1])
def test_interior_bits_agree_across_tile_row_and_per_pixel_kernels(pre):
    """"Identical bits" of the kernel comments: a map run with pt = pl = 1 through the 4x4 tile, and sub-maps of it run with
    pt = pl = 0 through the 5x5 tile, the row kernel and the per-pixel kernel, agree on the interior they share -- same taps, same
    order (bias first, then the taps in (ky, kx) order), so no tolerance."""
    _lib, lib, ops = _lib_ops()
    full = _shape("interior-33x36", 2, 16, 33, 36, pre_relu=pre)
    assert D.query(lib, full) == D.code(D.TILE, 4, 4, 1, pre, 1, D.F32)
    x, wgt, bias = _inputs(full)
    y = _run(full, x, wgt, bias, 0)
    y0, x0 = 3, 5
    for name, hh, ww, want in (("5x5 tile", 10, 10, D.code(D.TILE, 5, 5, 1, pre, 1, D.F32)), ("row kernel", 5, 12, D.code(D.ROW, 4, 1, 0, pre, 1, D.F32)),
                               ("per-pixel kernel", 9, 7, D.code(D.PIXEL, 1, 1, 0, pre, 0, D.F32)),
                               ("4x4 tile", 9, 11, D.code(D.TILE, 4, 4, 1, pre, 1, D.F32))):
        sub = _shape(name, 2, 16, hh + 2, ww + 2, pad=0, pre_relu=pre)
        assert D.out_extent(sub) == (hh, ww) and D.query(lib, sub) == want, (name, D.describe(D.query(lib, sub)))
        got = _run(sub, x[:, y0:y0 + hh + 2, x0:x0 + ww + 2].contiguous(), wgt, bias, 0)
        assert torch.equal(got, y[:, y0 + 1:y0 + 1 + hh, x0 + 1:x0 + 1 + ww]), f"{name} differs from the 4x4 tile in the interior"


@pytest.mark.parametrize("pre", [0, 1])
def test_border_bits_agree_across_tile_row_and_per_pixel_kernels(pre):
    """The same at the borders of the map.  There the kernels differ in form: the tile and row kernels add 0 * k for a tap outside the
    map, the per-pixel kernel skips it.  acc + (+-0) = acc for every acc but -0, and an accumulator that starts from a non-zero bias
    does not pass through -0 (a sum that cancels exactly gives +0), so the bits agree there too.  The top-left corner of the 4x4-tiled
    map (pt = pl = 1) and its bottom-right corner (pt = pl = 0, the last output row and column read the zeros behind the map) are run
    as maps of their own through the 5x5 tile, the row kernel and the per-pixel kernel."""
    _lib, lib, ops = _lib_ops()
    H, W = 33, 36
    full = _shape("border-33x36", 2, 16, H, W, pre_relu=pre)
    assert D.query(lib, full) == D.code(D.TILE, 4, 4, 1, pre, 1, D.F32)
    x, wgt, bias = _inputs(full)
    assert bool((bias != 0).all())
    y = _run(full, x, wgt, bias, 0)
    for name, hh, ww, want in (("5x5 tile", 10, 10, D.code(D.TILE, 5, 5, 1, pre, 1, D.F32)), ("row kernel", 5, 12, D.code(D.ROW, 4, 1, 0, pre, 1, D.F32)),
                               ("per-pixel kernel", 9, 7, D.code(D.PIXEL, 1, 1, 0, pre, 0, D.F32))):
        # top-left: rows / columns 0 .. hh / ww of the map behind one row / column of zeros give the outputs 0 .. hh-1 / ww-1
        sub = _shape(name, 2, 16, hh + 1, ww + 1, pad=1, pre_relu=pre, ho=hh, wo=ww)
        assert D.query(lib, sub) == want, (name, D.describe(D.query(lib, sub)))
        got = _run(sub, x[:, :hh + 1, :ww + 1].contiguous(), wgt, bias, 0)
        assert torch.equal(got, y[:, :hh, :ww]), f"{name} differs from the 4x4 tile at the top-left border"
        # bottom-right: the last hh + 1 rows / ww + 1 columns, no zeros in front, give the last hh / ww outputs
        sub = _shape(name, 2, 16, hh + 1, ww + 1, pad=0, pre_relu=pre, ho=hh, wo=ww)
        assert D.query(lib, sub) == want, (name, D.describe(D.query(lib, sub)))
        got = _run(sub, x[:, H - hh - 1:, W - ww - 1:].contiguous(), wgt, bias, 0)
        assert torch.equal(got, y[:, H - hh:, W - ww:]), f"{name} differs from the 4x4 tile at the bottom-right border"


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("rate,hh,tile_ahead", [(6, 7, 0), (2, 4, 1), (18, 5, 0)])
def test_interior_bits_agree_between_dilated_tile_and_per_pixel_kernel(rate, hh, tile_ahead, pre):
    _lib, lib, ops = _lib_ops()
    size = 61 if rate == 18 else 25
    full = _shape(f"interior-r{rate}", 2, 16, size, size, rate=rate, pre_relu=pre)
    assert D.query(lib, full) == D.code(D.TILE, 4, 4, tile_ahead, pre, 1, D.F32), D.describe(D.query(lib, full))
    x, wgt, bias = _inputs(full)
    y = _run(full, x, wgt, bias, 0)
    y0, x0 = 2, 1
    sub = _shape(f"interior-r{rate}-sub", 2, 16, hh + 2 * rate, hh + 2 * rate, rate=rate, pad=0, pre_relu=pre)
    assert D.out_extent(sub) == (hh, hh) and D.query(lib, sub) == D.code(D.PIXEL, 1, 1, 0, pre, 0, D.F32)
    got = _run(sub, x[:, y0:y0 + hh + 2 * rate, x0:x0 + hh + 2 * rate].contiguous(), wgt, bias, 0)
    assert torch.equal(got, y[:, y0 + rate:y0 + rate + hh, x0 + rate:x0 + rate + hh])


# ------------------------------------------------------------------------------------------------ companions
def _tf_coords(out_size, in_size, align):
    """tf.image.resize_bilinear (TF1) source coordinates, computed in float32 as TF and the kernel do."""
    scale = (np.float32(in_size - 1) / np.float32(out_size - 1)) if (align and out_size > 1) else (np.float32(in_size) / np.float32(out_size))
    s = np.arange(out_size, dtype=np.float32) * scale
    assert s.dtype == np.float32
    f = np.floor(s)
    lo = f.astype(np.int64)
    hi = np.minimum(np.ceil(s).astype(np.int64), in_size - 1)
    return lo, hi, (s - f).astype(np.float64)


@pytest.mark.parametrize("n,h,w,c,ho,wo,align,win_in,win_out", [
    (2, 25, 25, 256, 97, 97, 1, (256, 0), (304, 0)),        # the production call: ASPP output into channels [0, 256) of the decoder concat
    (1, 13, 31, 8, 40, 17, 1, (12, 4), (16, 4)),            # non-square, up in one axis and down in the other
    (2, 49, 49, 16, 25, 25, 0, (16, 0), (24, 8)),           # downscale
    (2, 49, 49, 16, 25, 25, 1, (24, 4), (16, 0)),
    (1, 97, 97, 8, 97, 97, 1, (8, 0), (8, 0)),              # identity size (the logits resize of the decoder)
    (1, 9, 11, 8, 1, 5, 1, (8, 0), (12, 0)),                # ho = 1: align_corners falls back to in / out on that axis
    (1, 9, 11, 8, 1, 5, 0, (8, 0), (12, 4)),
    (1, 20, 20, 4, 33, 47, 0, (8, 4), (4, 0)),
    (3, 25, 25, 12, 97, 97, 0, (12, 0), (20, 4)),
])
def test_resize_bilinear_against_float64_interpolation(n, h, w, c, ho, wo, align, win_in, win_out):
    """Source coordinates in float32 (as TF computes them), interpolation in float64.  Tolerance: one lerp a + (b - a) * t is three
    fp32 roundings, error <= |a| u + |b - a| t g3 <= M (u + 2 g3) with g3 = 3u / (1 - 3u) and M = max |input|; the third lerp
    passes the two first errors on as a convex combination of them and adds its own on operands of magnitude <= M + e1:
    |got - ref| <= e1 + (M + e1)(u + 2 g3), e1 = M (u + 2 g3)."""
    _lib, lib, ops = _lib_ops()
    x = torch.randn((n, h, w, c), generator=torch.Generator().manual_seed(h * w + ho))
    (in_ps, in_off), (out_ps, out_off) = win_in, win_out
    xin = torch.full((n, h, w, in_ps), SENTINEL, device="cuda")
    xin[..., in_off:in_off + c] = x.cuda()
    out = torch.full((n, ho, wo, out_ps), SENTINEL, device="cuda")
    _lib.check(lib.premvos_resize_bilinear_f32(xin.data_ptr() + 4 * in_off, in_ps, n, h, w, c, out.data_ptr() + 4 * out_off, out_ps, ho, wo,
                                               align, _lib.current_stream()), "resize")
    torch.cuda.synchronize()
    out = out.cpu()
    ylo, yhi, ty = _tf_coords(ho, h, align)
    xlo, xhi, tx = _tf_coords(wo, w, align)
    xd = x.double().numpy()
    tx_, ty_ = tx[None, None, :, None], ty[None, :, None, None]
    top = xd[:, ylo][:, :, xlo] + (xd[:, ylo][:, :, xhi] - xd[:, ylo][:, :, xlo]) * tx_
    bot = xd[:, yhi][:, :, xlo] + (xd[:, yhi][:, :, xhi] - xd[:, yhi][:, :, xlo]) * tx_
    ref = top + (bot - top) * ty_
    g3 = 3 * U / (1 - 3 * U)
    m = float(np.abs(xd).max())
    e1 = m * (U + 2 * g3)
    tol = e1 + (m + e1) * (U + 2 * g3)
    err = np.abs(out[..., out_off:out_off + c].double().numpy() - ref).max()
    print(f"resize {h}x{w}->{ho}x{wo} align {align}: max err {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    sent = _bits(torch.tensor([SENTINEL]))[0].item()
    assert torch.all(_bits(out[..., :out_off]) == sent) and torch.all(_bits(out[..., out_off + c:]) == sent)
    if (h, w) == (ho, wo) and align:
        assert torch.equal(out[..., out_off:out_off + c], x)


@pytest.mark.parametrize("c", [256, 2048])
def test_broadcast_pixel_is_bit_exact_inside_its_window(c):
    _lib, lib, ops = _lib_ops()
    n, h, w, in_ps, in_off, out_ps, out_off = 3, 25, 25, c + 8, 4, c + 48, 8
    x = torch.randn((n, c), generator=torch.Generator().manual_seed(c))
    xin = torch.full((n, in_ps), SENTINEL, device="cuda")
    xin[:, in_off:in_off + c] = x.cuda()
    out = torch.full((n, h, w, out_ps), SENTINEL, device="cuda")
    _lib.check(lib.premvos_broadcast_pixel_f32(xin.data_ptr() + 4 * in_off, in_ps, n, c, out.data_ptr() + 4 * out_off, out_ps, h, w,
                                               _lib.current_stream()), "broadcast")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(_bits(out[..., out_off:out_off + c]), _bits(x.view(n, 1, 1, c).expand(n, h, w, c)))
    sent = _bits(torch.tensor([SENTINEL]))[0].item()
    assert torch.all(_bits(out[..., :out_off]) == sent) and torch.all(_bits(out[..., out_off + c:]) == sent)


@pytest.mark.parametrize("c", [256, 2048])
def test_global_avgpool_inside_windows(c):
    """hw - 1 additions in any order and one division: |got - ref| <= g_hw * mean |x|, g_hw = hw u / (1 - hw u)."""
    _lib, lib, ops = _lib_ops()
    n, hw, in_ps, in_off, out_ps, out_off = 3, 625, c + 8, 4, c + 16, 8
    x = torch.randn((n, hw, c), generator=torch.Generator().manual_seed(c + 1)) + 0.25
    xin = torch.full((n, hw, in_ps), SENTINEL, device="cuda")
    xin[..., in_off:in_off + c] = x.cuda()
    out = torch.full((n, out_ps), SENTINEL, device="cuda")
    _lib.check(lib.premvos_global_avgpool_f32(xin.data_ptr() + 4 * in_off, in_ps, n, hw, c, out.data_ptr() + 4 * out_off, out_ps,
                                              _lib.current_stream()), "gap")
    torch.cuda.synchronize()
    out = out.cpu()
    ref = x.double().mean(dim=1)
    bound = hw * U / (1 - hw * U) * x.double().abs().mean(dim=1)
    assert bool(((out[:, out_off:out_off + c].double() - ref).abs() <= bound).all())
    sent = _bits(torch.tensor([SENTINEL]))[0].item()
    assert torch.all(_bits(out[:, :out_off]) == sent) and torch.all(_bits(out[:, out_off + c:]) == sent)
