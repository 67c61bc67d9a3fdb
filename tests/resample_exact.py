"""What the exact-coordinate tests of the resampling kernels share (csrc/refine_ops.hip: refine_input_kernel, resize_bilinear_kernel,
broadcast_kernel, seg_softmax_kernel / seg_uncrop_kernel / seg_conf_kernel; csrc/reid_ops.hip: reid_input_kernel,
reid_input_frames_kernel): source-coordinate tables in exact arithmetic and in the float32 order of the TF1 ops, float64 references
built from the exact tables only, float32-rule restatements of everything an index picks, the derived value bounds and the case
tables.  Host only: numpy, torch on the CPU, the oracles.  Everything takes the crop size S; nothing here touches
oracle.refinement_oracle.INPUT_SIZE.  Proven on the CPU by tests/test_cpu_resample_exact.py, used on the GPU by
tests/test_gpu_resample_exact.py.

Two specifications, on purpose.  Which source pixel an output pixel reads is decided by the FLOAT32 coordinate
src = float(d) * (float(in) / float(out)) (oracle.refinement_oracle._lerp_idx / resize_nearest_tf); for many crop extents floor(src) is one
lower than the exact floor(d * in / out) (``flip_set``), and the float32 one is what the reference's TF ops compute: guidance, class map,
mask and crop boxes are held to it bit for bit.  Interpolated VALUES are continuous in the coordinate, so they are held to the exact
float64 reference within ``value_bound``, which is derived below and not measured."""
from fractions import Fraction

import numpy as np
import torch

import refine_tta_restated as T
from oracle import refinement_oracle as R
from oracle import reid_oracle as RR

U = 2.0 ** -24                                   # unit roundoff of float32
MEAN = R.IMAGENET_RGB_MEAN.astype(np.float64)    # the float32 constants, promoted
STD = R.IMAGENET_RGB_STD.astype(np.float64)
TWO_255 = float(np.float32(2.0 / 255.0))
SENTINEL = -12345.0                              # float buffers; byte buffers use 0xA5, int buffers -77
SENTINEL_U8, SENTINEL_I32 = 0xA5, -77


# ---- coordinate tables -----------------------------------------------------------------------------------------------------------------

def ratio(out, inn, align=False):
    """The scale a / b as two integers: (in - 1) / (out - 1) for align-corners with out > 1, else in / out."""
    return (inn - 1, out - 1) if (align and out > 1) else (inn, out)


def exact_table(out, inn, align=False, shift=Fraction(0)):
    """(lo, hi, t) of s = d * a / b + shift in rational arithmetic: lo = floor(s), hi = min(ceil(s), in - 1), t = s - floor(s) rounded
    once to float64.  (``shift`` moves every coordinate, for the proof that a bound discriminates; lo is then clamped to in - 1.)"""
    a, b = ratio(out, inn, align)
    lo, hi, t = np.empty(out, np.int64), np.empty(out, np.int64), np.empty(out, np.float64)
    for d in range(out):
        s = Fraction(d * a, b) + shift
        f = s.numerator // s.denominator
        lo[d], hi[d], t[d] = min(f, inn - 1), min(f + (s != f), inn - 1), float(s - f)
    return lo, hi, t


def exact_nearest(out, inn):
    """min(floor(d * in / out), in - 1) in integers."""
    return np.minimum(np.arange(out, dtype=np.int64) * inn // out, inn - 1)


def f32_table(out, inn, align=False):
    """The oracle's own float32 table."""
    return R._lerp_idx(out, inn, bool(align))


def f32_nearest(out, inn):
    """The oracle's own float32 nearest rule, read off an index ramp."""
    ramp = torch.arange(inn, dtype=torch.float32).view(1, 1, inn, 1)
    return R.resize_nearest_tf(ramp, out, 1)[0, 0, :, 0].numpy().astype(np.int64)


def flip_set(out, inn, align=False):
    """Output indices whose float32 floor differs from the exact one."""
    return [int(d) for d in np.flatnonzero(f32_table(out, inn, align)[0] != exact_table(out, inn, align)[0])]


def s_max(out, inn, align=False):
    """The largest exact source coordinate."""
    a, b = ratio(out, inn, align)
    return (out - 1) * a / b


# ---- the value bound ---------------------------------------------------------------------------------------------------------------------

def value_bound(sy_max, sx_max, Dy, Dx, M):
    """How far a float32 TF1 bilinear resize may lie from the exact one: 2**-23 * (sy_max * Dy + sx_max * Dx) + 16 * 2**-24 * M.

    Coordinate.  s_f = fl(fl(d) * fl(a / b)): d, a, b are integers below 2**24, so exactly two roundings, |s_f - s| <= s * ((1 + u)**2 - 1)
    = s * (2**-23 + 2**-48), u = 2**-24.  t = s_f - floor(s_f) is exact (a float minus its own floor).  So in exact arithmetic the kernel
    evaluates the interpolant F of the source at (sy_f, sx_f) and the reference at (sy, sx).  F is continuous and piecewise linear in each
    coordinate, the clamp hi = min(ceil, in - 1) included (beyond in - 1 it is constant, the limit from the left); its slope along y is a
    convex combination of differences of vertically adjacent source values, so F is Lipschitz with constant Dy along y and Dx along x,
    D = the largest difference of adjacent source values along the axis -- ACROSS a flip of floor(s) as well: that is why values are
    tested against the exact table while indices are tested against the float32 one.  First term: sy * 2**-23 * Dy + sx * 2**-23 * Dx.

    Arithmetic.  top = tl + (tr - tl) * tx: the difference (<= 2M) rounds by 2uM, its product with tx <= 1 by 2uM, the sum (<= M) by uM:
    5uM, the same for bot.  top + (bot - top) * ty carries (1 - ty) * 5uM + ty * 5uM and adds 2uM + 2uM + uM: 10uM in first order, at most
    12uM with the second-order terms and the 2**-48 * s * D of the coordinate (s < 2**10, D <= 2M).  Rounded up to 16uM.  A contraction of
    a product and a sum into one FMA removes a rounding and stays inside."""
    return 2.0 ** -23 * (sy_max * Dy + sx_max * Dx) + 16 * U * M


def adjacent(x, axis):
    """The largest difference of adjacent values of a float64 array along ``axis`` (0 for a single line)."""
    d = np.abs(np.diff(np.asarray(x, np.float64), axis=axis))
    return float(d.max()) if d.size else 0.0


def resize_bound(x, ho, wo, align=False):
    """``value_bound`` of resizing the NHWC array x."""
    _, h, w, _ = x.shape
    return value_bound(s_max(ho, h, align), s_max(wo, w, align), adjacent(x, 1), adjacent(x, 2), float(np.abs(x).max()))


# ---- float64 references, from the exact tables only ----------------------------------------------------------------------------------------

def interp(x, ytab, xtab):
    """Bilinear gather of a float64 NHWC array by (lo, hi, t) tables."""
    (ylo, yhi, ty), (xlo, xhi, tx) = ytab, xtab
    ty, tx = ty[None, :, None, None], tx[None, None, :, None]
    top = x[:, ylo][:, :, xlo] * (1 - tx) + x[:, ylo][:, :, xhi] * tx
    bot = x[:, yhi][:, :, xlo] * (1 - tx) + x[:, yhi][:, :, xhi] * tx
    return top * (1 - ty) + bot * ty


def bilinear_ref(x, ho, wo, align=False, table=exact_table):
    """The TF1 bilinear resize of an NHWC array in float64."""
    x = np.asarray(x, np.float64)
    return interp(x, table(ho, x.shape[1], align), table(wo, x.shape[2], align))


def refine_input_ref(img_u8, box, S, table=exact_table):
    """The three image channels of the refinement net's input for one box, [S][S][3] float64, and the crop box (the oracle's
    ``crop_box``).  The normalisation chain is kept, in float64, with the float32 constants: byte / 255 -> bilinear -> (x - mean) / std
    -> (x * std + mean) * 255 -> float32(2 / 255) * x - 1.  An empty crop gives zeros."""
    h, w = img_u8.shape[:2]
    y0, x0, y1, x1 = crop = R.crop_box(box, h, w)
    if y1 <= y0 or x1 <= x0:
        return np.zeros((S, S, 3)), crop
    r = bilinear_ref(img_u8[None, y0:y1, x0:x1].astype(np.float64) / 255.0, S, S, False, table)[0]
    r = (r - MEAN) / STD
    r = (r * STD + MEAN) * 255.0
    return TWO_255 * r - 1.0, crop


def refine_input_bound(img_u8, box, S):
    """(v) for the three image channels.  The source is byte / 255 in [0, 1] (M = 1) and the output is 2r - 1, so the bilinear bound counts
    twice.  The chain's roundings in units of u, taken at r in [0, 1]: byte / 255 1 (a convex combination of four), r - mean 1,
    / std 1 (relative u of a quotient whose numerator is |r - mean| < 1), * std 1, + mean 1, * 255 1: 6, so 2 * (16 + 6) = 44 at the output;
    there float32(2 / 255) * x (<= 2) adds 2 and the - 1 (result in [-1, 1]) adds 1: 16 -> 47 in the second term.  The constants are the same
    float32 numbers in the kernel and in the reference, where the chain cancels exactly."""
    h, w = img_u8.shape[:2]
    y0, x0, y1, x1 = R.crop_box(box, h, w)
    if y1 <= y0 or x1 <= x0:
        return 0.0
    src = img_u8[y0:y1, x0:x1].astype(np.float64) / 255.0
    coord = value_bound(s_max(S, y1 - y0), s_max(S, x1 - x0), adjacent(src, 0), adjacent(src, 1), 0.0)
    return 2.0 * coord + 47 * U


def refine_output_ref(logits, crop, S, H, W, table=exact_table):
    """The posterior of SegmentationSoftmax's eval branch for one box in float64: logits [lh][lw][2] -> exact legacy bilinear to S x S ->
    softmax -> exact legacy bilinear to the crop -> zero padding.  Returns (posterior [H][W], probability [S][S], up-scaled logits)."""
    lg = bilinear_ref(np.asarray(logits, np.float64)[None, :, :, :2], S, S, False, table)[0]
    d = lg[..., 1] - lg[..., 0]
    prob = np.where(d >= 0, 1.0 / (1.0 + np.exp(-np.abs(d))), np.exp(-np.abs(d)) / (1.0 + np.exp(-np.abs(d))))
    y0, x0, y1, x1 = crop
    post = np.zeros((H, W))
    if y1 > y0 and x1 > x0:
        post[y0:y1, x0:x1] = bilinear_ref(prob[None, :, :, None], y1 - y0, x1 - x0, False, table)[0, :, :, 0]
    return post, prob, lg


def refine_output_bound(logits, crop, S):
    """(v) for the posterior: the bound twice.  The up-scaled logits lie within b1 = value_bound(logits) of the exact ones, l1 - l0 within
    2 * b1, and the softmax is the logistic function of l1 - l0, Lipschitz 1/4: b1 / 2.  The kernel's softmax itself: l - max (one of the two is
    an exact 0, the other rounds by u * |d|, |d| * sigma'(d) < 1/4), two expf of at most 1 ulp = 2u relative each (the documented accuracy
    of the device's expf), the sum u, the quotient u: p <= 1 within 8u.  A convex combination of probabilities that are off by e is off by
    at most e, so the second resize adds value_bound(exact probability map, M = 1)."""
    lg = np.asarray(logits, np.float64)[None, :, :, :2]
    y0, x0, y1, x1 = crop
    if y1 <= y0 or x1 <= x0:
        return 0.0
    b1 = resize_bound(lg, S, S)
    prob = refine_output_ref(logits, crop, S, y1, x1)[1]
    b2 = value_bound(s_max(y1 - y0, S), s_max(x1 - x0, S), adjacent(prob, 0), adjacent(prob, 1), 1.0)
    return b2 + 0.5 * b1 + 8 * U


def reid_clip(box_xywh, H, W):
    """Tensor slicing [y:y+h, x:x+w] of an H x W frame: (x0, y0, x1, y1)."""
    x, y, w, h = (int(v) for v in box_xywh)
    return max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)


def reid_crop_ref(img_u8, box_xywh, S, zero_small, table=exact_table):
    """One ReID crop [S][S][3] in float64: byte / 255 -> slice -> exact legacy bilinear -> (x - mean) / std; a box with min(w, h) <= 10
    (zero_small) or an empty slice is a zero image before the normalisation."""
    H, W = img_u8.shape[:2]
    x0, y0, x1, y1 = reid_clip(box_xywh, H, W)
    v = np.zeros((S, S, 3))
    if not (zero_small and min(int(box_xywh[2]), int(box_xywh[3])) <= 10) and x1 > x0 and y1 > y0:
        v = bilinear_ref(img_u8[None, y0:y1, x0:x1].astype(np.float64) / 255.0, S, S, False, table)[0]
    return (v - MEAN) / STD


def reid_bound(img_u8, box_xywh, S, zero_small):
    """(v) for a ReID crop.  Source in [0, 1]: byte / 255 is one rounding, byte * float32(1 / 255) two (the constant and the product);
    the bilinear bound with M = 1; v - mean one more: (coordinate + (16 + 3)u) / min(std), and the quotient (< 4 in magnitude, half an ulp
    there is 2u) adds 2u."""
    H, W = img_u8.shape[:2]
    x0, y0, x1, y1 = reid_clip(box_xywh, H, W)
    if (zero_small and min(int(box_xywh[2]), int(box_xywh[3])) <= 10) or x1 <= x0 or y1 <= y0:
        return 2 * U
    src = img_u8[y0:y1, x0:x1].astype(np.float64) / 255.0
    coord = value_bound(s_max(S, y1 - y0), s_max(S, x1 - x0), adjacent(src, 0), adjacent(src, 1), 0.0)
    return (coord + 19 * U) / float(STD.min()) + 2 * U


# ---- the float32 rule: everything an index picks, and the float32 values the project's own tolerances refer to --------------------------------

def nchw(x_nhwc):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float32))).permute(0, 3, 1, 2)


def resize_f32(x_nhwc, ho, wo, align=False):
    """The oracle's float32 resize on an NHWC array."""
    return R.resize_bilinear_tf(nchw(x_nhwc), ho, wo, bool(align)).permute(0, 2, 3, 1).numpy()


def guidance01(h, w, box, S, nearest=f32_nearest):
    """The {0, 1} guidance channel of one box at S x S (make_input's painting, BoundingBox.py:15-19, with the crop and the nearest resize
    by ``nearest``), or None for an empty crop."""
    gy0, gx0, gy1, gx1 = (int(v) for v in np.round(np.asarray(box, np.float32)))
    guid = np.zeros((h, w), np.float32)
    guid[max(gy0, 0):max(gy1, 0), max(gx0, 0):max(gx1, 0)] = 1
    y0, x0, y1, x1 = R.crop_box(box, h, w)
    if y1 <= y0 or x1 <= x0:
        return None
    return guid[y0:y1, x0:x1][nearest(S, y1 - y0)][:, nearest(S, x1 - x0)]


def refine_input_f32(img_u8, box, S):
    """``make_input`` + ``deeplab_preprocess`` of the oracle at a free crop size, from the oracle's own pieces: (net input [S][S][4] float32,
    crop box).  An empty crop gives zeros, as the kernel documents."""
    h, w = img_u8.shape[:2]
    y0, x0, y1, x1 = crop = R.crop_box(box, h, w)
    g = guidance01(h, w, box, S)
    if g is None:
        return np.zeros((S, S, 4), np.float32), crop
    img = img_u8.astype("float32") / 255
    ri = R.resize_bilinear_tf(torch.from_numpy(img[y0:y1, x0:x1]).permute(2, 0, 1)[None], S, S, False)
    ri = (ri - torch.from_numpy(R.IMAGENET_RGB_MEAN).view(1, 3, 1, 1)) / torch.from_numpy(R.IMAGENET_RGB_STD).view(1, 3, 1, 1)
    x = R.deeplab_preprocess(torch.cat([ri, torch.from_numpy(g)[None, None]], 1))
    return x[0].permute(1, 2, 0).numpy(), crop


def class_map_f32(logits, S):
    """The first half of the oracle's ``output_layer`` at a free S: logits [lh][lw][>= 2] float32 -> (probability [S][S] float32, class
    [S][S] uint8, l1 - l0 [S][S] float32), torch tensors."""
    lg = R.resize_bilinear_tf(nchw(np.asarray(logits)[None, :, :, :2]), S, S, False)
    return torch.softmax(lg, dim=1)[0, 1], lg.argmax(dim=1)[0].to(torch.uint8), (lg[0, 1] - lg[0, 0])


def uncrop_map(cls, crop, H, W, nearest=f32_nearest):
    """A [S][S] map un-cropped by a nearest rule and zero padded: the mask (with ``f32_nearest``: what refine_tta_restated.uncrop gives)."""
    cls = np.asarray(cls)
    y0, x0, y1, x1 = crop
    out = np.zeros((H, W), cls.dtype)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = cls[nearest(y1 - y0, cls.shape[0])][:, nearest(x1 - x0, cls.shape[1])]
    return out


def refine_output_f32(logits, crop, S, H, W, margin=None):
    """The float32 restatement of one box of the output layer: (mask uint8 [H][W], posterior float32 [H][W], exempt bool [H][W]).
    ``margin``: the mask pixels whose class-map source has |l1 - l0| < margin are exempt (a kernel may round l1 - l0 to the other side of
    zero there); None: nothing is."""
    prob, cls, d = class_map_f32(logits, S)
    mask, post = T.uncrop(prob, cls, crop, H, W)
    exempt = np.zeros((H, W), bool)
    if margin is not None:
        exempt = uncrop_map((d.abs() < margin).numpy(), crop, H, W).astype(bool)
    return mask, post, exempt


def conf_ref(mask, post):
    """The float64 mean of the float32 conf_score integrand (FewShotSegmentationForwarder.py:144-147): 2c - 1, c = p inside the mask, 1 - p
    outside."""
    post = np.asarray(post, np.float32)
    c = np.where(np.asarray(mask) != 0, post, np.float32(1) - post).astype(np.float32)
    return float((np.float32(2) * c - np.float32(1)).astype(np.float64).mean())


def reid_bytes_f32(b, zero_small):
    """What a byte becomes in front of the bilinear resize: float32(b) / 255 in the in-merge feed (zero_small), float32(b) * float32(1 / 255)
    in the batch stage."""
    b = np.asarray(b).astype(np.float32)
    return b / np.float32(255) if zero_small else b * np.float32(1.0 / 255.0)


def reid_crop_f32(img_u8, box_xywh, S, zero_small):
    """``reid_oracle.make_crop`` at a free size, from the oracle's own resize: [S][S][3] float32."""
    H, W = img_u8.shape[:2]
    x0, y0, x1, y1 = reid_clip(box_xywh, H, W)
    v = np.zeros((S, S, 3), np.float32)
    if not (zero_small and min(int(box_xywh[2]), int(box_xywh[3])) <= 10) and x1 > x0 and y1 > y0:
        v = RR.resize_bilinear_legacy(reid_bytes_f32(img_u8, zero_small)[y0:y1, x0:x1], S, S)
    return ((v - RR.IMAGENET_RGB_MEAN) / RR.IMAGENET_RGB_STD).astype(np.float32)


# ---- case tables: plain data, shared by the CPU and the GPU tests ----------------------------------------------------------------------------

# A. premvos_resize_bilinear_f32: (n, C, h, w, ho, wo, in_ps, out_ps, aligns)
RESIZE_CASES = [
    (3, 8, 5, 7, 13, 9, 12, 16, (0, 1)),            # non-square up-scale, channel windows
    (2, 4, 25, 25, 97, 97, 4, 4, (0, 1)),           # C = 4
    (1, 132, 9, 6, 4, 11, 132, 136, (0, 1)),        # down in y, up in x, an odd number of float4 units
    (2, 8, 1, 1, 6, 5, 8, 12, (0, 1)),              # a 1x1 source
    (2, 8, 6, 5, 1, 1, 12, 8, (0, 1)),              # align with out = 1 falls back to in / out
    (2, 8, 1, 7, 1, 7, 8, 8, (0, 1)),               # identity size: a bit-equal copy
    (1, 4, 39, 78, 33, 33, 4, 4, (0,)),             # flip ratios 39 -> 33 and 78 -> 33
    (1, 4, 33, 33, 60, 243, 4, 4, (0,)),            # flip ratio 33 -> 243
]
RESIZE_FLIP_CASES = RESIZE_CASES[6:]

# the float32 floor is one below the exact one at exactly these output indices: (in, out) -> indices
FLIPS = {
    (39, 33): [11, 22], (78, 33): [11, 22], (33, 243): [81, 162], (33, 209): [95, 171, 190],
    (112, 385): [55, 110, 220], (126, 385): [165, 275, 330],
    (385, 165): [27, 51, 54, 99, 102, 105, 108], (385, 190): [114],
}



def resize_data(case, align):
    """The float32 NHWC source [n][h][w][C] of a RESIZE_CASES entry."""
    n, c, h, w = case[:4]
    return np.random.default_rng(1000 + 2 * RESIZE_CASES.index(case) + align).standard_normal((n, h, w, c)).astype(np.float32)


# B. premvos_broadcast_pixel_f32: (n, C, h, w, in_ps, out_ps)
BROADCAST_CASE = (3, 8, 5, 7, 12, 20)

# C. premvos_refine_input_u8: (S, H, W, frame seed, boxes y0 x0 y1 x1, kind per box).  max_boxes = number of boxes + 2.
INPUT_CASES = [
    (33, 39, 78, 21, [(13, 26, 30, 60)], ["flip"]),
    (33, 120, 200, 22, [(10.4, 20.5, 110.6, 180.5), (0, 0, 120, 200), (60.5, 100.5, 61.5, 102.5), (-20.3, -5.5, 30.2, 40.4),
                        (100, 180, 140, 230), (50, 50, 50, 50), (200, 300, 220, 330)],
     ["down", "edges", "thin", "negative", "overhang", "zero-area", "empty"]),
    (385, 120, 200, 23, [(8, 10, 62, 76), (20.4, 30.5, 90.6, 150.5), (58, 124, 72, 164)], ["flip", "benign", "flip"]),
]


def frame_u8(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


# D. premvos_refine_output_f32.  kind: "checker" (l1 - l0 = +-(1 + |noise|), the sign alternating per pixel, logits at S x S: an identity
# up-scale, so the class map is the checkerboard), "smooth" (random 9 x 13 logits at pixel stride 4).  margin: the class exemption, None = no
# exemption.
OUTPUT_CASES = {
    "checker33": dict(S=33, H=60, W=260, lh=33, lw=33, ps=2, max_boxes=5, kind="checker", seed=31, margin=None,
                      crops=[(0, 0, 60, 243), (0, 17, 60, 226), (59, 259, 60, 260), (0, 0, 0, 0)]),
    "checker385": dict(S=385, H=120, W=200, lh=385, lw=385, ps=2, max_boxes=3, kind="checker", seed=32, margin=None,
                       crops=[(0, 10, 120, 175), (5, 0, 100, 190)]),
    "smooth33": dict(S=33, H=40, W=56, lh=9, lw=13, ps=4, max_boxes=3, kind="smooth", seed=33, margin=1e-4,
                     crops=[(0, 30, 25, 56), (18, 0, 40, 29)]),
    "block2000": dict(S=33, H=40, W=50, lh=33, lw=33, ps=2, max_boxes=2, kind="checker", seed=34, margin=None, crops=[(0, 0, 40, 50)]),
    "block2049": dict(S=33, H=3, W=683, lh=33, lw=33, ps=2, max_boxes=2, kind="checker", seed=35, margin=None, crops=[(0, 0, 3, 683)]),
}
EXEMPT_CAP = 0.005
# mask-flip cases: (case, box) whose un-crop extent has a flip ratio, and how many mask pixels the float32 rule and the exact rule differ on
MASK_FLIPS = {("checker33", 0): 120, ("checker33", 1): 180, ("checker385", 0): 840}


def output_logits(case):
    """float32 [max_boxes][lh][lw][ps] of an OUTPUT_CASES entry, the slots behind the boxes and the pad channels included (random: the
    kernels read every slot)."""
    c = OUTPUT_CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng(c["seed"])
    lg = rng.standard_normal((c["max_boxes"], c["lh"], c["lw"], c["ps"])).astype(np.float32)
    if c["kind"] == "checker":
        yy, xx = np.mgrid[:c["lh"], :c["lw"]]
        sign = np.where((yy + xx) % 2 == 0, 1.0, -1.0).astype(np.float32)
        noise = np.abs(rng.standard_normal((c["max_boxes"], c["lh"], c["lw"]))).astype(np.float32)
        lg[..., 1] = lg[..., 0] + sign * (np.float32(1) + noise)
    else:
        lg[..., :2] *= 2
    return lg


# E. premvos_reid_input_u8 / premvos_reid_input_frames_u8, S = 16.  Boxes are (x, y, w, h), already clipped at the origin by the host.
REID_S = 16
REID_SMALL_BOXES = [(3, 4, 10, 20), (3, 4, 20, 10), (3, 4, 11, 20), (3, 4, 20, 11)]          # min(w, h) = 10 | 11, on a 40 x 56 frame
REID_CLIP_BOXES = [(40, 20, 30, 30), (0, 30, 56, 20), (5, 5, 0, 12)]                         # over the right / bottom edge; empty
REID_DOWN_BOX = (50, 10, 100, 90)                                                            # 100 x 90 -> 16 on a 120 x 200 frame


def reid_byte_frame():
    """16 x 16 x 3: every byte value three times, each channel in another order."""
    b = np.arange(256, dtype=np.uint8)
    return np.stack([b, b[::-1], np.roll(b, 77)], 1).reshape(16, 16, 3).copy()
