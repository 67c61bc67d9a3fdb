"""The kit of the exact-coordinate resampling tests (tests/resample_exact.py) and its case tables, proven without a GPU: the tables agree
with the oracle, every flip case has a flip that is visible in the data, every value bound is at least ten times below the effect of a
half-pixel error, every class exemption stays under its cap, and the float64 references agree with the oracle's own float32 path."""
from fractions import Fraction
from functools import partial

import numpy as np
import pytest
import torch

import refine_tta_restated as T
import resample_exact as K
from oracle import refinement_oracle as R
from oracle import reid_oracle as RR

HALF = partial(K.exact_table, shift=Fraction(1, 2))


def _ratios():
    """Every (out, in, align) a case of the tables resamples by."""
    out = set()
    for n, c, h, w, ho, wo, _, _, aligns in K.RESIZE_CASES:
        for a in aligns:
            out |= {(ho, h, a), (wo, w, a)}
    for S, H, W, _, boxes, _ in K.INPUT_CASES:
        for b in boxes:
            y0, x0, y1, x1 = R.crop_box(b, H, W)
            if y1 > y0 and x1 > x0:
                out |= {(S, y1 - y0, 0), (S, x1 - x0, 0)}
    for c in K.OUTPUT_CASES.values():
        out |= {(c["S"], c["lh"], 0), (c["S"], c["lw"], 0)}
        for y0, x0, y1, x1 in c["crops"]:
            if y1 > y0 and x1 > x0:
                out |= {(y1 - y0, c["S"], 0), (x1 - x0, c["S"], 0)}
    for (inn, o) in K.FLIPS:
        out.add((o, inn, 0))
    return sorted(out)


def test_the_tables_agree_with_the_oracle_outside_the_flip_sets():
    ratios = _ratios()
    assert len(ratios) > 40
    for out, inn, align in ratios:
        lo, hi, t = K.f32_table(out, inn, align)
        olo, ohi, ot = R._lerp_idx(out, inn, bool(align))
        assert np.array_equal(lo, olo) and np.array_equal(hi, ohi) and np.array_equal(t, ot)
        elo, ehi, et = K.exact_table(out, inn, align)
        a, b = K.ratio(out, inn, align)
        assert all(elo[d] == d * a // b and ehi[d] == min(-(-d * a // b), inn - 1) for d in range(out))
        keep = np.ones(out, bool)
        keep[K.flip_set(out, inn, align)] = False
        s = np.arange(out) * (a / b)
        assert np.array_equal(lo[keep], elo[keep]) and np.array_equal(hi[keep], ehi[keep]), (out, inn, align)
        assert (np.abs(t.astype(np.float64) - et)[keep] <= 2.0 ** -23 * s[keep] * (1 + 1e-6)).all(), (out, inn, align)
        assert (lo[~keep] == elo[~keep] - 1).all()                      # a flip is always one DOWN
        if not align:
            near = K.f32_nearest(out, inn)
            assert np.array_equal(near, np.minimum(lo, inn - 1))
            assert np.array_equal(K.exact_nearest(out, inn), np.minimum(elo, inn - 1))
            x = torch.arange(inn * 3, dtype=torch.float32).view(1, 1, inn, 3)
            assert torch.equal(R.resize_nearest_tf(x, out, 3)[0, 0], x[0, 0][near])


def test_the_flip_sets_are_the_listed_ones():
    for (inn, out), want in K.FLIPS.items():
        assert K.flip_set(out, inn) == want and want, (inn, out)
    # extents of one S with a flip, as counted for the crop sizes the nets run at (small S: the complete list)
    assert [i for i in range(1, 200) if K.flip_set(33, i)] == [39, 77, 78, 154, 156, 189]
    assert [o for o in range(1, 260) if K.flip_set(o, 33)] == [209, 243]
    up = [i for i in range(1, 970) if K.flip_set(385, i)]
    down = [o for o in range(1, 970) if K.flip_set(o, 385)]
    assert len(up) == 34 and up[:10] == [7, 14, 28, 56, 63, 112, 126, 145, 203, 224]
    assert len(down) == 31 and down[:7] == [95, 161, 165, 190, 297, 322, 330] and len(K.flip_set(165, 385)) == 7
    # the ratios the project's older tests resample by have none
    for inn, out in ((25, 97), (97, 385), (33, 25), (33, 41), (9, 33), (385, 289), (385, 481)):
        assert K.flip_set(out, inn) == [] and K.flip_set(out, inn, True) == []


def test_every_flip_case_has_a_flip():
    for n, c, h, w, ho, wo, _, _, aligns in K.RESIZE_FLIP_CASES:
        assert aligns == (0,) and (K.flip_set(ho, h) or K.flip_set(wo, w))
    kinds = 0
    for S, H, W, _, boxes, kind in K.INPUT_CASES:
        assert len(boxes) == len(kind)
        for b, k in zip(boxes, kind):
            y0, x0, y1, x1 = R.crop_box(b, H, W)
            if k == "flip":
                kinds += 1
                assert K.flip_set(S, y1 - y0) and K.flip_set(S, x1 - x0)
            elif k == "benign":
                assert not K.flip_set(S, y1 - y0) and not K.flip_set(S, x1 - x0)
            elif k == "empty":
                assert y1 <= y0 or x1 <= x0
    assert kinds == 3
    assert R.crop_box(K.INPUT_CASES[0][4][0], 39, 78) == (0, 0, 39, 78)                       # the whole frame
    assert R.crop_box(K.INPUT_CASES[2][4][0], 120, 200) == (0, 0, 112, 126) and R.crop_box(K.INPUT_CASES[2][4][2], 120, 200) == (8, 74, 120, 200)
    for (case, i) in K.MASK_FLIPS:
        c = K.OUTPUT_CASES[case]
        y0, x0, y1, x1 = c["crops"][i]
        assert K.flip_set(y1 - y0, c["S"]) or K.flip_set(x1 - x0, c["S"])
    y0, x0, y1, x1 = K.OUTPUT_CASES["checker385"]["crops"][1]
    assert K.flip_set(y1 - y0, 385) and K.flip_set(x1 - x0, 385)                              # height 95 and width 190


def test_the_flips_are_visible_in_the_guidance():
    counts = []
    for S, H, W, _, boxes, kind in K.INPUT_CASES:
        for b, k in zip(boxes, kind):
            if k == "flip":
                f, e = K.guidance01(H, W, b, S), K.guidance01(H, W, b, S, K.exact_nearest)
                counts.append(int((f != e).sum()))
                assert 0 < f.sum() < f.size
    # S = 385: the flipped sources of box (8, 10, 62, 76), rows 15|16, 31|32, 63|64 and columns 53|54, 89|90, 107|108 of the crop, lie on one
    # side of every edge of that box, so its guidance cannot show them; box (58, 124, 72, 164) has the same crop extents 112 x 126 with
    # its bottom and right edges ON flipped sources
    assert counts == [29, 0, 171], counts


def test_the_flips_are_visible_in_the_mask():
    for (case, i), want in K.MASK_FLIPS.items():
        c = K.OUTPUT_CASES[case]
        _, cls, d = K.class_map_f32(K.output_logits(case)[i], c["S"])
        yy, xx = np.mgrid[:c["S"], :c["S"]]
        assert np.array_equal(cls.numpy(), ((yy + xx) % 2 == 0).astype(np.uint8)) and float(d.abs().min()) >= 1.0   # the checkerboard itself
        f = K.uncrop_map(cls, c["crops"][i], c["H"], c["W"])
        e = K.uncrop_map(cls, c["crops"][i], c["H"], c["W"], K.exact_nearest)
        assert int((f != e).sum()) == want, (case, i, int((f != e).sum()))
        assert np.array_equal(f, T.uncrop(torch.zeros(c["S"], c["S"]), cls, c["crops"][i], c["H"], c["W"])[0])
    c = K.OUTPUT_CASES["checker385"]
    cls = K.class_map_f32(K.output_logits("checker385")[1], 385)[1]
    assert (K.uncrop_map(cls, c["crops"][1], 120, 200) != K.uncrop_map(cls, c["crops"][1], 120, 200, K.exact_nearest)).sum() >= 1


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------------

def test_value_bound_is_the_formula():
    assert K.value_bound(3.0, 5.0, 0.5, 0.25, 2.0) == 2.0 ** -23 * (3.0 * 0.5 + 5.0 * 0.25) + 16 * 2.0 ** -24 * 2.0
    assert K.adjacent(np.array([[0.0, 3.0], [1.0, 1.0]]), 0) == 2.0 and K.adjacent(np.zeros((1, 4)), 0) == 0.0
    assert K.s_max(13, 5) == 12 * 5 / 13 and K.s_max(13, 5, True) == 4.0 and K.s_max(1, 6, True) == 0.0


def test_the_resize_bounds_discriminate():
    for case in K.RESIZE_CASES:
        n, c, h, w, ho, wo = case[:6]
        for align in case[8]:
            x = K.resize_data(case, align)
            bound = K.resize_bound(x, ho, wo, align)
            assert bound < 1e-4
            if h == 1 and w == 1:
                continue            # a single source pixel has no neighbour to slide to: every output is that pixel, compared bit for bit
            moved = np.abs(K.bilinear_ref(x, ho, wo, align, HALF) - K.bilinear_ref(x, ho, wo, align)).max()
            assert moved >= 10 * bound, (case, align, moved, bound)
            assert np.abs(K.resize_f32(x, ho, wo, align) - K.bilinear_ref(x, ho, wo, align)).max() <= bound


def test_the_input_bounds_discriminate():
    for S, H, W, seed, boxes, kind in K.INPUT_CASES:
        img = K.frame_u8(seed, H, W)
        for b, k in zip(boxes, kind):
            ref, crop = K.refine_input_ref(img, b, S)
            bound = K.refine_input_bound(img, b, S)
            if k == "empty":
                assert bound == 0.0 and not ref.any()
                continue
            moved = np.abs(K.refine_input_ref(img, b, S, HALF)[0] - ref).max()
            assert 0 < bound < 1e-4 and moved >= 10 * bound, (S, b, moved, bound)
            f32, fcrop = K.refine_input_f32(img, b, S)
            assert fcrop == crop and np.abs(f32[..., :3] - ref).max() <= bound


def test_the_output_bounds_discriminate():
    for name, c in K.OUTPUT_CASES.items():
        lg = K.output_logits(name)
        for i, crop in enumerate(c["crops"]):
            ref = K.refine_output_ref(lg[i], crop, c["S"], c["H"], c["W"])[0]
            bound = K.refine_output_bound(lg[i], crop, c["S"])
            if crop[2] <= crop[0] or crop[3] <= crop[1]:
                assert bound == 0.0 and not ref.any()
                continue
            moved = np.abs(K.refine_output_ref(lg[i], crop, c["S"], c["H"], c["W"], HALF)[0] - ref).max()
            assert 0 < bound < 1e-3 and moved >= 10 * bound, (name, i, moved, bound)
            assert np.abs(K.refine_output_f32(lg[i], crop, c["S"], c["H"], c["W"])[1] - ref).max() <= bound


def test_the_reid_bounds_discriminate():
    cases = [(K.reid_byte_frame(), (0, 0, 16, 16))] + [(K.frame_u8(41, 40, 56), b) for b in K.REID_SMALL_BOXES + K.REID_CLIP_BOXES[:2]]
    cases.append((K.frame_u8(42, 120, 200), K.REID_DOWN_BOX))
    for img, box in cases:
        for zs in (0, 1):
            ref = K.reid_crop_ref(img, box, K.REID_S, zs)
            bound = K.reid_bound(img, box, K.REID_S, zs)
            if zs and min(box[2:]) <= 10:
                assert np.array_equal(ref, np.broadcast_to((0 - K.MEAN) / K.STD, ref.shape))
                continue
            moved = np.abs(K.reid_crop_ref(img, box, K.REID_S, zs, HALF) - ref).max()
            assert bound < 1e-4 and moved >= 10 * bound, (box, zs, moved, bound)
            assert np.abs(K.reid_crop_f32(img, box, K.REID_S, zs) - ref).max() <= bound


def test_the_class_exemptions_stay_under_their_cap():
    for name, c in K.OUTPUT_CASES.items():
        lg = K.output_logits(name)
        for i, crop in enumerate(c["crops"]):
            mask, _, exempt = K.refine_output_f32(lg[i], crop, c["S"], c["H"], c["W"], c["margin"])
            if c["margin"] is None:
                assert exempt.sum() == 0
                d = K.class_map_f32(lg[i], c["S"])[2]
                assert float(d.abs().min()) >= 1.0                      # and none is needed: no pixel is near a tie
            else:
                assert exempt.sum() <= K.EXEMPT_CAP * exempt.size, (name, i, int(exempt.sum()))
                assert 0 < mask.sum() < (crop[2] - crop[0]) * (crop[3] - crop[1])              # (both classes inside the crop)


def test_the_two_byte_scalings_differ():
    b = np.arange(256)
    feed, batch = K.reid_bytes_f32(b, 1), K.reid_bytes_f32(b, 0)
    assert feed.dtype == batch.dtype == np.float32
    assert int((feed != batch).sum()) == 126                              # 49 % of the byte values, by one ulp
    assert np.abs(feed.astype(np.float64) - batch).max() <= 2.0 ** -24


# ---- the float64 references against the oracle, on benign ratios -----------------------------------------------------------------------------

def test_the_input_reference_agrees_with_the_oracle():
    img, box = K.frame_u8(5, 120, 200), [20.4, 30.5, 90.6, 150.5]
    x, crop = R.make_input(img, box)
    want = R.deeplab_preprocess(x)[0].permute(1, 2, 0).numpy()
    assert not K.flip_set(385, crop[2] - crop[0]) and not K.flip_set(385, crop[3] - crop[1])
    f32, fcrop = K.refine_input_f32(img, box, 385)
    assert fcrop == crop and np.array_equal(f32, want)                   # the free-size restatement IS the oracle at 385
    ref, rcrop = K.refine_input_ref(img, box, 385)
    assert rcrop == crop and np.abs(ref - want[..., :3]).max() <= K.refine_input_bound(img, box, 385)
    assert np.array_equal(2 * K.guidance01(120, 200, box, 385, K.exact_nearest) - 1, want[..., 3])


def test_the_output_reference_agrees_with_the_oracle():
    lg = torch.randn((1, 2, 97, 97), generator=torch.Generator().manual_seed(3)) * 3
    crop, H, W = (10, 20, 100, 190), 120, 200
    assert not K.flip_set(90, 385) and not K.flip_set(170, 385) and not K.flip_set(385, 97)
    mask, post = R.output_layer(lg, crop, H, W)
    nhwc = lg[0].permute(1, 2, 0).numpy()
    fm, fp, _ = K.refine_output_f32(nhwc, crop, 385, H, W)
    assert np.array_equal(fm, mask) and np.array_equal(fp, post)
    ref = K.refine_output_ref(nhwc, crop, 385, H, W)[0]
    assert np.abs(ref - post).max() <= K.refine_output_bound(nhwc, crop, 385)
    assert abs(K.conf_ref(mask, post) - float(R.conf_score(mask, post))) < 1e-6


def test_the_reid_reference_agrees_with_the_oracle():
    img = K.frame_u8(6, 120, 200)
    for box, feed in (((30, 5, 100, 110), True), ((150, 80, 80, 60), False), ((0, 0, 8, 30), True)):
        want = RR.make_crop(img, box, feed)
        assert np.array_equal(K.reid_crop_f32(img, box, 128, int(feed)), want)
        assert np.abs(K.reid_crop_ref(img, box, 128, int(feed)) - want).max() <= K.reid_bound(img, box, 128, int(feed))
