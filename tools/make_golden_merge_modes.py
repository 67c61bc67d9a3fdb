"""Generates tests/golden/merge_modes_ref.npz by IMPORTING AND EXECUTING MergeTrack/merge_functions.py (unmodified): direct calls of
``calculate_gt_scores`` (merge_functions.py:78-94) and ``probabilitic_combination`` (merge_functions.py:151-195) on crafted inputs.
The stand-ins for what the build image lacks are those of tools/make_golden_track.py (its ``install()``); no import of premvos_amd.
``probabilitic_combination`` prints its probabilities and returns only the masks: the module's ``print`` is given a recorder, the
file is not touched.

A condition, not a measurement: the package takes the argmax WITHOUT the function's second softmax (monotone), so a fixture in which
some pixel's two largest values of [background, objects] are unequal but less than 1e-9 apart is refused.  Arrays only.
Usage: python tools/make_golden_merge_modes.py <PReMVOS checkout>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden_track as GT  # noqa: E402  (reads the checkout's place from sys.argv[1], like this file)

GAP = 1e-9
H, W = 24, 32


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[:h, :w]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.uint8)


def props_of(masks):
    return [{"segmentation": GT.seg_str(m), "score": 0.9} for m in masks]


def gap_check(tag, masks, ws):
    """The reference's own expressions up to probs_incl_background (merge_functions.py:156-169), for the 1e-9 condition only."""
    p = np.exp(ws / 0.1)
    p = p / p.sum(axis=1)[:, np.newaxis]
    m = np.repeat(masks.astype(np.float32)[np.newaxis], [p.shape[0]], axis=0)
    pe = np.repeat(np.repeat(p[:, :, np.newaxis], [m.shape[2]], axis=2)[:, :, :, np.newaxis], m.shape[3], axis=3)
    comb = np.average(m, axis=1, weights=pe)
    full = np.append(1 - comb.max(axis=0)[np.newaxis], comb, axis=0)
    srt = np.sort(full, axis=0)
    d = srt[-1] - srt[-2]
    bad = int(np.count_nonzero((d != 0) & (d < GAP)))
    if bad:
        raise SystemExit(f"{tag}: {bad} pixels whose two largest values are unequal but closer than {GAP}: change the inputs")
    nz = d[d != 0]
    return float(nz.min()) if nz.size else np.inf


def main():
    M, MF = GT.install()
    printed = []
    MF.print = lambda *a, **k: printed.append(np.array(a[0], np.float64))        # the function's print(probs_over_proposals)
    rng = np.random.default_rng(11)
    arrays, gaps = {}, {}

    def case(tag, masks, ws, label_map):
        masks = np.asarray(masks, np.uint8)
        T, P = ws.shape
        assert masks.shape[0] == P
        templates = [{"id": t + 1} for t in range(T)]
        gaps[tag] = gap_check(tag, masks, ws)
        del printed[:]
        out = MF.probabilitic_combination(props_of(masks), ws.copy(), templates, 1e-10)
        assert len(printed) == 1 and printed[0].shape == (T, P)
        gt_props = [{"id": int(i), "segmentation": GT.seg_str((label_map == i).astype(np.uint8))} for i in np.unique(label_map) if i != 0]
        planes = MF.calculate_gt_scores(props_of(masks), gt_props, templates)
        assert planes.shape == (5, T, P)
        arrays.update({f"{tag}_masks": masks, f"{tag}_weighted": ws, f"{tag}_labels": label_map.astype(np.uint8),
                       f"{tag}_probs": printed[0], f"{tag}_out_masks": np.array([p["mask"] for p in out], np.uint8),
                       f"{tag}_out_ids": np.array([p["id"] for p in out], np.int64),
                       f"{tag}_out_final_score": np.array([p["final_score"] for p in out], np.float64),
                       f"{tag}_out_bbox": np.array([p["bbox"] for p in out], np.float64), f"{tag}_gt_planes": planes})

    # T = 1, P = 1
    m = ellipse(H, W, 12, 15, 6, 9)[None]
    lab = ellipse(H, W, 11, 17, 7, 8)
    case("t1p1", m, np.array([[0.62]]), lab)
    # T = 1, P = 2, equal scores: a pixel one of the two covers is 0.5 against a background of 0.5 -> background; both: 1 -> object
    m = np.array([ellipse(H, W, 10, 10, 6, 7), ellipse(H, W, 13, 18, 6, 8)])
    case("tie", m, np.array([[0.5, 0.5]]), m[0].copy())
    # T = 3, P = 6, ellipses; the annotation holds all three objects
    m = np.array([ellipse(H, W, 7, 8, 5, 6), ellipse(H, W, 15, 20, 6, 8), ellipse(H, W, 12, 14, 4, 10), ellipse(H, W, 8, 9, 4, 6),
                  ellipse(H, W, 16, 22, 5, 6), ellipse(H, W, 20, 6, 3, 5)])
    lab = np.zeros((H, W), np.uint8)
    for i, e in enumerate((ellipse(H, W, 7, 8, 5, 5), ellipse(H, W, 15, 21, 6, 7), ellipse(H, W, 12, 14, 3, 8))):
        lab[e != 0] = i + 1
    ws = np.round(rng.uniform(0.05, 0.95, (3, 6)), 3)
    case("t3p6", m, ws, lab)
    # a proposal that covers the whole frame, an all-empty one; the annotation lacks object 2
    m4 = np.array([np.ones((H, W), np.uint8), np.zeros((H, W), np.uint8), m[0], m[1], m[2]])
    lab2 = lab.copy()
    lab2[lab2 == 2] = 0
    case("edge", m4, np.round(rng.uniform(0.05, 0.95, (3, 5)), 3), lab2)
    assert not arrays["edge_gt_planes"][:, 1].any() and arrays["t3p6_gt_planes"][:, 1].any()
    arrays["smallest_gaps"] = np.array([gaps[k] for k in sorted(gaps)])
    fn = os.path.join(GT.GOLD, "merge_modes_ref.npz")
    np.savez_compressed(fn, **arrays)
    print(f"{fn}: {os.path.getsize(fn)} bytes; smallest non-zero top-two gaps {gaps}")


if __name__ == "__main__":
    main()
