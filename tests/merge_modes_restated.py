"""A numpy restatement of the two swaps merge.py imports next to its loop's functions (merge.py:50-52): ``calculate_gt_scores``
(merge_functions.py:78-94) and ``probabilitic_combination`` (merge_functions.py:151-195), and of the loop of tests/track_restated.py
with each swap applied.  The CPU yardstick of csrc/merge_modes_ops.hip: pinned against the reference EXECUTED
(tests/golden/merge_modes_ref.npz, tools/make_golden_merge_modes.py) by tests/test_cpu_merge_modes.py, then used by
tests/test_gpu_merge_modes.py on inputs the fixture does not hold.

Sums run in the kernel's fixed order (p ascending, one rounding per operation), which is also np.average's over axis 1.  Three rules
are this package's own: the oracle scores row k against annotation id k + 1 and refuses other template ids; 'id' of the
combination is the template's; the argmax is taken without the second softmax (monotone), so inputs must keep every pixel's top two
values equal or >= 1e-9 apart (``gap_violations`` counts the pixels that do not)."""
import glob
import os
from copy import deepcopy as copy

import numpy as np

import track_restated as R
from oracle import merge_oracle as MO
from premvos_amd import rle

TEMPERATURE = 0.1
GAP = 1e-9


# ------------------------------------------------------------------------------------------------------------ array level
def label_overlap(masks, labels, T):
    """-> inter int64 [T,P], area_p [P], area_l [T]: mask p (nonzero = foreground) against the pixels of ``labels`` equal to t + 1."""
    m = np.asarray(masks) != 0
    lab = np.asarray(labels)
    on = np.array([lab == t + 1 for t in range(T)]).reshape(T, *lab.shape)
    inter = np.array([[np.count_nonzero(a & b) for a in m] for b in on], np.int64).reshape(T, len(m))
    return inter, m.reshape(len(m), -1).sum(1).astype(np.int64), on.reshape(T, -1).sum(1).astype(np.int64)


def gt_planes_from_counts(inter, area_p, area_l):
    """-> float64 [5,T,P], all five the IoU; 0 where the intersection is empty (pycocotools' iou of disjoint masks)."""
    inter, area_p, area_l = np.asarray(inter, np.int64), np.asarray(area_p, np.int64), np.asarray(area_l, np.int64)
    union = np.where(inter == 0, 1, area_p[None, :] + area_l[:, None] - inter)
    iou = inter.astype(np.float64) / union.astype(np.float64)
    return np.array([iou, iou, iou, iou, iou])


def probs_from_weighted(weighted):
    """merge_functions.py:156-158, 181 on [T,P] (a non-finite score counts as 0) -> probs [T,P], denom [T] (np.average's divisor),
    best [T].  Sums over p ascending."""
    ws = np.array(weighted, np.float64)
    ws[np.logical_not(np.isfinite(ws))] = 0
    e = np.exp(ws / TEMPERATURE)
    part = np.zeros(len(ws))
    for p in range(ws.shape[1]):
        part = part + e[:, p]
    probs = e / part[:, None]
    return probs, denom_of(probs), ws.max(axis=1)


def denom_of(probs):
    d = np.zeros(len(probs))
    for p in range(probs.shape[1]):
        d = d + probs[:, p]
    return d


def combined_from_probs(masks, probs):
    """merge_functions.py:162-169 -> float64 [T+1,h,w]: background, then the objects' weighted averages (p ascending)."""
    m = np.asarray(masks) != 0
    probs = np.asarray(probs, np.float64)
    acc = np.zeros((len(probs),) + m.shape[1:])
    for p in range(len(m)):
        acc = acc + np.where(m[p][None], probs[:, p][:, None, None], 0.0)
    combined = acc / denom_of(probs)[:, None, None]
    return np.append(1.0 - combined.max(axis=0)[None], combined, axis=0)


def gap_violations(full):
    """The pixels whose two largest values of [background, objects] are unequal but less than GAP apart."""
    srt = np.sort(full, axis=0)
    d = srt[-1] - srt[-2]
    return int(np.count_nonzero((d != 0) & (d < GAP)))


def combine_from_probs(masks, probs, ids):
    """-> labels, idmap, refined (the three outputs of paint_from_arrays) and the [T+1,h,w] values the argmax was taken of."""
    full = combined_from_probs(masks, probs)
    T = len(probs)
    labels = np.argmax(full, axis=0).astype(np.uint8)                  # the first maximum: the background wins a tie
    idmap = np.zeros_like(labels)
    for t in range(T):
        idmap[labels == t + 1] = np.uint8(ids[t])
    return labels, idmap, np.array([(labels == t + 1).astype(np.uint8) for t in range(T)]).reshape((T,) + labels.shape), full


# -------------------------------------------------------------------------------------------------------------- dict level
def calculate_gt_scores(proposals, gt_props, templates):
    T = len(templates)
    pm = np.array([rle.decode(p["segmentation"]) for p in proposals])
    labels = np.zeros(pm.shape[1:], np.uint8)
    for g in gt_props:
        assert 1 <= int(g["id"]) <= T, "rule of our own: annotation ids are 1 .. T"
        labels[rle.decode(g["segmentation"]).astype(bool)] = int(g["id"])
    return gt_planes_from_counts(*label_overlap(pm, labels, T))


def probabilitic_combination(proposals, weighted_scores, templates, score_thresh):
    masks = np.array([rle.decode(p["segmentation"]) for p in proposals])
    probs, _, best = probs_from_weighted(weighted_scores)
    _, _, refined, full = combine_from_probs(masks, probs, [t["id"] for t in templates])
    out = []
    for i, t in enumerate(templates):
        seg = rle.encode(refined[i])
        out.append({"segmentation": seg, "bbox": np.array(rle.to_bbox(seg)), "final_score": best[i], "mask": refined[i], "id": t["id"]})
    return out, probs, full


def do_video(video_dir, images, anns, props, flows, do_refinement, add_ReID, combine="argmax", oracle=False):
    """tests/track_restated.py ``do_video`` with the swaps: ``oracle``: calculate_gt_scores for calculate_scores (the frame's own
    annotation is read for every frame); ``combine="probabilistic"``: probabilitic_combination for calculate_selected_props +
    remove_mask_overlap (the reference's warp_proposals would then miss 'object_score'; nothing uses it, it is carried as 0)."""
    from PIL import Image
    log, templates, next_props = [], [], []
    fns = sorted(glob.glob(video_dir + "*"))
    for k, image_fn in enumerate(fns):
        stem = os.path.splitext(os.path.relpath(image_fn, images))[0]
        ann_fn = os.path.join(anns, stem + ".png")
        if os.path.exists(ann_fn) and "00000.jpg" in image_fn:
            new = add_ReID(R.read_ann(ann_fn), image_fn, None)
            templates, next_props = templates + copy(new), next_props + copy(new)
        if not templates:
            with Image.open(image_fn) as im:
                log.append({"png": np.zeros((im.size[1], im.size[0]), np.uint8)})
            continue
        proposals = next_props + R.read_props(os.path.join(props, stem + ".json"))
        if oracle:
            assert [int(t["id"]) for t in templates] == list(range(1, len(templates) + 1)), "rule of our own: template ids are 1 .. T"
            planes = calculate_gt_scores(proposals, R.read_ann(ann_fn), templates)
        else:
            planes = R.calculate_scores(proposals, templates)
        weighted = R.weighted_from_planes(planes)
        rec = {"planes": planes, "weighted": R.select_from_weighted(weighted)[0]}
        if combine == "probabilistic":
            sel, probs, full = probabilitic_combination(proposals, weighted, templates, R.SCORE_THRESH)
            for p in sel:
                p["object_score"] = 0.0
            rec.update({"probs": probs, "gap_violations": gap_violations(full)})
        else:
            with np.errstate(invalid="ignore"):
                object_scores = planes[0] + planes[1]
            sel, index = R.calculate_selected_props(proposals, weighted, templates, R.SCORE_THRESH, object_scores)
            rec.update({"selected": index, "selected_masks": np.array([rle.decode(p["segmentation"]) for p in sel])})
            sel = R.remove_mask_overlap(sel)
        rec["final_score"] = np.array([p["final_score"] for p in sel])
        flow_fn = os.path.join(flows, stem + ".flo")
        if os.path.exists(flow_fn) and k + 1 < len(fns):
            next_props = MO.warp_proposals(sel, MO.get_flow(flow_fn), rle)
            next_props = do_refinement(next_props, fns[k + 1], None)
            next_props = add_ReID(next_props, fns[k + 1], None)
            templates = R.update_templates(templates, next_props)
        rec["png"] = R.idmap_of(sel)
        log.append(rec)
    return log


# ------------------------------------------------------------------------------------------------------------- test inputs
def ellipses(rng, h, w, n):
    """n object-like masks (one ellipse each) uint8 [n,h,w]."""
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(1, max(2.0, h / 3)), rng.uniform(1, max(2.0, w / 3))
        out[i] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


def load_fixture():
    return np.load(os.path.join(R.HERE, "golden", "merge_modes_ref.npz"))


def segs_of(masks):
    return [rle.encode(np.asarray(m, np.uint8)) for m in masks]
