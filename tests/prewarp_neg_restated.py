"""MergeTrack/oldmerge.py with ``use_ff_negative_props = True`` (oldmerge.py:43, get_negative_ff_props :63-85, its use at :137-138,147),
restated in numpy on the plain arrays of tests/prewarp_restated.py: the yardstick of premvos_prewarp_negatives_i32 and of the chain and
paint entries with trailing negative templates.  tests/test_cpu_prewarp_neg.py holds it against what the reference itself computed
(tests/golden/prewarp_neg_ref.npz).

Templates = the annotated objects of the whole video in frame order, THEN the negatives in acceptance order (oldmerge.py:138).  A
negative starts on its own mask (:147), is forced in no frame (:168-174 covers annotated objects only), keeps label 0 (:148,173) and so
never shows in the PNG, but takes columns in the snapping, lowers the objects' two "other" planes and hides lower scores in the paint.

Rules of our own:
  * a candidate whose score is NaN is never taken (Python's sort has no defined order for it);
  * ``negatives`` = K: the walk stops after the K-th acceptance; "all": as the reference; None / 0: no negatives;
  * a video without annotated objects has no negatives."""
import numpy as np

import prewarp_restated as R

EMB = R.EMB


def select_negatives(masks, ann_masks, scores, K=None):
    """oldmerge.py:63-85.  ``masks`` [P,h,w] frame 0's proposals in file order, ``ann_masks`` the objects annotated in frame 0,
    ``scores`` [P]; ``K`` None = all.  -> proposal indices in acceptance order."""
    scores = np.asarray(scores, np.float64).reshape(-1)
    cand = [i for i in range(len(scores)) if not np.isnan(scores[i])]
    cand.sort(key=lambda i: scores[i], reverse=True)           # stable: equal scores keep file order (reverse=True keeps it too)
    current = [np.asarray(m) != 0 for m in ann_masks]
    taken = []
    for i in cand:
        if K is not None and len(taken) >= K:
            break
        m = np.asarray(masks[i]) != 0
        if any(int(np.count_nonzero(m & s)) > 0 for s in current):       # iou > 0 <=> the intersection has a pixel
            continue
        current.append(m)
        taken.append(i)
    return taken


def cap_of(negatives):
    """None -> off; "all" -> no cap (None); an int K >= 0 -> K"""
    assert negatives is not None
    return None if negatives == "all" else int(negatives)


def negatives_of(frames, h, w, negatives):
    if negatives is None or not any(len(f["ann"]) for f in frames) or not len(frames[0]["score"]):
        return []
    f0 = frames[0]
    P = len(f0["score"])
    return select_negatives(np.asarray(f0["mask"]).reshape(P, h, w), [o["mask"] for o in f0["ann"]], f0["score"], cap_of(negatives))


def reid_planes(frames, emb_t):
    """oldmerge.py:87-110 for the template embeddings ``emb_t`` [T,128] (prewarp_restated.reid_planes takes them from the annotations)"""
    T = len(emb_t)
    dist = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for f in frames:
            e = np.asarray(f["reid"], np.float64).reshape(-1, EMB)
            d = np.zeros((T, len(e)))
            for i in range(T):
                for j in range(len(e)):
                    d[i, j] = np.sqrt(np.sum((e[j] - emb_t[i]) ** 2))
            dist.append(d)
        mx = np.zeros(T)
        for d in dist:
            if d.shape[1]:
                dd = d.copy()
                dd[np.isinf(dd)] = 0
                mx = np.maximum(mx, dd.max(axis=1))
        reid = []
        for d in dist:
            s = 1 - d / mx[:, None]
            s[~np.isfinite(s)] = 0
            reid.append(s)
    return reid, [R.other_max_plane(s) for s in reid]


def merge_video(frames, h, w, weights=None, negatives="all"):
    """oldmerge.py:129-218 do_video with the switch on.  -> prewarp_restated.merge_video's dict over T = annotated + negatives templates,
    + "negatives" (frame-0 proposal indices in acceptance order) and "T_ann"."""
    neg = negatives_of(frames, h, w, negatives)
    ids, start, emb_ann, first = R.templates_of(frames)
    T_ann = len(ids)
    if not neg:
        out = R.merge_video(frames, h, w, weights)
        out.update(negatives=[], T_ann=T_ann)
        return out
    nw = R.normalised(weights)
    N, T = len(frames), T_ann + len(neg)
    P0 = len(frames[0]["score"])
    masks0 = np.asarray(frames[0]["mask"]).reshape(P0, h, w)
    emb_t = np.concatenate([emb_ann, np.asarray(frames[0]["reid"], np.float64).reshape(P0, EMB)[neg]])
    reid, oreid = reid_planes(frames, emb_t)
    empty = np.zeros((h, w), np.uint8)
    flat = [o for f in frames for o in f["ann"]]
    cur = [np.asarray(flat[k]["mask"]) if start[k] == 0 else empty for k in range(T_ann)] + [masks0[i] for i in neg]
    labels = np.zeros(T, np.int64)
    out = {"planes": [], "weighted": [], "chosen": np.full((N, T), -1, np.int64), "best": np.zeros((N, T)),
           "index": np.zeros((N, h, w), np.uint8), "idmap": np.zeros((N, h, w), np.uint8), "negatives": list(neg), "T_ann": T_ann}
    for t, f in enumerate(frames):
        P = len(f["score"])
        masks = np.asarray(f["mask"]).reshape(P, h, w)
        obj = np.repeat(np.asarray(f["score"], np.float64)[None, :], T, axis=0)
        warp = np.array([[R.mask_iou(masks[p], cur[k]) for p in range(P)] for k in range(T)], np.float64).reshape(T, P)
        planes = np.array([obj, reid[t], oreid[t], warp, R.other_max_plane(warp)])
        weighted = np.zeros((T, P))
        for k in range(5):
            weighted = weighted + nw[k] * planes[k]
        out["planes"].append(planes)
        out["weighted"].append(weighted.copy())
        chosen, best = np.full(T, -1, np.int64), np.zeros(T)
        if P:
            with np.errstate(invalid="ignore"):
                closest = np.argmax(weighted, axis=0)
                snapped = np.array([weighted[k] * (closest == k) for k in range(T)])
            for k in range(T):
                best[k], chosen[k] = R.first_max(snapped[k])
        for k in range(first[t], first[t + 1]):                # annotated IN this frame; a negative (k >= T_ann) is never forced
            chosen[k], best[k], labels[k] = P + k - first[t], 1.0, ids[k]
        sel = [empty if chosen[k] < 0 else masks[chosen[k]] if chosen[k] < P else np.asarray(flat[k]["mask"]) for k in range(T)]
        for k in R.paint_order(best):
            out["index"][t][sel[k] != 0] = k + 1
        for k in range(T):
            out["idmap"][t][out["index"][t] == k + 1] = labels[k]        # 0 for a negative, in every frame: it still hid lower scores
        out["chosen"][t], out["best"][t] = chosen, best
        fwd = np.asarray(f["fwd"]).reshape(P, h, w)
        cur = [empty if chosen[k] < 0 else fwd[chosen[k]] if chosen[k] < P else np.asarray(flat[k]["fwd"]) for k in range(T)]
    return out


def fixture_video(ref, g, name, late=True):
    """tests/golden/prewarp_neg_ref.npz's video ``name`` (the layout of prewarp_ref.npz: prewarp_restated.fixture_video reads it)"""
    return R.fixture_video(ref, g, name, late)
