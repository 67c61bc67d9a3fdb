"""MergeTrack/oldmerge.py:87-218 (the pre-warp merge, "PREMVOS 1 uses pre-warp") and merge_functions.py:613-634 (eval_video), restated in
numpy on plain arrays: the yardstick of premvos_amd/csrc/prewarp_ops.hip and premvos_amd/prewarp.py, in the role track_restated.py has
for the live-warp loop.  tests/test_cpu_prewarp_restated.py holds it against what the reference itself computed (tests/golden/prewarp_ref.npz).

A video is a list of frames; a frame is a dict
    "score" [P] float64, "mask" [P,h,w] uint8, "fwd" [P,h,w] uint8 (the mask warped to the next frame), "reid" [P,128] float64 (an
    all-inf row: the proposal has no 'ReID'), "ann": the objects annotated IN this frame, each {"id", "mask", "fwd", "reid"}.
T = the annotated objects of the whole video in frame order ("templates").  A selection is a column of the NEXT frame's candidate
list: p < P_t = proposal p of frame t, P_t + j = the j-th object annotated in frame t, -1 = the empty mask.

Rules of our own, none of which the fixture exercises:
  * IoU: 0 where the intersection is empty (mergetrack.mask_iou, pycocotools).
  * equal scores: the higher index paints last (np.argsort is not stable; track_paint's rule).
  * NaN follows numpy: max / argmax return the first NaN; a NaN score sorts last, so it paints last.
  * a frame without proposals (the reference raises): templates not annotated in it choose the empty mask with score 0 and carry it.
  * a non-finite ReID score is 0 (the reference zeroes the infinite ones; a NaN arises only where a template's largest distance is 0)."""
import numpy as np

EMB = 128
WEIGHTS = np.array([0.1639026729185494, 0.3090363324359478, 0.11728252456485666, 0.18345061062541546, 0.2263278594552307])   # oldmerge.py:220-221


def normalised(weights=None):
    w = np.asarray(WEIGHTS if weights is None else weights, np.float64)
    return w / np.sum(w)


def templates_of(frames):
    """-> (ids [T], start frame [T], reid [T,128], first template of each frame [N+1])"""
    ids, start, reid, first = [], [], [], [0]
    for t, f in enumerate(frames):
        for o in f["ann"]:
            ids.append(int(o["id"]))
            start.append(t)
            reid.append(np.asarray(o["reid"], np.float64))
        first.append(len(ids))
    return np.array(ids, np.int64), np.array(start, np.int64), np.array(reid, np.float64).reshape(len(ids), EMB), np.array(first, np.int64)


def other_max_plane(mat):
    """oldmerge.py:100-108 / 118-123: 1 - the maximum over the OTHER rows; all ones for a single row"""
    out = np.ones_like(mat)
    T = mat.shape[0]
    if T > 1:
        ids = np.arange(T)
        for i in ids:
            out[i, :] = 1 - np.max(np.atleast_2d(mat[ids != i, :]), axis=0)
    return out


def reid_planes(frames):
    """oldmerge.py:87-110 -> (reid [N] of [T,P_t], inverse reid [N] of [T,P_t])"""
    _, _, emb_t, _ = templates_of(frames)
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
                mx = np.maximum(mx, dd.max(axis=1))            # (np.maximum and .max both hand a NaN on)
        reid = []
        for d in dist:
            s = 1 - d / mx[:, None]
            s[~np.isfinite(s)] = 0
            reid.append(s)
    return reid, [other_max_plane(s) for s in reid]


def mask_iou(a, b):
    inter = int(np.count_nonzero((a != 0) & (b != 0)))
    return inter / int(np.count_nonzero((a != 0) | (b != 0))) if inter else 0.0


def first_max(v):
    """numpy's max / argmax of a 1-D array: the first NaN if there is one, else the first maximum"""
    i = int(np.argmax(v))
    return v[i], i


def paint_order(best):
    """ascending score, equal scores by index, NaN last: the LAST entry is painted last (on top)"""
    key = np.where(np.isnan(best), np.inf, best)
    return sorted(range(len(best)), key=lambda i: (key[i], i))


def merge_video(frames, h, w, weights=None):
    """oldmerge.py:129-218 do_video.  -> dict: "planes" / "weighted" per frame ([5,T,P_t] / [T,P_t], before the snapping), "chosen"
    [N,T] int64, "best" [N,T], "index" [N,h,w] (template index + 1: oldmerge.py:179-181), "idmap" [N,h,w] (what the PNG holds)."""
    nw = normalised(weights)
    ids, start, _, first = templates_of(frames)
    T, N = len(ids), len(frames)
    reid, oreid = reid_planes(frames)
    empty = np.zeros((h, w), np.uint8)
    flat = [o for f in frames for o in f["ann"]]
    cur = [np.asarray(flat[k]["mask"]) if start[k] == 0 else empty for k in range(T)]
    labels = np.zeros(T, np.int64)
    out = {"planes": [], "weighted": [], "chosen": np.full((N, T), -1, np.int64), "best": np.zeros((N, T)),
           "index": np.zeros((N, h, w), np.uint8), "idmap": np.zeros((N, h, w), np.uint8)}
    for t, f in enumerate(frames):
        P = len(f["score"])
        masks = np.asarray(f["mask"]).reshape(P, h, w)
        obj = np.repeat(np.asarray(f["score"], np.float64)[None, :], T, axis=0)
        warp = np.array([[mask_iou(masks[p], cur[k]) for p in range(P)] for k in range(T)], np.float64).reshape(T, P)
        planes = np.array([obj, reid[t], oreid[t], warp, other_max_plane(warp)])
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
                best[k], chosen[k] = first_max(snapped[k])
        for k in range(first[t], first[t + 1]):                # annotated IN this frame: the annotation itself, score exactly 1
            chosen[k], best[k], labels[k] = P + k - first[t], 1.0, ids[k]
        sel = [empty if chosen[k] < 0 else masks[chosen[k]] if chosen[k] < P else np.asarray(flat[k]["mask"]) for k in range(T)]
        for k in paint_order(best):
            out["index"][t][sel[k] != 0] = k + 1
        for k in range(T):
            out["idmap"][t][out["index"][t] == k + 1] = labels[k]        # 0 for a template not annotated yet: it still hid lower scores
        out["chosen"][t], out["best"][t] = chosen, best
        fwd = np.asarray(f["fwd"]).reshape(P, h, w)
        cur = [empty if chosen[k] < 0 else fwd[chosen[k]] if chosen[k] < P else np.asarray(flat[k]["fwd"]) for k in range(T)]
    return out


def region_counts(index, gt, T0):
    """per frame and scored object k < T0: |R and G|, |R or G|, |R| with R = (index == k + 1), G = (gt == k + 1) -> int64 [N,T0,3]"""
    N = len(index)
    c = np.zeros((N, T0, 3), np.int64)
    for t in range(N):
        for k in range(T0):
            r, g = index[t] == k + 1, gt[t] == k + 1
            c[t, k] = np.count_nonzero(r & g), np.count_nonzero(r | g), np.count_nonzero(r)
    return c


def scores_from_counts(counts):
    """merge_functions.py:613-634 eval_video on integer counts [N,T0,3]: the mean over frames 1 .. N-2"""
    N, T0, _ = counts.shape
    scores = np.zeros(T0)
    for t in range(1, N - 1):
        for k in range(T0):
            inter, union, area = (int(x) for x in counts[t, k])
            if union - area + inter == 0:                      # |G| == 0: the id is not in this frame's annotation
                score = 1 if area == 0 else 0
            else:
                score = inter / union if inter else 0.0
            scores[k] += score
    with np.errstate(invalid="ignore", divide="ignore"):
        return scores / (N - 2)


def check_first_frame_ids(frames):
    ids = [int(o["id"]) for o in frames[0]["ann"]] if frames else []
    if ids != list(range(1, len(ids) + 1)):
        raise ValueError(f"the search scores object k against annotation id k + 1 (merge_functions.py:623): frame 0 must hold ids 1 .. T0, got {ids}")
    return len(ids)


def eval_video(index, gt, T0):
    return scores_from_counts(region_counts(index, gt, T0))


def search_weights(W, seed=0):
    """set 0 = the default weights, sets 1 .. W-1 = default_rng(seed).random(5); all normalised -> [W,5]"""
    rng = np.random.default_rng(seed)
    return np.array([normalised()] + [normalised(rng.random(5)) for _ in range(W - 1)])


def fixture_video(ref, g, name, late=True):
    """tests/golden/prewarp_ref.npz's video ``name`` as the frames list above (masks unpacked); ``late`` False: only the objects of frame 0"""
    h, w = g["h"], g["w"]
    unpack = lambda a: np.unpackbits(a, axis=-1)[..., :w]                   # noqa: E731
    mask, fwd = unpack(ref[f"v_{name}_mask"]), unpack(ref[f"v_{name}_fwd"])
    am, af, ae = unpack(ref[f"v_{name}_ann_mask"]), unpack(ref[f"v_{name}_ann_fwd"]), ref[f"v_{name}_ann_emb"]
    frames = []
    for t in range(g["videos"][name]["frames"]):
        ann = [{"id": o["id"], "mask": am[k], "fwd": af[k], "reid": ae[k]} for k, o in enumerate(g["videos"][name]["objects"])
               if o["start"] == t and (late or t == 0)]
        frames.append({"score": ref[f"v_{name}_score"][t], "mask": mask[t], "fwd": fwd[t], "reid": ref[f"v_{name}_emb"][t], "ann": ann})
    return frames
