"""A numpy restatement of MergeTrack's two diagnostics: ``viz_scores`` (merge_functions.py:547-611) with scipy.misc.imsave's bytescale,
and print_max_reid_distance.py.  The CPU yardstick of csrc/viz_ops.hip: its float canvas is pinned against the reference EXECUTED
(tests/golden/viz_ref.npz, tools/make_golden_viz.py) by tests/test_cpu_viz.py, then used by tests/test_gpu_viz.py on inputs the
fixture does not hold.

UNPINNED, restated from memory of scipy 1.0 / 1.1 (scipy.misc.imsave does not exist in the scipy installed here): ``bytescale``.  cv2's
resize is oracle/cv_resize_oracle.py's restatement, unpinned as everywhere in this project.

Rules of this package's own, which the reference does not have or where it would raise: a crop is clipped to the frame
(a negative origin to 0) and an empty one gives a black tile; a box with a non-finite number gives a black tile; a non-finite weighted
score counts as 0 (for the marks a non-finite gt too); a non-finite plane or gt value makes non-finite red and green values (numpy's
own arithmetic; blue stays 0), which bytescale leaves out of the extremes and writes as 0."""
import os

import numpy as np

from oracle.cv_resize_oracle import resize_linear_u8

BOX = 100
ALPHA = 0.3
MAX_REID_DISTANCE = 25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viz_ref.npz")


def load_fixture():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def colour(s):
    """A score's colour on the float canvas: red for 0, green for 1 (merge_functions.py:547-551 times the 255 of :590)."""
    return np.array([(1 - s) * 255, s * 255, 0.0])


def tile_of(frame, mask, box, tint):
    """The top row's tile of one candidate, uint8 [100,100,3] (merge_functions.py:569-583, draw_mask :527-537 with alpha 0.3)."""
    frame = np.asarray(frame)
    hh, ww = frame.shape[:2]
    black = np.zeros((BOX, BOX, 3), np.uint8)
    if not np.all(np.isfinite(np.asarray(box, np.float64))):
        return black
    x, y, w, h = (int(np.clip(v, -2.0 ** 30, 2.0 ** 30)) for v in box)      # int(): truncation toward zero
    if min(h, w) < 2:
        return black
    x0, y0 = min(max(x, 0), ww), min(max(y, 0), hh)
    x1, y1 = min(max(x + w - 1, 0), ww), min(max(y + h - 1, 0), hh)
    if x1 - x0 < 1 or y1 - y0 < 1:
        return black
    picture = resize_linear_u8(np.ascontiguousarray(frame[y0:y1, x0:x1, :]), BOX, BOX)
    inside = (np.asarray(mask)[y0:y1, x0:x1] != 0).astype(np.uint8)
    inside = resize_linear_u8(np.ascontiguousarray(inside[:, :, None]), BOX, BOX)[:, :, 0] > 0
    tinted = (picture * (1 - ALPHA) + np.asarray(tint).astype(np.float64) * ALPHA).astype(np.uint8)      # float64, then truncation
    return np.where(inside[:, :, None], tinted, picture)


def marks_of(weighted, gt):
    """-> (argmax of the weighted rows, argmax of the gt rows): first maxima over the P candidates, non-finite = 0."""
    ws, g = np.array(weighted, np.float64), np.array(gt, np.float64)
    ws[~np.isfinite(ws)] = 0
    g[~np.isfinite(g)] = 0
    return ws.argmax(axis=1), g.argmax(axis=1)


def score_tile(planes5, weighted, gt, mark_weighted, mark_gt):
    """Template i's tile under candidate j, float64 [100,100,3]: the five planes stacked in the left half (20 rows each), the weighted
    score top right, gt bottom right; row 0 and column 0 are the separators; a black 25 x 25 mark at rows / columns 12 .. 37 of the
    right half's upper (weighted) or lower (gt) cell (merge_functions.py:584-609)."""
    tile = np.zeros((BOX, BOX, 3))
    half, fifth, lo, hi = BOX // 2, BOX // 5, BOX // 8, BOX // 4 + BOX // 8
    for k in range(5):
        tile[fifth * k:fifth * (k + 1), :half] = colour(planes5[k])
    tile[:half, half:] = colour(weighted)
    tile[half:, half:] = colour(gt)
    tile[0, :] = 0
    tile[:, 0] = 0
    if mark_weighted:
        tile[lo:hi, half + lo:half + hi] = 0
    if mark_gt:
        tile[half + lo:half + hi, half + lo:half + hi] = 0
    return tile


def float_sheet(frame, masks, boxes, planes, weighted, gt, tint):
    """The float64 canvas viz_scores hands to imsave: [100 (T + 1), 100 P, 3].  ``weighted`` [T,P] (or [T,P+1]: the last column is not
    read), ``gt`` [T,P] (the reference's ``gt_scores[0]``).  A non-finite plane or gt value gives non-finite red and green (numpy's own
    arithmetic; blue stays 0)."""
    planes, gt = np.asarray(planes, np.float64), np.asarray(gt, np.float64)
    T, P = gt.shape
    ws = np.array(weighted, np.float64)[:, :P]
    ws[~np.isfinite(ws)] = 0
    best_w, best_g = marks_of(ws, gt)
    sheet = np.zeros((BOX * (T + 1), BOX * P, 3))
    with np.errstate(invalid="ignore"):
        for j in range(P):
            crop = tile_of(frame, masks[j], boxes[j], tint).astype(np.float64)
            crop[:, 0] = 0                                                      # the column separator runs through the top row too
            sheet[:BOX, BOX * j:BOX * (j + 1)] = crop
            for i in range(T):
                sheet[BOX * (i + 1):BOX * (i + 2), BOX * j:BOX * (j + 1)] = score_tile(planes[:, i, j], ws[i, j], gt[i, j], j == best_w[i], j == best_g[i])
    return sheet


def bytescale(data):
    """scipy.misc.bytescale(data) as toimage calls it for a float array (cmin / cmax = the array's own extremes, low 0, high 255); a
    non-finite value (this package's rule) stays out of the extremes and becomes 0."""
    data = np.asarray(data, np.float64)
    ok = np.isfinite(data)
    cmin, cmax = data[ok].min(), data[ok].max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    scale = float(255 - 0) / cscale
    bytedata = (np.where(ok, data, cmin) - cmin) * scale + 0
    out = (bytedata.clip(0, 255) + 0.5).astype(np.uint8)
    out[~ok] = 0
    return out


def sheet_u8(frame, masks, boxes, planes, weighted, gt, tint):
    """The uint8 picture imsave codes: what premvos_viz_scores_u8 writes."""
    return bytescale(float_sheet(frame, masks, boxes, planes, weighted, gt, tint))


# ----------------------------------------------------------------------------------------------------- print_max_reid_distance.py
def max_distances_program(templates, frames):
    """print_max_reid_distance.py:40-48: ``templates`` [T,128], ``frames`` a list of [F,128] arrays, one per frame -> per template the
    largest distance over all frames; an infinite distance counts as 0, a frame without proposals contributes zeros."""
    t = np.asarray(templates, np.float64).reshape(-1, 128)
    best = []
    for cur in frames:
        cur = np.asarray(cur, np.float64).reshape(-1, 128)
        if len(cur) == 0:
            best.append(np.zeros(len(t)))
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            dist = np.array([[np.linalg.norm(c - row) for c in cur] for row in t])
        dist[np.isinf(dist)] = 0
        best.append(dist.max(axis=1))
    return np.max(np.array(best), axis=0)


def max_distances_ordered(templates, pooled):
    """The kernel's order: squares summed over the embedding index ascending (np.cumsum adds sequentially), one correctly rounded
    square root, inf -> 0, a maximum that starts at 0 and that a NaN wins.  -> (max [T], how many of each row exceed 25 [T])."""
    t = np.asarray(templates, np.float64).reshape(-1, 128)
    p = np.asarray(pooled, np.float64).reshape(-1, 128)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[None, :, :] - t[:, None, :]
        dist = np.sqrt(np.cumsum(d * d, axis=2)[:, :, -1]) if p.shape[0] else np.zeros((t.shape[0], 0))
    dist[np.isinf(dist)] = 0
    best = np.concatenate([np.zeros((t.shape[0], 1)), dist], axis=1).max(axis=1)             # (np.max: a NaN wins)
    return best, (dist > MAX_REID_DISTANCE).sum(axis=1).astype(np.int64)
