"""The per-object largest-component clean-up restated with scipy: the rule of ReID_net/scripts/postproc/postproc.py:41-63
(``postproc_posteriors_connected_components``), run per object id on ``res = (M == k)``.  Written from the rule, not from the kernels
(csrc/components_ops.hip), which are held to it exactly.

    per id k >= 1 present in the id map M (uint8 [H,W]), independently of the other ids:
    res    = (M == k)
    dil    = scipy.ndimage.grey_dilation(res, size=(D, D))            D = 100: a box clipped to the frame, one further up / left when D is even
    comp   = scipy.ndimage.label(dil, structure=ones((3, 3)))         8-connected, numbered in raster order of each component's first pixel
                                                                      (the reference's skimage.measure.label, default connectivity)
    count  = pixels of res per component; the largest wins, a strict ``>`` over c = 1 .. n: a tie goes to the lowest number
    M'     = M with the pixels of res outside the winner set to 0     (freed pixels become background, never another object)

numpy and scipy only; nothing here imports the package."""
import numpy as np
from scipy import ndimage

DILATE = 100                                                                  # postproc.py:43
EIGHT = np.ones((3, 3), np.int32)
SEED = 2                                                                      # of the tests' synthetic maps: the fixture conditions hold for it
SYNTHETIC = [(37, 53, 3, 1), (37, 53, 3, 4), (37, 53, 3, 5), (70, 150, 4, 16), (130, 260, 17, 9)]      # H, W, L, D of the tests' cases


def dilate(res, D=DILATE):
    """bool / uint8 [H,W] -> uint8 [H,W]: postproc.py:43 with a box of D x D."""
    return ndimage.grey_dilation(np.asarray(res).astype(np.uint8), size=(D, D)).astype(np.uint8)


def components(mask):
    """[H,W] (non-zero = set) -> (int32 [H,W] numbered from 1 in raster order of the first pixel, 0 = background; the number n)."""
    comp, n = ndimage.label(np.asarray(mask) != 0, structure=EIGHT)
    return comp.astype(np.int32), int(n)


def min_index_labels(mask):
    """[H,W] -> int32 [H,W]: every pixel's component as the smallest linear index y * W + x inside it, -1 on background (scipy's numbering
    made canonical: what premvos_cc_label_i32 writes)."""
    comp, n = components(mask)
    flat = comp.reshape(-1)
    first = np.full(n + 1, flat.size, np.int64)
    idx = np.flatnonzero(flat)
    np.minimum.at(first, flat[idx], idx)
    first[0] = -1
    out = first[flat].reshape(comp.shape).astype(np.int32)
    assert n == 0 or (np.diff(first[1:]) > 0).all()                           # raster order of the first pixel IS the order of the roots
    return out


def keep_largest(idmap, L=None, D=DILATE):
    """uint8 [H,W] -> {"idmap": uint8 [H,W], "removed": int64 [L-1], "components": int64 [L-1]} (entry k-1: object id k; L = 1 + the largest
    id when not given; an id >= L is left alone)."""
    M = np.asarray(idmap, np.uint8)
    L = 1 + int(M.max()) if L is None else int(L)
    out = M.copy()
    removed, ncomp = np.zeros(max(L - 1, 0), np.int64), np.zeros(max(L - 1, 0), np.int64)
    for k in range(1, L):
        res = M == k
        if not res.any():
            continue
        comp, n = components(dilate(res, D))
        comp[~res] = 0                                                        # postproc.py:45
        largest, largest_count = 0, 0
        for c in range(1, n + 1):                                             # postproc.py:48-54
            count = int((comp == c).sum())
            if count > largest_count:
                largest, largest_count = c, count
        drop = res & (comp != largest)
        out[drop] = 0
        removed[k - 1], ncomp[k - 1] = int(drop.sum()), n
    return {"idmap": out, "removed": removed, "components": ncomp}


def synthetic(H, W, L, seed, blobs=3, speckle=0.01):
    """uint8 [H,W] with ids 0 .. L-1: per object ``blobs`` ellipses of decreasing size at random places (later objects paint over earlier
    ones, which cuts slivers), then ``speckle`` of the pixels set to a random id >= 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    M = np.zeros((H, W), np.uint8)
    scale = min(H, W) / (2.0 * np.sqrt(L))
    for k in range(1, L):
        for b in range(blobs):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = (scale * rng.uniform(0.5, 1.0) / (1 + b) + 1.0 for _ in range(2))
            M[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = k
    noise = rng.random((H, W)) < speckle
    M[noise] = rng.integers(1, L, int(noise.sum()), dtype=np.uint8)
    return M


def hand_cases():
    """name -> (id map, D, the expected map, removed of id 1, components of id 1): the issue's hand-made cases, each run with scipy."""
    out = {}
    M = np.zeros((20, 30), np.uint8)
    M[2:5, 20:23] = M[10:13, 3:6] = 1
    keep = M.copy()
    keep[10:13, 3:6] = 0
    out["two_blobs_D3"] = (M, 3, keep, 9, 2)                                  # a tie of 9 pixels: the first in raster order is kept
    M = np.zeros((40, 60), np.uint8)
    M[3:5, 25:27] = M[5:7, 2:4] = 1                                           # A above and right of B, 4 pixels each
    keep_a, keep_b = M.copy(), M.copy()
    keep_a[5:7, 2:4] = 0
    keep_b[3:5, 25:27] = 0
    out["clipped_tie_D1"] = (M, 1, keep_a, 4, 2)
    out["clipped_tie_D20"] = (M, 20, keep_b, 4, 2)                            # both boxes are clipped to row 0, B's starts at column 0
    for D in (4, 5):
        for d in (D - 1, D, D + 1):
            M = np.zeros((9, 40), np.uint8)
            M[4, 10] = M[4, 10 + d] = 1
            keep = M.copy()
            if d > D:
                keep[4, 10 + d] = 0
            out[f"gap_D{D}_d{d}"] = (M, D, keep, int(d > D), 1 + int(d > D))
    M = np.zeros((40, 260), np.uint8)
    M[10:14, 5:10] = M[20:24, 70:75] = M[15:21, 230:236] = 1                  # 20 + 20 pixels 65 columns apart, and 36 pixels far away
    small, big = M.copy(), M.copy()
    small[15:21, 230:236] = 0
    big[:, :100] = 0
    out["far_blobs_D60"] = (M, 60, big, 40, 3)
    out["far_blobs_D61"] = (M, 61, small, 36, 2)
    out["far_blobs_D100"] = (M, 100, small, 36, 2)
    return out
