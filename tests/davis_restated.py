"""The DAVIS measures of tools/davis_eval.py restated in plain numpy (no scipy: the GPU tests must run where scipy is absent):
seg2bmap, the disk dilation as an OR of shifted copies, the six integer counts premvos_davis_counts_u8 returns, the two measures
and the sequence protocol.  tests/test_cpu_davis_gpu_host.py pins this restatement to tools/davis_eval.py with ``==`` where scipy is
installed; the GPU tests then compare the kernel with it."""
import glob
import math
import os

import numpy as np


def seg2bmap(seg):
    """East, south or south-east neighbour differs; the last row / column compare with themselves; the corner never is."""
    seg = np.asarray(seg).astype(bool)
    h, w = seg.shape
    b = np.zeros((h, w), bool)
    b[:, :-1] |= seg[:, :-1] ^ seg[:, 1:]
    b[:-1, :] |= seg[:-1, :] ^ seg[1:, :]
    b[:-1, :-1] |= seg[:-1, :-1] ^ seg[1:, 1:]
    return b


def dilate_disk(b, r):
    """Binary dilation by the disk dx*dx + dy*dy <= r*r, background outside the image: the OR of the shifted copies."""
    b = np.asarray(b).astype(bool)
    h, w = b.shape
    out = np.zeros((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy > r * r or abs(dy) >= h or abs(dx) >= w:
                continue
            ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
            xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
            out[yd, xd] |= b[ys, xs]
    return out


def bound_pix(h, w):
    return int(np.ceil(0.008 * np.linalg.norm((h, w))))


def maps(result, gt, i, r):
    """bR, bG, bR & dil(bG), bG & dil(bR) of object ``i`` as uint8 [4,h,w]."""
    br, bg = seg2bmap(result == i), seg2bmap(gt == i)
    return np.stack([br, bg, br & dilate_disk(bg, r), bg & dilate_disk(br, r)]).astype(np.uint8)


def counts(result, gt, ids, r=None):
    """int64 [T,6] = |R&G|, |R|G|, |bR|, |bG|, |bR & dil(bG)|, |bG & dil(bR)| of one frame (and the maps [T,4,h,w])."""
    result, gt = np.asarray(result), np.asarray(gt)
    r = bound_pix(*result.shape) if r is None else r
    c = np.zeros((len(ids), 6), np.int64)
    m = np.zeros((len(ids), 4) + result.shape, np.uint8)
    for t, i in enumerate(ids):
        R, G = result == i, gt == i
        m[t] = maps(result, gt, i, r)
        c[t] = [(R & G).sum(), (R | G).sum()] + [int(m[t, k].sum()) for k in range(4)]
    return c, m


def db_eval_iou(annotation, segmentation):
    a, s = np.asarray(annotation).astype(bool), np.asarray(segmentation).astype(bool)
    union = np.logical_or(a, s).sum()
    if union == 0:
        return 1.0
    return float(np.logical_and(a, s).sum()) / float(union)


def db_eval_boundary(segmentation, annotation, bound_th=0.008):
    segmentation, annotation = np.asarray(segmentation), np.asarray(annotation)
    r = bound_th if bound_th >= 1 else int(np.ceil(bound_th * np.linalg.norm(segmentation.shape)))
    fg, gt = seg2bmap(segmentation), seg2bmap(annotation)
    gt_match, fg_match = gt & dilate_disk(fg, int(r)), fg & dilate_disk(gt, int(r))
    n_fg, n_gt = int(fg.sum()), int(gt.sum())
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = float(fg_match.sum()) / n_fg, float(gt_match.sum()) / n_gt
    return 0.0 if precision + recall == 0 else 2.0 * precision * recall / (precision + recall)


def read_ids(fn):
    from PIL import Image
    a = np.asarray(Image.open(fn))
    assert a.ndim == 2, fn
    return a.astype(np.int64)


def sequence_counts(result_dir, annotation_dir):
    """-> (names of the evaluated frames, ids, int64 [N,T,6]) by the protocol of evaluate_sequence."""
    ann_files = sorted(glob.glob(os.path.join(annotation_dir, "*.png")))
    if len(ann_files) < 3:
        raise ValueError(f"{annotation_dir}: need at least three annotated frames")
    ids = [int(i) for i in np.unique(read_ids(ann_files[0])) if i != 0]
    names, rows = [], []
    for fn in ann_files[1:-1]:
        gt = read_ids(fn)
        rf = os.path.join(result_dir, os.path.basename(fn))
        res = read_ids(rf) if os.path.exists(rf) else np.zeros_like(gt)
        if res.shape != gt.shape:
            raise ValueError(f"{rf}: shape {res.shape} differs from the annotation's {gt.shape}")
        names.append(os.path.splitext(os.path.basename(fn))[0])
        rows.append(counts(res, gt, ids)[0])
    return names, ids, np.stack(rows).reshape(len(rows), len(ids), 6)


def evaluate_sequence(result_dir, annotation_dir):
    ann_files = sorted(glob.glob(os.path.join(annotation_dir, "*.png")))
    if len(ann_files) < 3:
        raise ValueError(f"{annotation_dir}: need at least three annotated frames")
    ids = [int(i) for i in np.unique(read_ids(ann_files[0])) if i != 0]
    per = {i: ([], []) for i in ids}
    for fn in ann_files[1:-1]:
        gt = read_ids(fn)
        rf = os.path.join(result_dir, os.path.basename(fn))
        res = read_ids(rf) if os.path.exists(rf) else np.zeros_like(gt)
        if res.shape != gt.shape:
            raise ValueError(f"{rf}: shape {res.shape} differs from the annotation's {gt.shape}")
        for i in ids:
            per[i][0].append(db_eval_iou(gt == i, res == i))
            per[i][1].append(db_eval_boundary(res == i, gt == i))
    return {i: (float(np.mean(j)), float(np.mean(f))) for i, (j, f) in per.items()}


def evaluate(results_root, annotations_root, sequences=None):
    seqs = sequences or sorted(d for d in os.listdir(annotations_root) if os.path.isdir(os.path.join(results_root, d)))
    js, fs, table = [], [], {}
    for s in seqs:
        r = evaluate_sequence(os.path.join(results_root, s), os.path.join(annotations_root, s))
        table[s] = {str(i): {"J": round(j, 5), "F": round(f, 5)} for i, (j, f) in r.items()}
        js += [j for j, _ in r.values()]
        fs += [f for _, f in r.values()]
    mj, mf = (float(np.mean(js)) if js else math.nan), (float(np.mean(fs)) if fs else math.nan)
    return {"mean_J": round(mj, 5), "mean_F": round(mf, 5), "mean_JF_percent": round(50.0 * (mj + mf), 4), "objects": len(js),
            "sequences": len(seqs), "per_sequence": table}


# ------------------------------------------------------------------------------------------------------------------ synthetic data
def ellipse(h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0, h), rng.uniform(0, w)
    ry, rx = rng.uniform(1, max(2, h / 2)), rng.uniform(1, max(2, w / 2))
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1


def blob_maps(h, w, seed, ids=(1, 3, 7)):
    """A (result, annotation) pair of uint8 id maps: per id a random elliptical blob in the annotation and a shifted, dented copy of
    it in the result."""
    rng = np.random.default_rng(seed)
    res, gt = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for i in ids:
        b = ellipse(h, w, rng)
        gt[b] = i
        res[np.roll(b, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1)) & ~(ellipse(h, w, rng) & ellipse(h, w, rng))] = i
    return res, gt


def case_frames(h, w, seed):
    """Three frames (results [3,h,w], annotations [3,h,w]) for the ids [1, 3, 7]:
      0  id 1 in both maps, touching all four borders; id 3 only in the result; id 7 only in the annotation; a foreign id 9 in the result
      1  ids 1 and 3 in both maps, id 7 in neither
      2  id 1 covers the whole result frame (a mask without any boundary pixel); ids 1, 3 and 7 as blobs in the annotation"""
    rng = np.random.default_rng(seed)
    res, gt = np.zeros((3, h, w), np.uint8), np.zeros((3, h, w), np.uint8)
    frame = np.zeros((h, w), bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    b = ellipse(h, w, rng)
    res[0][b | frame] = 1
    gt[0][ellipse(h, w, rng) | b | frame] = 1
    res[0][ellipse(h, w, rng)] = 3
    gt[0][ellipse(h, w, rng)] = 7
    res[0][ellipse(h, w, rng) & (res[0] == 0)] = 9
    if h * w >= 12 and not (res[0] == 9).any():
        res[0][h // 2, w // 2] = 9
    res[1], gt[1] = blob_maps(h, w, seed + 1, ids=(1, 3))
    res[2], gt[2] = blob_maps(h, w, seed + 2, ids=(1, 3, 7))
    res[2][:] = 1
    return res, gt


def write_index_png(fn, idmap):
    from PIL import Image
    os.makedirs(os.path.dirname(fn), exist_ok=True)
    arr = np.ascontiguousarray(idmap, dtype=np.uint8)
    im = Image.frombytes("P", (arr.shape[1], arr.shape[0]), arr.tobytes())
    im.putpalette([v for i in range(256) for v in ((i * 37) % 256, (i * 91) % 256, (i * 53) % 256)])
    im.save(fn)


def make_tree(root, h=40, w=56):
    """Two videos under ``root``/results and ``root``/annotations: 'alpha' (6 annotated frames, ids 1 and 3; object 3 is lost from
    frame 3 on, the result of frame 2 is missing, the masks of frame 4 touch the bottom and right borders) and 'beta' (4 frames, id 2)."""
    root = str(root)
    for video, n, ids in (("alpha", 6, (1, 3)), ("beta", 4, (2,))):
        for k in range(n):
            res, gt = blob_maps(h, w, 100 * len(video) + 7 * n + k, ids=ids)
            if video == "alpha" and k >= 3:
                res[res == 3] = 0
            if video == "alpha" and k == 4:
                gt[h - 9:, w - 12:] = 1
                res[h - 7:, w - 15:] = 1
            if k == 0:
                for i in ids:                                   # the first annotation names the objects
                    gt[2 * i:2 * i + 2, 1:4] = i
            write_index_png(os.path.join(root, "annotations", video, f"{k:05d}.png"), gt)
            if not (video == "alpha" and k == 2):
                write_index_png(os.path.join(root, "results", video, f"{k:05d}.png"), res)
    return os.path.join(root, "results"), os.path.join(root, "annotations")
