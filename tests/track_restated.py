"""A numpy restatement of the merge loop (MergeTrack/merge.py:69-121, merge_functions.py:14-149, 243-248, 508-525), the CPU yardstick
of premvos_amd.track: pinned against the reference EXECUTED (tests/golden/track_ref.npz, tools/make_golden_track.py) by
tests/test_cpu_track.py, then used by tests/test_gpu_track.py on inputs the fixture does not hold.  It lives in tests/ next to its
users; the warp comes from oracle.merge_oracle, RLE strings from premvos_amd.rle.  Also here: what both test files share -- the
fixture loader, the tree a fixture video is replayed from, and the replay engines.

Sums run in the kernel's fixed order (embedding index ascending, plane index ascending), products and sums as separate roundings."""
import json
import os
from copy import deepcopy as copy

import numpy as np

from oracle import merge_oracle as MO
from premvos_amd import rle

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_REID_DISTANCE = 25
SCORE_THRESH = 1e-10
WEIGHTS = np.array([0.25920137, 0.22541801, 0.0775609, 0.12509281, 0.3127269])
NORMALISED_WEIGHTS = WEIGHTS / np.sum(WEIGHTS)


# ------------------------------------------------------------------------------------------------------------ array level
def scores_from_arrays(inter, area_p, area_t, template_score, proposal_score, emb_p, emb_t):
    """-> planes float64 [5,T,P].  inter [T,P] / areas are pixel counts."""
    inter, area_p, area_t = np.asarray(inter, np.int64), np.asarray(area_p, np.int64), np.asarray(area_t, np.int64)
    T, P = inter.shape
    union = np.where(inter == 0, 1, area_p[None, :] + area_t[:, None] - inter)
    wsw = np.maximum(np.asarray(template_score, np.float64) - 0.5, 0) / (1 - 0.5)
    warp = (inter.astype(np.float64) / union.astype(np.float64)) * wsw[:, None]
    ep, et = np.asarray(emb_p, np.float64).reshape(P, -1), np.asarray(emb_t, np.float64).reshape(T, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((T, P))
        for k in range(ep.shape[1]):                                    # ascending k, one rounding per product and per sum
            d = ep[None, :, k] - et[:, None, k]
            acc = acc + d * d
        reid = 1 - np.sqrt(acc) / MAX_REID_DISTANCE
        reid[np.isinf(reid)] = 0
        reid[np.less(reid, 0)] = 0
    other_warp, other_reid = np.ones_like(warp), np.ones_like(reid)
    if T > 1:
        ids = np.arange(T)
        for t in ids:
            other_warp[t] = 1 - np.max(warp[ids != t], axis=0)
            other_reid[t] = 1 - np.max(reid[ids != t], axis=0)
    ms = np.maximum(np.asarray(proposal_score, np.float64) - 0.5, 0) / (1 - 0.5)
    return np.array([np.repeat(ms[None, :], T, axis=0), reid, other_reid, warp, other_warp])


def weighted_from_planes(planes, weights=NORMALISED_WEIGHTS):
    """merge.py:89 in plane order -> [T,P] (without the threshold column)."""
    w = np.asarray(weights, np.float64)
    with np.errstate(invalid="ignore"):
        out = w[0] * planes[0]
        for k in range(1, 5):
            out = out + w[k] * planes[k]
    return out


def select_from_weighted(weighted, score_thresh=SCORE_THRESH):
    """merge_functions.py:107-112 -> (full [T,P+1], index [T], best [T])."""
    full = np.append(np.asarray(weighted, np.float64), score_thresh * np.ones((len(weighted), 1)), axis=1)
    full[np.logical_not(np.isfinite(full))] = 0
    return full, full.argmax(axis=1), full.max(axis=1)


def paint_from_arrays(masks, selected, final_score, ids):
    """remove_mask_overlap + save_pngs on arrays: -> labels, idmap, refined.  Ascending (score, index): the last painted wins."""
    masks = np.asarray(masks)
    T = len(selected)
    h, w = masks.shape[1:]
    key = [(np.inf if s != s else float(s), t) for t, s in enumerate(np.asarray(final_score, np.float64))]
    labels = np.zeros((h, w), np.uint8)
    for _, t in sorted(key):
        if 0 <= selected[t] < len(masks):
            labels[masks[selected[t]] != 0] = t + 1
    idmap = np.zeros((h, w), np.uint8)
    for t in range(T):
        idmap[labels == t + 1] = np.uint8(ids[t])
    return labels, idmap, np.array([(labels == t + 1).astype(np.uint8) for t in range(T)]).reshape(T, h, w)


# -------------------------------------------------------------------------------------------------------------- dict level
def read_props(prop_fn):
    try:
        with open(prop_fn) as f:
            proposals = json.load(f)
        for p in proposals:
            if "ReID" not in p:
                p["ReID"] = np.inf * np.ones(128)
    except Exception:        # noqa: BLE001
        proposals = []
    return proposals


def read_ann(ann_fn):
    from PIL import Image
    ann = np.array(Image.open(ann_fn))
    out = []
    for id_ in [i for i in np.unique(ann) if i != 0]:
        seg = rle.encode((ann == id_).astype(np.uint8))
        out.append({"id": id_, "bbox": np.array(rle.to_bbox(seg)), "segmentation": seg, "conf_score": "1.0", "score": 1.0})
    return out


def calculate_scores(proposals, templates):
    pm = [rle.decode(p["segmentation"]) for p in proposals]
    tm = [rle.decode(t["segmentation"]) for t in templates]
    inter = np.array([[np.count_nonzero(a & b) for a in pm] for b in tm], np.int64).reshape(len(tm), len(pm))
    return scores_from_arrays(inter, [int(m.sum()) for m in pm], [int(m.sum()) for m in tm], [t["score"] for t in templates],
                              [float(p["score"]) for p in proposals], [np.asarray(p["ReID"], np.float64) for p in proposals],
                              [np.asarray(t["ReID"], np.float64) for t in templates])


def calculate_selected_props(proposals, weighted_scores, templates, score_thresh, object_scores):
    h, w = proposals[0]["segmentation"]["size"]
    seg = rle.encode(np.zeros((h, w), np.uint8))
    proposals.append({"segmentation": seg, "bbox": np.array(rle.to_bbox(seg))})
    _, index, best = select_from_weighted(weighted_scores, score_thresh)
    with np.errstate(invalid="ignore"):
        best_obj = np.asarray(object_scores).max(axis=1)
    sel = [proposals[i].copy() for i in index]
    for p, s, t, o in zip(sel, best, templates, best_obj):
        p["final_score"], p["object_score"], p["id"] = s, o, t["id"]
    return sel, index


def remove_mask_overlap(proposals):
    scores = [p["final_score"] if p["final_score"] else 0 for p in proposals]
    oscores = [p["object_score"] if p["object_score"] else 0 for p in proposals]
    masks = np.array([rle.decode(p["segmentation"]) for p in proposals])
    _, _, refined = paint_from_arrays(masks, list(range(len(proposals))), scores, [0] * len(proposals))
    out = []
    for i, p in enumerate(proposals):
        seg = rle.encode(refined[i])
        out.append({"segmentation": seg, "bbox": np.array(rle.to_bbox(seg)), "final_score": scores[i], "object_score": oscores[i],
                    "mask": refined[i], "id": p["id"]})
    return out


def update_templates(templates, next_props):
    new = copy(list(next_props))
    for p, t in zip(new, templates):
        p["ReID"], p["id"] = t["ReID"], t["id"]
    return new


def idmap_of(proposals, empty=False):
    png = np.zeros_like(proposals[0]["mask"])
    if not empty:
        for p in proposals:
            png[p["mask"].astype(bool)] = p["id"]
    return png


def do_video(video_dir, images, anns, props, flows, do_refinement, add_ReID):
    """merge.py:69-115 -> one record per frame: {"png": id map, "selected", "weighted" (with the threshold column), "planes",
    "final_score", "object_score"} (the last five only for frames with templates)."""
    from PIL import Image
    import glob
    log, templates, next_props = [], [], []
    fns = sorted(glob.glob(video_dir + "*"))
    for k, image_fn in enumerate(fns):
        stem = os.path.splitext(os.path.relpath(image_fn, images))[0]
        ann_fn = os.path.join(anns, stem + ".png")
        if os.path.exists(ann_fn) and "00000.jpg" in image_fn:
            new = add_ReID(read_ann(ann_fn), image_fn, None)
            templates, next_props = templates + copy(new), next_props + copy(new)
        if not templates:
            with Image.open(image_fn) as im:
                log.append({"png": np.zeros((im.size[1], im.size[0]), np.uint8)})
            continue
        proposals = next_props + read_props(os.path.join(props, stem + ".json"))
        planes = calculate_scores(proposals, templates)
        weighted = weighted_from_planes(planes)
        with np.errstate(invalid="ignore"):
            object_scores = planes[0] + planes[1]
        sel, index = calculate_selected_props(proposals, weighted, templates, SCORE_THRESH, object_scores)
        rec = {"selected": index, "weighted": select_from_weighted(weighted)[0], "planes": planes,
               "final_score": np.array([p["final_score"] for p in sel]), "object_score": np.array([p["object_score"] for p in sel]),
               "selected_masks": np.array([rle.decode(p["segmentation"]) for p in sel])}
        sel = remove_mask_overlap(sel)
        flow_fn = os.path.join(flows, stem + ".flo")
        if os.path.exists(flow_fn) and k + 1 < len(fns):
            next_props = MO.warp_proposals(sel, MO.get_flow(flow_fn), rle)
            next_props = do_refinement(next_props, fns[k + 1], None)
            next_props = add_ReID(next_props, fns[k + 1], None)
            templates = update_templates(templates, next_props)
        rec["png"] = idmap_of(sel)
        log.append(rec)
    return log


def margins(log):
    """(smallest best-minus-second-best gap of a weighted row, smallest final-score gap between two selections whose masks overlap)
    over the frames of a ``do_video`` log."""
    mw, mp = np.inf, np.inf
    for rec in log:
        if "weighted" not in rec:
            continue
        srt = np.sort(rec["weighted"], axis=1)
        mw = min(mw, float((srt[:, -1] - srt[:, -2]).min()))
        m, fs = rec["selected_masks"], rec["final_score"]
        for a in range(len(m)):
            for b in range(a + 1, len(m)):
                if (m[a] & m[b]).any():
                    mp = min(mp, abs(float(fs[a] - fs[b])))
    return mw, mp


# --------------------------------------------------------------------------------------------------- fixture and its replay
def load_fixture():
    with open(os.path.join(HERE, "golden", "track_host_refs.json")) as f:
        g = json.load(f)
    return np.load(os.path.join(HERE, "golden", "track_ref.npz")), g


def with_embeddings(dicts, emb):
    """the fixture keeps embeddings in the npz, the dicts in the JSON"""
    out = copy(dicts)
    for p, e in zip(out, emb):
        p["ReID"] = np.array(e, np.float64) if np.isinf(e).any() else np.array(e, np.float64).tolist()
    return out


def write_flo(fn, flow):
    with open(fn, "wb") as f:
        np.array([202021.25], np.float32).tofile(f)
        np.array([flow.shape[1], flow.shape[0]], np.int32).tofile(f)
        np.ascontiguousarray(flow, np.float32).tofile(f)


def write_index_png(fn, index):
    from PIL import Image
    im = Image.frombytes("P", (index.shape[1], index.shape[0]), np.ascontiguousarray(index, np.uint8).tobytes())
    im.putpalette([0, 0, 0, 128, 0, 0] + [0] * (3 * 254))
    im.save(fn)


def make_video_tree(root, name, arrays, g):
    """The input tree of fixture video ``name`` under ``root`` -> the five roots (images, anns, props, flows, out) with trailing '/'."""
    from PIL import Image
    vid = g["videos"][name]
    h, w = g["h"], g["w"]
    dirs = {k: os.path.join(str(root), k) + "/" for k in ("images", "anns", "props", "flows", "out")}
    for k in ("images", "anns", "props", "flows"):
        os.makedirs(os.path.join(dirs[k], name), exist_ok=True)
    flow = arrays[f"v_{name}_flow"]
    for t in range(vid["frames"]):
        Image.fromarray(np.full((h, w, 3), 90 + t, np.uint8)).save(os.path.join(dirs["images"], name, f"{t:05d}.jpg"))
        if t < len(flow):
            write_flo(os.path.join(dirs["flows"], name, f"{t:05d}.flo"), flow[t])
        if f"{t:05d}" in vid["proposals"]:
            with open(os.path.join(dirs["props"], name, f"{t:05d}.json"), "w") as f:
                json.dump(vid["proposals"][f"{t:05d}"], f)
    if vid["with_annotation"]:
        write_index_png(os.path.join(dirs["anns"], name, "00000.png"), arrays[f"v_{name}_ann"])
    return dirs


class ReplayEngines:
    """Stand-ins with the call shapes of do_refinement / add_ReID that return, call by call, what the fixture's stub engines (or a
    recorded run of the real ones) returned -- and check that they are asked about the same boxes."""

    def __init__(self, refine_masks, reid, refine_bbox=None):
        self.refine_masks, self.reid, self.refine_bbox = refine_masks, reid, refine_bbox
        self.n_refine = self.n_reid = 0

    def do_refinement(self, proposals, image_fn, net):
        k = self.n_refine
        self.n_refine += 1
        assert len(proposals) == len(self.refine_masks[k])
        if self.refine_bbox is not None:
            got = np.array([np.asarray(p["bbox"], np.float64) for p in proposals])
            assert np.array_equal(got, self.refine_bbox[k]), (k, got, self.refine_bbox[k])
        for p, m in zip(proposals, self.refine_masks[k]):
            p["segmentation"], p["conf_score"] = rle.encode(m), "0.25"
        return proposals

    def add_ReID(self, proposals, image_fn, net):
        k = self.n_reid
        self.n_reid += 1
        assert len(proposals) == len(self.reid[k])
        for p, e in zip(proposals, self.reid[k]):
            p["ReID"] = np.asarray(e, np.float64).tolist()
        return proposals
