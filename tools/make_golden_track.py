"""Generates tests/golden/track_ref.npz / track_host_refs.json by IMPORTING AND EXECUTING MergeTrack/merge.py and
MergeTrack/merge_functions.py (unmodified): the functions of the merge loop called directly on crafted inputs, and ``do_video`` on two
tiny videos.  What the build image lacks is stood in for, none of it from this package (no import of premvos_amd):

  * cv2.remap: a gather, exact for the integer-valued flows used here (as tools/make_golden_merge.py);
  * pycocotools.mask: encode / decode / iou / toBbox / area on real COCO RLE strings (this file's own small codec, after maskApi.c);
  * scipy.misc.imread: PIL;  tensorpack's palette: unused by do_video;
  * MergeTrack.refinement_net_functions / ReID_net_functions (they import TensorFlow engines): STUB engines, deterministic functions
    of the warped mask / the box.  Every stub output is recorded, tests replay them.

A condition, not a measurement: float64 sums in another order may differ in the last bits, so in every frame and in every direct case
that tests selection the best and second-best weighted score of each template must differ by >= 1e-6, and so must the final scores
of any two selections of a frame whose masks overlap (their order decides the paint).  The seed is advanced until that holds for
ALL cases; the smallest margins are stored.  Data only.
Usage: python tools/make_golden_track.py <PReMVOS checkout>"""
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
GOLD = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
H, W, EMB = 40, 56, 128
MARGIN = 1e-6


# ------------------------------------------------------------------------------------------------ COCO RLE (after maskApi.c)
def counts_of(mask):
    flat = (np.asarray(mask) != 0).reshape(-1, order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate(([0], change, [flat.size])))
    return ([0] if flat[0] else []) + [int(r) for r in runs]


def to_string(counts):
    out = bytearray()
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        while True:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            out.append((c | 0x20 if more else c) + 48)
            if not more:
                break
    return bytes(out)


def from_string(s):
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts, p = [], 0
    while p < len(b):
        x, k = 0, 0
        while True:
            c = b[p] - 48
            x |= (c & 0x1F) << (5 * k)
            p, k = p + 1, k + 1
            if not (c & 0x20):
                if c & 0x10:
                    x |= -1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def encode(m):
    m = np.asarray(m)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": to_string(counts_of(m))}


def decode(r):
    h, w = r["size"]
    c = from_string(r["counts"])
    ends = np.cumsum(c)
    flat = np.zeros(h * w, np.uint8)
    for i in range(1, len(c), 2):
        flat[ends[i - 1]:ends[i]] = 1
    return flat.reshape((h, w), order="F")


def to_bbox(r):
    h, w = r["size"]
    c = from_string(r["counts"])
    if sum(c[1::2]) == 0:
        return np.zeros(4)
    xs, ys, xe, ye, pos = w, h, 0, 0, 0
    for i, n in enumerate(c):
        if i % 2 == 1 and n > 0:
            a, b = pos, pos + n - 1
            xa, xb = a // h, b // h
            xs, xe = min(xs, xa), max(xe, xb)
            if xa < xb:
                ys, ye = 0, h - 1
            else:
                ys, ye = min(ys, a % h), max(ye, b % h)
        pos += n
    return np.array([xs, ys, xe - xs + 1, ye - ys + 1], np.float64)


def iou(dt, gt, iscrowd):
    out = np.zeros((len(dt), len(gt)))
    for i, a in enumerate(dt):
        for j, b in enumerate(gt):
            ma, mb = decode(a), decode(b)
            inter = int(np.count_nonzero(ma & mb))
            out[i, j] = inter / (int(np.count_nonzero(ma | mb)) if inter else 1)
    return out


def remap(img, map1, map2, interpolation, *a, **k):
    assert map2 is None and interpolation == 1
    h, w = img.shape[:2]
    x, y = map1[..., 0], map1[..., 1]
    assert np.array_equal(x, np.rint(x)) and np.array_equal(y, np.rint(y)), "integer flows only: bilinear == gather"
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    out = np.zeros(map1.shape[:2], img.dtype)
    out[ok] = img[yi[ok], xi[ok]]
    return out


# ------------------------------------------------------------------------------------------------------------- stub engines
UNITS = np.random.default_rng(7).integers(-8, 9, (6, EMB)).astype(np.float64) / 8.0
LOG = {"refine": [], "reid": []}


def stub_embedding(bbox, seed=0):
    """a point of an affine 4-d family in R^128, quantised to 1/64 (exact in float32, as an engine's .tolist() output is)"""
    x, y, w, h = (float(v) for v in bbox)
    e = UNITS[4] + (x / 8) * UNITS[0] + (y / 8) * UNITS[1] + (w / 4) * UNITS[2] + (h / 4) * UNITS[3] + seed * UNITS[5] / 4
    return (np.round(e * 64) / 64).astype(np.float32)


def stub_do_refinement(proposals, image_fn, net):
    masks = []
    for p in proposals:
        m = np.asarray(p["mask"], np.uint8)
        new = m.copy()
        new[:, 1:] |= m[:, :-1]                                 # grows one pixel to the right ...
        new[::7] &= m[::7]                                      # ... except in every seventh row
        seg = encode(new * 255)
        seg["counts"] = seg["counts"].decode("utf-8")
        p["segmentation"], p["conf_score"] = seg, str(np.float32(0.25))
        masks.append(new)
    LOG["refine"].append({"image_fn": image_fn, "bbox": np.array([np.asarray(p["bbox"], np.float64) for p in proposals]),
                          "mask": np.array(masks, np.uint8)})
    return proposals


def stub_add_ReID(proposals, image_fn, net):
    embs = []
    for p in proposals:
        e = stub_embedding(p["bbox"])
        p["ReID"] = e.tolist()
        embs.append(e)
    LOG["reid"].append({"image_fn": image_fn, "ReID": np.array(embs, np.float32)})
    return proposals


def install():
    cv2 = types.ModuleType("cv2")
    cv2.remap, cv2.INTER_LINEAR = remap, 1
    cv2.imwrite = cv2.cvtColor = cv2.resize = None
    cv2.COLOR_RGB2BGR = 0
    pm = types.ModuleType("pycocotools.mask")
    pm.encode, pm.decode, pm.iou, pm.toBbox = encode, decode, iou, to_bbox
    pm.area, pm.merge = (lambda r: int(sum(from_string(r["counts"])[1::2]))), None
    pc = types.ModuleType("pycocotools")
    pc.mask = pm
    sm = types.ModuleType("scipy.misc")
    sm.imread = lambda fn: np.array(Image.open(fn))
    sm.imsave = None
    tp, tpu, tpp = types.ModuleType("tensorpack"), types.ModuleType("tensorpack.utils"), types.ModuleType("tensorpack.utils.palette")
    tpp.PALETTE_RGB = np.zeros((1, 3))
    rf = types.ModuleType("MergeTrack.refinement_net_functions")
    rf.refinement_net_init, rf.do_refinement = (lambda: "stub refinement engine"), stub_do_refinement
    qf = types.ModuleType("MergeTrack.ReID_net_functions")
    qf.ReID_net_init, qf.add_ReID = (lambda: "stub ReID engine"), stub_add_ReID
    sys.modules.update({"cv2": cv2, "pycocotools": pc, "pycocotools.mask": pm, "scipy.misc": sm, "tensorpack": tp, "tensorpack.utils": tpu,
                        "tensorpack.utils.palette": tpp, "MergeTrack.refinement_net_functions": rf, "MergeTrack.ReID_net_functions": qf})
    sys.path.insert(0, os.path.join(REF, "code"))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:                    # an empty directory: the module-level video list is empty
        os.chdir(td)
        try:
            import MergeTrack.merge as M
            import MergeTrack.merge_functions as MF
        finally:
            os.chdir(cwd)
    return M, MF


# ------------------------------------------------------------------------------------------------------------------ helpers
def ellipse(cy, cx, ry, rx):
    yy, xx = np.mgrid[:H, :W]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.uint8)


def seg_str(m):
    s = encode(m)
    s["counts"] = s["counts"].decode("utf-8")
    return s


def jsonable(p):
    """a proposal dict without its embedding (kept in the npz) and with plain Python numbers"""
    out = {}
    for k, v in p.items():
        if k in ("ReID", "mask", "_idx"):
            continue
        out[k] = v.tolist() if isinstance(v, np.ndarray) else v.item() if isinstance(v, (np.floating, np.integer)) else v
    return out


def row_margin(ws, thresh):
    """smallest gap between the best and the second-best entry of a row of the weighted scores as calculate_selected_props sees them"""
    full = np.append(ws, thresh * np.ones((ws.shape[0], 1)), axis=1)
    full[~np.isfinite(full)] = 0
    srt = np.sort(full, axis=1)
    return float((srt[:, -1] - srt[:, -2]).min())


class TooClose(Exception):
    pass


def build(seed, M, MF):
    rng = np.random.default_rng(seed)
    arrays, g = {}, {"seed": seed, "h": H, "w": W}
    margins = {"weighted": np.inf, "paint": np.inf}

    def need(kind, value):
        margins[kind] = min(margins[kind], value)
        if value < MARGIN:
            raise TooClose(f"{kind}: {value}")

    def emb(bbox, s):
        return stub_embedding(bbox, s).astype(np.float64)

    # ---- calculate_scores: one template; three templates with a proposal without ReID, a template score < 0.5, a distance > 25
    def score_case(tag, n_t, n_p):
        props, templs, ep, et = [], [], [], []
        for i in range(n_t):
            m = ellipse(rng.integers(8, 32), rng.integers(8, 48), rng.integers(4, 10), rng.integers(4, 12))
            s = seg_str(m)
            e = emb(to_bbox(s), i)
            templs.append({"segmentation": s, "score": [1.0, 0.42, 0.83][i % 3], "ReID": e.tolist(), "id": i + 1})
            et.append(e)
        for j in range(n_p):
            m = ellipse(rng.integers(8, 32), rng.integers(8, 48), rng.integers(4, 10), rng.integers(4, 12))
            if j < n_t:
                m = np.roll(decode(templs[j]["segmentation"]), (1, 2), (0, 1))
            s = seg_str(m)
            p = {"segmentation": s, "score": round(float(rng.uniform(0.3, 1.0)), 2)}
            e = emb(to_bbox(s), j % 3)
            if j == n_p - 1 and n_t > 1:
                e = e + 40.0 * UNITS[5]                                           # farther than MAX_REID_DISTANCE from everything
            if j == n_p - 2 and n_t > 1:
                e = np.inf * np.ones(EMB)                                         # what read_props gives a proposal without 'ReID'
                p["ReID"] = e
            else:
                p["ReID"] = e.tolist()
            props.append(p)
            ep.append(e)
        planes = MF.calculate_scores(props, templs)
        weighted = np.dot(M.normalised_weights, planes.transpose((1, 0, 2)))
        need("weighted", row_margin(weighted, M.score_thesh))
        arrays.update({f"{tag}_emb_p": np.array(ep), f"{tag}_emb_t": np.array(et), f"{tag}_planes": planes, f"{tag}_weighted": weighted})
        g[tag] = {"proposals": [jsonable(p) for p in props], "templates": [jsonable(t) for t in templs]}
    score_case("scores1", 1, 5)
    score_case("scores3", 3, 8)

    # ---- calculate_selected_props on crafted weighted scores
    props = [{"segmentation": seg_str(ellipse(10 + 5 * j, 10 + 8 * j, 5, 6)), "bbox": [0, 0, 1, 1], "_idx": j} for j in range(4)]
    templs = [{"id": 3}, {"id": 1}, {"id": 7}, {"id": 2}]
    ws = np.array([[0.2, np.nan, 0.7, np.inf],                   # NaN and inf count as 0
                   [-0.5, -1.0, -0.2, -0.7],                     # everything below the threshold -> the empty proposal
                   [0.1, 0.4, -0.3, np.nan],
                   [M.score_thesh, 0.0, -np.inf, np.nan]])       # equal to the threshold: the first maximum wins
    obj = np.array([[0.3, 0.9, 0.1, 0.2], [1.5, 0.2, 0.1, 0.0], [0.0, 0.0, 0.0, 0.0], [0.2, 0.4, 1.9, 0.1]])
    plist = [dict(p) for p in props]
    sel = MF.calculate_selected_props(plist, ws.copy(), templs, M.score_thesh, obj)
    need("weighted", row_margin(ws[:3], M.score_thesh))          # (row 3 is the tie with the threshold on purpose: first maximum)
    arrays.update({"select_weighted": ws, "select_object": obj,
                   "select_index": np.array([p.get("_idx", len(props)) for p in sel]),
                   "select_final": np.array([p["final_score"] for p in sel]), "select_objscore": np.array([p["object_score"] for p in sel])})
    g["select"] = {"proposals": [jsonable(p) for p in props], "template_ids": [t["id"] for t in templs], "ids": [int(p["id"]) for p in sel],
                   "empty_bbox": np.asarray(plist[-1]["bbox"]).tolist(), "empty_counts": plist[-1]["segmentation"]["counts"]}

    # ---- remove_mask_overlap: overlapping masks, distinct scores; equal scores only on empty masks
    ms = [ellipse(18, 20, 9, 12), ellipse(22, 28, 8, 10), np.zeros((H, W), np.uint8), ellipse(14, 30, 6, 14), np.zeros((H, W), np.uint8)]
    fs = [0.61, 0.87, 1e-10, 0.35, 1e-10]
    sel = [{"segmentation": seg_str(m), "final_score": f, "object_score": 0.1 * i, "id": i + 2} for i, (m, f) in enumerate(zip(ms, fs))]
    out = MF.remove_mask_overlap(sel)
    arrays.update({"overlap_in": np.array(ms), "overlap_scores": np.array(fs), "overlap_out": np.array([p["mask"] for p in out]),
                   "overlap_bbox": np.array([np.asarray(p["bbox"], np.float64) for p in out])})
    g["overlap"] = {"out": [jsonable(p) for p in out], "keys": sorted(out[0].keys())}

    # ---- update_templates
    templs = [{"ReID": [1.0, 2.0], "id": 4, "score": 1.0}, {"ReID": [3.0, 4.0], "id": 9, "score": 1.0}]
    nxt = [{"ReID": [5.0, 5.0], "id": 0, "score": 0.7, "bbox": [1.0, 2.0, 3.0, 4.0]}, {"ReID": [6.0, 6.0], "id": 1, "score": 0.6, "bbox": [0.0, 0.0, 0.0, 0.0]}]
    g["update_templates"] = {"templates": templs, "next_props": copy_json(nxt), "out": MF.update_templates(templs, nxt), "next_props_after": nxt}

    # ---- read_ann / save_pngs (through real PNG files)
    ann = np.zeros((H, W), np.uint8)
    ann[ellipse(12, 14, 6, 8) > 0] = 1
    ann[ellipse(26, 40, 8, 9) > 0] = 2
    ann[ellipse(30, 10, 5, 6) > 0] = 5
    with tempfile.TemporaryDirectory() as td:
        im = Image.frombytes("P", (W, H), ann.tobytes())
        im.putpalette([0, 0, 0, 128, 0, 0] + [0] * (3 * 254))
        im.save(os.path.join(td, "a.png"))
        got = MF.read_ann(os.path.join(td, "a.png"))
        g["read_ann"] = [jsonable(p) for p in got]
        arrays["ann"] = ann
        sp = [{"mask": (ann == i).astype(np.uint8), "id": i} for i in (1, 2, 5)]
        MF.save_pngs(sp, os.path.join(td, "out", "sub", "00003.png"))
        MF.save_pngs([{"mask": np.zeros((H, W), np.uint8)}], os.path.join(td, "out", "sub", "00004.png"), empty=True)
        a, b = Image.open(os.path.join(td, "out", "sub", "00003.png")), Image.open(os.path.join(td, "out", "sub", "00004.png"))
        g["save_pngs"] = {"mode": a.mode, "ids": [1, 2, 5]}
        arrays.update({"png_index": np.array(a), "png_palette": np.array(a.getpalette(), np.uint8), "png_empty_index": np.array(b)})

    # ---- do_video on two tiny videos
    g["videos"] = {}
    for name, frames, with_ann in (("alpha", 7, True), ("beta", 6, False)):
        LOG["refine"].clear()
        LOG["reid"].clear()
        frames_log, vid = [], {"frames": frames, "with_annotation": with_ann, "proposals": {}}
        objs = [(6, 10, 4, 6), (19, 12, 5, 7), (33, 30, 4, 8)]                   # cy, cx, ry, rx
        vel = [(0, 3), (0, -6), (0, 4)]                                           # dy, dx per frame: apart and out of the frame
        flow = np.zeros((frames - 1, H, W, 2), np.float32)
        ann = np.zeros((H, W), np.uint8)
        for i, o in enumerate(objs):
            ann[ellipse(*o) > 0] = (1, 2, 4)[i]
        with tempfile.TemporaryDirectory() as td:
            dirs = {k: os.path.join(td, k) + "/" for k in ("images", "anns", "props", "flows", "out")}
            for d in dirs.values():
                os.makedirs(os.path.join(d, name))
            for t in range(frames):
                Image.fromarray(np.full((H, W, 3), 90 + t, np.uint8)).save(os.path.join(dirs["images"], name, f"{t:05d}.jpg"))
                pos = [(cy + t * dy, cx + t * dx, ry, rx) for (cy, cx, ry, rx), (dy, dx) in zip(objs, vel)]
                if t < frames - 1:
                    for (r0, r1), (dy, dx) in zip(((0, 13), (13, 27), (27, H)), vel):      # three bands moving apart, one out of the frame
                        flow[t, r0:r1] = (dx, dy)
                    with open(os.path.join(dirs["flows"], name, f"{t:05d}.flo"), "wb") as f:
                        np.array([202021.25], np.float32).tofile(f)
                        np.array([W, H], np.int32).tofile(f)
                        flow[t].tofile(f)
                # fresh proposals: near some objects (sometimes better than the warped candidate), plus clutter
                fresh = []
                for i, (cy, cx, ry, rx) in enumerate(pos):
                    if (t + i) % 2 == 0:
                        m = ellipse(cy, cx, ry + (t % 2), rx)
                        s = seg_str(m)
                        if to_bbox(s)[2] > 0:
                            fresh.append({"bbox": to_bbox(s).tolist(), "score": round(float(rng.uniform(0.75, 0.99)), 2), "segmentation": s,
                                          "conf_score": str(np.float32(rng.uniform(0.2, 0.9))), "ReID": stub_embedding(to_bbox(s), 0).tolist()})
                m = ellipse(rng.integers(6, 34), rng.integers(6, 50), 4, 5)
                s = seg_str(m)
                fresh.append({"bbox": to_bbox(s).tolist(), "score": round(float(rng.uniform(0.5, 0.9)), 2), "segmentation": s,
                              "conf_score": str(np.float32(0.5)), "ReID": stub_embedding(to_bbox(s), 2).tolist()})
                if t == 2:
                    del fresh[-1]["ReID"]                                         # a proposal without 'ReID'
                if t != 3:                                                        # frame 3: the proposal file is missing
                    with open(os.path.join(dirs["props"], name, f"{t:05d}.json"), "w") as f:
                        json.dump(fresh, f)
                    vid["proposals"][f"{t:05d}"] = fresh
            if with_ann:
                im = Image.frombytes("P", (W, H), ann.tobytes())
                im.putpalette([0, 0, 0, 128, 0, 0] + [0] * (3 * 254))
                im.save(os.path.join(dirs["anns"], name, "00000.png"))
            M.input_images, M.first_frame_anns, M.input_proposals = dirs["images"], dirs["anns"], dirs["props"]
            M.input_optical_flow, M.output_images = dirs["flows"], dirs["out"]
            orig_sel, orig_scores = MF.calculate_selected_props, MF.calculate_scores

            def rec_scores(proposals, templates):
                planes = orig_scores(proposals, templates)
                frames_log.append({"planes": planes})
                return planes

            def rec_select(proposals, weighted_scores, templates, score_thresh, object_scores):
                for j, p in enumerate(proposals):
                    p["_idx"] = j
                n = len(proposals)
                need("weighted", row_margin(weighted_scores, score_thresh))
                sel = orig_sel(proposals, weighted_scores, templates, score_thresh, object_scores)
                idx = [p.get("_idx", n) for p in sel]
                dm = [decode(p["segmentation"]) for p in sel]
                for a in range(len(sel)):
                    for b in range(a + 1, len(sel)):
                        if (dm[a] & dm[b]).any():
                            need("paint", abs(sel[a]["final_score"] - sel[b]["final_score"]))
                frames_log[-1].update({"weighted": np.array(weighted_scores), "selected": np.array(idx),
                                       "final_score": np.array([p["final_score"] for p in sel]),
                                       "object_score": np.array([p["object_score"] for p in sel])})
                for p in sel + proposals:
                    p.pop("_idx", None)
                return sel
            M.calculate_scores, M.calculate_selected_props = rec_scores, rec_select
            try:
                M.do_video(os.path.join(dirs["images"], name) + "/")
            finally:
                M.calculate_scores, M.calculate_selected_props = orig_scores, orig_sel
            pngs = [np.array(Image.open(os.path.join(dirs["out"], name, f"{t:05d}.png"))) for t in range(frames)]
        v = f"v_{name}"
        arrays.update({f"{v}_flow": flow, f"{v}_ann": ann, f"{v}_png": np.array(pngs)})
        if with_ann:
            assert len(frames_log) == frames and len(LOG["refine"]) == frames - 1 and len(LOG["reid"]) == frames
            arrays.update({f"{v}_selected": np.array([f["selected"] for f in frames_log]),
                           f"{v}_final_score": np.array([f["final_score"] for f in frames_log]),
                           f"{v}_object_score": np.array([f["object_score"] for f in frames_log]),
                           f"{v}_refine_bbox": np.array([c["bbox"] for c in LOG["refine"]]),
                           f"{v}_refine_mask": np.array([c["mask"] for c in LOG["refine"]]),
                           f"{v}_reid": np.array([c["ReID"] for c in LOG["reid"]])})
            for t, f in enumerate(frames_log):
                arrays[f"{v}_planes_{t}"], arrays[f"{v}_weighted_{t}"] = f["planes"], f["weighted"]
            sel = arrays[f"{v}_selected"]
            n_tmpl = sel.shape[1]
            vid["fresh_beats_warped_frames"] = [t for t in range(frames) if (sel[t] >= n_tmpl).any() and (sel[t] < frames_log[t]["planes"].shape[2]).all()]
            vid["object_left_frames"] = [t for t in range(frames) if any(not (pngs[t] == i).any() for i in (1, 2, 4))]
            assert vid["fresh_beats_warped_frames"] and vid["object_left_frames"], (vid["fresh_beats_warped_frames"], vid["object_left_frames"])
            assert (arrays[f"{v}_refine_bbox"][:, :, 2] == 0).any(), "no zero-area box went through the stub engines"
        else:
            assert not frames_log and not any(p.any() for p in pngs)
        g["videos"][name] = vid
    g["min_margin_weighted"], g["min_margin_paint"] = margins["weighted"], margins["paint"]
    g["normalised_weights"], g["score_thresh"], g["weights"] = M.normalised_weights.tolist(), M.score_thesh, M.weights.tolist()
    g["max_reid_distance"] = MF.MAX_REID_DISTANCE
    return arrays, g


def copy_json(x):
    return json.loads(json.dumps(x))


def main():
    M, MF = install()
    seed = 11
    while True:
        try:
            arrays, g = build(seed, M, MF)
            break
        except TooClose as e:
            print(f"seed {seed}: {e}; trying the next seed")
            seed += 1
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, "track_ref.npz"), **arrays)
    with open(os.path.join(GOLD, "track_host_refs.json"), "w") as f:
        json.dump(g, f, separators=(",", ":"))
    total = 0
    for fn in ("track_ref.npz", "track_host_refs.json"):
        total += os.path.getsize(os.path.join(GOLD, fn))
        print(fn, os.path.getsize(os.path.join(GOLD, fn)), "bytes")
    assert total < 256 * 1024, total
    print("seed", g["seed"], "min margins", g["min_margin_weighted"], g["min_margin_paint"])
    for name, v in g["videos"].items():
        print(name, {k: v[k] for k in v if k.endswith("_frames")})


if __name__ == "__main__":
    main()
