"""Generates tests/golden/viz_ref.npz by IMPORTING AND EXECUTING MergeTrack/merge_functions.py and MergeTrack/print_max_reid_distance.py
(both unmodified): ``viz_scores`` (merge_functions.py:547-611) called directly on crafted 40 x 56 frames, and the whole program
print_max_reid_distance.py run with ``runpy`` on a two-video tree laid out under its hard-coded relative roots.  The stand-ins for what
the build image lacks are those of tools/make_golden_track.py (its ``install()``), plus, none of them from this package (no import of
premvos_amd):

  * cv2.resize: oracle/cv_resize_oracle.py ``resize_linear_u8``, the project's restatement of cv2's fixed-point INTER_LINEAR -- what
    gets pinned is the COMPOSITION (crop, resize, tint, cells, separators, marks), the primitive stays unpinned;
  * scipy.misc.imsave: a recorder of the float64 canvas (its bytescale is restated in tests/viz_restated.py, unpinned);
  * scipy.misc.imread: PIL;  tensorpack's PALETTE_RGB: a table whose row 2 is the DAVIS palette's entry 2, (0, 128, 0);
  * print_max_reid_distance.py: the stub ``add_ReID`` / ``ReID_net_init`` of make_golden_track.py; ``builtins.print`` is a recorder
    while the program runs, so its arrays are captured exactly.  One difference: the stub hands the templates' 'ReID' back as numpy
    arrays.  The released add_ReID (ReID_net_functions.py:39) stores ``.tolist()`` and a proposal file holds lists too, so line 42's
    ``c_reid - gt_reid`` is list - list and the program as released raises TypeError; the block it keeps commented out (:27-33)
    converts the templates with ``np.array`` -- the state it ran in.

Both run in a temporary working directory (viz_scores makes DAVIS/viz2/... relative to it).  Data only.
Usage: python tools/make_golden_viz.py <PReMVOS checkout>"""
import builtins
import json
import os
import runpy
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import make_golden_track as GT  # noqa: E402  (reads the checkout's place from sys.argv[1], like this file)
from oracle.cv_resize_oracle import resize_linear_u8  # noqa: E402

H, W, EMB = GT.H, GT.W, GT.EMB
TINT_ROW = (0, 128, 0)                                    # the DAVIS palette's entry 2 (its bit-reversal formula: id 2 = green bit 7)


def resize(img, dsize, interpolation):
    assert interpolation == 1 and tuple(dsize) == (100, 100)
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        return resize_linear_u8(img[:, :, None], dsize[0], dsize[1])[:, :, 0]
    return resize_linear_u8(img, dsize[0], dsize[1])


def frame_of(rng, lo, hi):
    """a smooth ramp plus a little noise, in [lo, hi]: tiles that compress"""
    yy, xx = np.mgrid[:H, :W]
    base = np.stack([(yy * 3 + xx) % 64, (yy + xx * 2) % 64, (yy * 2 + xx * 3) % 64], axis=2) / 63.0
    f = lo + (hi - lo) * base + rng.integers(0, 3, (H, W, 3))
    return np.clip(f, lo, hi).astype(np.uint8)


def box_mask(x, y, w, h):
    m = np.zeros((H, W), np.uint8)
    m[y:y + h, x:x + w] = 1
    return m


def main():
    M, MF = GT.install()
    recorded = []
    MF.cv2.resize = resize
    MF.imsave = lambda fn, arr: recorded.append((fn, np.array(arr, np.float64)))
    MF.imread = lambda fn: np.array(Image.open(fn))
    MF.PALETTE_RGB = np.array([(0, 0, 0), (128, 0, 0), TINT_ROW, (128, 128, 0)], np.int32)
    rng = np.random.default_rng(5)
    arrays = {"tint_row": np.array(TINT_ROW, np.uint8)}
    cwd = os.getcwd()

    def case(tag, frame, masks, boxes, planes, weighted, gt):
        masks = np.asarray(masks, np.uint8)
        P, T = len(masks), weighted.shape[0]
        assert planes.shape == (5, T, P) and weighted.shape == (T, P) and gt.shape == (T, P) and len(boxes) == P
        props = [{"bbox": np.asarray(b, np.float64), "segmentation": GT.seg_str(m)} for b, m in zip(boxes, masks)]
        with tempfile.TemporaryDirectory() as td:
            os.chdir(td)
            try:
                os.makedirs("in/v")
                fn = "in/v/00000.png"
                Image.fromarray(frame).save(fn)
                del recorded[:]
                MF.viz_scores(planes.copy(), weighted.copy(), props, fn, "in/", gt_scores=np.array([gt] * 5))
                assert len(recorded) == 1 and recorded[0][0] == "DAVIS/viz2/v/00000.png" and os.path.isdir("DAVIS/viz2/v")
            finally:
                os.chdir(cwd)
        canvas = recorded[0][1]
        assert canvas.shape == (100 * (T + 1), 100 * P, 3) and canvas.dtype == np.float64
        arrays.update({f"{tag}_frame": frame, f"{tag}_masks": masks, f"{tag}_boxes": np.array(boxes, np.float64), f"{tag}_planes": planes,
                       f"{tag}_weighted": weighted, f"{tag}_gt": gt, f"{tag}_canvas": canvas})
        return canvas

    # ---- t1p4: one template (the "other" planes are all ones); a box with min(h, w) < 2; a 2 x 2 box (a 1 x 1 crop); cmax = 255
    boxes = [(10.7, 8.2, 20.9, 15.0), (30.0, 5.0, 1.9, 12.0), (44.0, 20.0, 2.0, 2.0), (3.0, 22.0, 17.0, 13.0)]
    masks = [GT.ellipse(15, 20, 6, 9), box_mask(30, 5, 1, 12), box_mask(44, 20, 2, 2), GT.ellipse(28, 11, 5, 7)]
    planes = np.round(rng.uniform(0.05, 0.95, (5, 1, 4)), 3)
    planes[2] = planes[4] = 1.0
    c = case("t1p4", frame_of(rng, 20, 250), masks, boxes, planes, np.round(rng.uniform(0.05, 0.95, (1, 4)), 3),
             np.round(rng.uniform(0.0, 0.95, (1, 4)), 3))
    assert c.max() == 255.0 and c.min() == 0.0
    assert not c[:100, 100:200].any() and c[:100, 200:300].any()                # the black tile; the 1 x 1 crop is one colour
    # ---- t3p6: three templates; a box touching the right and bottom frame edge; an all-zero mask; cmax = 255 (a score of exactly 1)
    boxes = [(4.0, 3.0, 22.0, 17.0), (36.0, 24.0, 20.0, 16.0), (20.5, 10.5, 12.5, 9.5), (0.0, 0.0, 56.0, 40.0), (12.0, 20.0, 9.0, 14.0),
             (30.0, 2.0, 15.0, 11.0)]
    masks = [GT.ellipse(11, 14, 7, 9), box_mask(36, 24, 20, 16), GT.ellipse(15, 26, 4, 5), np.ones((H, W), np.uint8),
             np.zeros((H, W), np.uint8), GT.ellipse(7, 37, 4, 6)]
    planes = np.round(rng.uniform(0.0, 1.0, (5, 3, 6)), 3)
    planes[1, 2, 3], planes[0, 0, 0] = 1.0, 0.0
    ws = np.round(rng.uniform(0.05, 0.95, (3, 6)), 3)
    ws[1, 2] = ws[1, 4] = 0.97                                                   # a tie: the first maximum carries the mark
    gt = np.round(rng.uniform(0.0, 0.9, (3, 6)), 3)
    gt[2] = 0.0                                                                  # an object the annotation lacks: argmax 0
    c = case("t3p6", frame_of(rng, 0, 255), masks, boxes, planes, ws, gt)
    assert c.max() == 255.0
    # ---- dark: no score is exactly 0 or 1 and every tile is dark: cmax < 255, the bytescale factor is not 1
    boxes = [(5.0, 5.0, 30.0, 20.0), (20.0, 12.0, 25.0, 25.0), (2.0, 18.0, 14.0, 19.0), (33.0, 3.0, 21.0, 30.0)]
    masks = [GT.ellipse(14, 19, 8, 12), GT.ellipse(23, 32, 9, 10), GT.ellipse(27, 8, 7, 5), GT.ellipse(17, 43, 12, 8)]
    c = case("dark", frame_of(rng, 5, 90), masks, boxes, np.round(rng.uniform(0.25, 0.75, (5, 2, 4)), 3),
             np.round(rng.uniform(0.25, 0.75, (2, 4)), 3), np.round(rng.uniform(0.25, 0.75, (2, 4)), 3))
    assert 100 < c.max() < 255 and c.min() == 0.0
    arrays["cases"] = np.array(["t1p4", "t3p6", "dark"])

    # ---- print_max_reid_distance.py on a two-video tree under its hard-coded relative roots
    printed = []
    vids = {"alpha": {"frames": 4, "anns": (0, 2)}, "beta": {"frames": 3, "anns": (0,)}}
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            for name, v in vids.items():
                for d in ("DAVIS/val17", "DAVIS/ReID_props", "DAVIS/val17-ff"):
                    os.makedirs(os.path.join(d, name))
                embs, counts = [], []
                for t in range(v["frames"]):
                    Image.fromarray(np.full((H, W, 3), 60 + t, np.uint8)).save(f"DAVIS/val17/{name}/{t:05d}.jpg")
                    if t in v["anns"]:                                           # (an annotation on a later frame: more templates)
                        ann = np.zeros((H, W), np.uint8)
                        ann[GT.ellipse(10 + 3 * t, 12 + 5 * t, 5, 7) > 0] = 1
                        if t == 0:
                            ann[GT.ellipse(28, 40, 6, 8) > 0] = 2
                        im = Image.frombytes("P", (W, H), ann.tobytes())
                        im.putpalette([0, 0, 0, 128, 0, 0] + [0] * (3 * 254))
                        im.save(f"DAVIS/val17-ff/{name}/{t:05d}.png")
                    if name == "alpha" and t == 1:                               # a frame without a proposal file
                        counts.append(0)
                        continue
                    props = []
                    for j in range(3 + t):
                        s = GT.seg_str(GT.ellipse(rng.integers(8, 32), rng.integers(8, 48), rng.integers(3, 8), rng.integers(3, 9)))
                        e = GT.stub_embedding(GT.to_bbox(s), j % 3).astype(np.float64)
                        if name == "beta" and t == 2 and j == 1:
                            e = e + 40.0 * GT.UNITS[5]                           # farther than MAX_REID_DISTANCE from everything
                        p = {"bbox": GT.to_bbox(s).tolist(), "score": 0.8, "segmentation": s, "ReID": e.tolist()}
                        if name == "alpha" and t == 3 and j == 0:
                            del p["ReID"]                                        # a proposal without 'ReID': read_props gives inf x 128
                            e = np.inf * np.ones(EMB)
                        props.append(p)
                        embs.append(e)
                    with open(f"DAVIS/ReID_props/{name}/{t:05d}.json", "w") as f:
                        json.dump(props, f)
                    counts.append(len(props))
                arrays[f"mrd_{name}_props"], arrays[f"mrd_{name}_counts"] = np.array(embs, np.float64), np.array(counts, np.int64)
            GT.LOG["reid"].clear()
            qf = sys.modules["MergeTrack.ReID_net_functions"]

            def add_ReID_arrays(proposals, image_fn, net):                       # see the docstring: arrays, not lists
                for p in GT.stub_add_ReID(proposals, image_fn, net):
                    p["ReID"] = np.array(p["ReID"])
                return proposals
            qf.add_ReID = add_ReID_arrays
            real_print = builtins.print
            builtins.print = lambda *a, **k: printed.append(np.array(a[0], np.float64))
            try:
                runpy.run_path(os.path.join(GT.REF, "code", "MergeTrack", "print_max_reid_distance.py"), run_name="__main__")
            finally:
                builtins.print = real_print
        finally:
            os.chdir(cwd)
    assert len(printed) == 3 and printed[0].shape == (3,) and printed[1].shape == (2,) and printed[2].shape == ()
    for name in vids:                                                            # what the stub engine returned for the templates
        arrays[f"mrd_{name}_templates"] = np.concatenate([c["ReID"] for c in GT.LOG["reid"] if f"/{name}/" in c["image_fn"]]).astype(np.float64)
    arrays.update({"mrd_alpha_max": printed[0], "mrd_beta_max": printed[1], "mrd_dataset_max": printed[2], "mrd_videos": np.array(sorted(vids))})
    assert arrays["mrd_alpha_templates"].shape == (3, EMB) and arrays["mrd_beta_templates"].shape == (2, EMB)
    assert printed[2] > MF.MAX_REID_DISTANCE > printed[0].min() and np.isinf(arrays["mrd_alpha_props"]).any()     # both sides of 25
    fn = os.path.join(GT.GOLD, "viz_ref.npz")
    np.savez_compressed(fn, **arrays)
    assert all(np.asarray(v).dtype != object for v in arrays.values())
    print(f"{fn}: {os.path.getsize(fn)} bytes; max distances {printed[0]} {printed[1]} {printed[2]}")
    assert os.path.getsize(fn) < 512 * 1024


if __name__ == "__main__":
    main()
