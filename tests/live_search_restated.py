"""The live loop under other weights, and its objective, restated in numpy: ``track_restated.do_video``'s loop (merge.py:69-115) with
``weighted_from_planes(planes, weights)`` in place of the default weights, plus ``prewarp_restated.eval_video`` (merge_functions.py:
613-634, pinned to the reference's function through tests/golden/prewarp_ref.npz) of the id maps it paints -- what
MergeTrack/oldmerge.py:225-227,253-255 appends per weight set.  The yardstick of ``premvos_amd.track.SearchGroup`` / ``track --search``;
also here: what the CPU and GPU tests of the search share (the three hand-made weight sets, the kernel test's score inputs)."""
import glob
import os
from copy import deepcopy as copy

import numpy as np

import prewarp_restated as PR
import track_restated as R
from oracle import merge_oracle as MO
from premvos_amd import rle

ONE_HOT_MASK = np.array([1.0, 0.0, 0.0, 0.0, 0.0])          # the objectness plane alone
ONE_HOT_WARP = np.array([0.0, 0.0, 0.0, 1.0, 0.0])          # the mask-propagation plane alone
THREE_SETS = np.array([R.NORMALISED_WEIGHTS, ONE_HOT_MASK, ONE_HOT_WARP])


def weight_sets(V, seed=0):
    """the default, the two one-hot sets, then seeded random ones, normalised -> [V,5] (the first V of them)"""
    rng = np.random.default_rng(seed)
    rows = list(THREE_SETS) + [PR.normalised(rng.random(5)) for _ in range(max(0, V - 3))]
    return np.array(rows[:V])


def read_gt(fn):
    from PIL import Image
    return np.array(Image.open(fn)).astype(np.uint8)


def do_video(video_dir, images, anns, props, flows, do_refinement, add_ReID, weights):
    """merge.py:69-115 under ``weights`` (normalised [5]) -> (``track_restated.do_video``'s log, eval_video's scores [T0] of its id maps
    against ``anns``' annotation of EVERY frame: object k against id k + 1; None where a frame has no annotation -- the loop itself reads
    only 00000's)."""
    w = np.asarray(weights, np.float64)
    log, templates, next_props = [], [], []
    fns = sorted(glob.glob(video_dir + "*"))
    gts = []
    for k, image_fn in enumerate(fns):
        stem = os.path.splitext(os.path.relpath(image_fn, images))[0]
        ann_fn = os.path.join(anns, stem + ".png")
        gts.append(read_gt(ann_fn) if os.path.exists(ann_fn) else None)
        if os.path.exists(ann_fn) and "00000.jpg" in image_fn:
            new = add_ReID(R.read_ann(ann_fn), image_fn, None)
            templates, next_props = templates + copy(new), next_props + copy(new)
        assert templates, "the search skips a video without templates"
        proposals = next_props + R.read_props(os.path.join(props, stem + ".json"))
        planes = R.calculate_scores(proposals, templates)
        weighted = R.weighted_from_planes(planes, w)
        with np.errstate(invalid="ignore"):
            object_scores = planes[0] + planes[1]
        sel, index = R.calculate_selected_props(proposals, weighted, templates, R.SCORE_THRESH, object_scores)
        rec = {"selected": index, "weighted": R.select_from_weighted(weighted)[0], "planes": planes,
               "final_score": np.array([p["final_score"] for p in sel]), "object_score": np.array([p["object_score"] for p in sel]),
               "selected_masks": np.array([rle.decode(p["segmentation"]) for p in sel])}
        sel = R.remove_mask_overlap(sel)
        flow_fn = os.path.join(flows, stem + ".flo")
        if os.path.exists(flow_fn) and k + 1 < len(fns):
            next_props = MO.warp_proposals(sel, MO.get_flow(flow_fn), rle)
            next_props = do_refinement(next_props, fns[k + 1], None)
            next_props = add_ReID(next_props, fns[k + 1], None)
            templates = R.update_templates(templates, next_props)
        rec["png"] = R.idmap_of(sel)
        log.append(rec)
    ids = [int(t["id"]) for t in templates]
    if any(g is None for g in gts) or ids != list(range(1, len(ids) + 1)):
        return log, None
    return log, PR.eval_video(np.array([r["png"] for r in log]), np.array(gts), len(ids))


# ------------------------------------------------------------------------------------------- the score kernel's inputs (CPU + GPU tests)
DIFFER = ("V3", "V2F300", "V8")                               # cases in which two seats with the SAME inputs must select differently
SETS_CASES = {"V1": (1, [(3, 5)]), "V3": (3, [(5, 200)] * 3), "V3F0": (3, [(4, 0)] * 3), "V2F300": (2, [(10, 300), (10, 300)]),
              "V8": (8, [(T, 200) for T in (1, 2, 10, 32, 32, 0, 32, 4)])}                         # T + F > 256: a second pass of the lanes


def sets_inputs(name, seed):
    """Per seat (T, F) of ``SETS_CASES[name]`` (T = 0: an empty seat) ``test_gpu_track._score_inputs``-shaped arrays in which the F fresh
    rows (scores, embeddings) are the SAME for every seat, and seats of equal T have equal inputs altogether (they differ by their
    weights only): -> (per-seat list of [inter, area_p, area_t, ts, ps, ep, et] or None, the
    shared fresh scores [F], the shared fresh embeddings [F,128])."""
    from test_gpu_track import _score_inputs
    V, tf = SETS_CASES[name]
    F = tf[0][1]
    shared = _score_inputs(seed + 1000, 1, max(F, 1), no_reid=[j for j in (1, F - 2) if 0 <= j < F and F > 4])
    fs, fe = shared[4][:F].copy(), shared[5][:F].copy()
    per = []
    for v, (T, _) in enumerate(tf):
        if not T:
            per.append(None)
            continue
        a = list(_score_inputs(seed + 17 * T, T, T + F))
        a[4][:T] = a[3]                                      # the template score IS the candidate score of the same slot
        a[4][T:], a[5][T:] = fs, fe
        per.append(a)
    return per, fs, fe


def selections(a, weights):
    """the restatement's selection [T] of one seat's inputs under ``weights``"""
    planes = R.scores_from_arrays(*a)
    return R.select_from_weighted(R.weighted_from_planes(planes, weights))[1]
