"""The merge stage on the GPU (csrc/track_ops.hip, premvos_amd/track.py) against the numpy restatement (tests/track_restated.py, itself
pinned to the reference executed: tests/test_cpu_track.py) and against the reference's own ``do_video`` results in the fixture.
One process, no subprocess fan-out.

Bounds.  Planes 0 / 3 / 4 are chains of single correctly rounded operations on the same operands: bit-equal.  Planes 1 / 2 and the
weighted scores: <= 1e-12 (a 128-term float64 sum of squares carries at most ~65 ulp relative error in the distance, <= 1e-14 on a
score in [0,1]; 100x margin).  Selections: equal, on inputs whose best and second-best weighted score differ by >= 1e-6 (asserted, never
skipped).  Labels, id maps, masks, PNG indices: bit-equal."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_restated as R  # noqa: E402
from premvos_amd import rle  # noqa: E402

TOL = 1e-12


def _blobs(rng, h, w, n):
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), np.uint8)
    for _ in range(n):
        cy, cx = rng.integers(0, h), rng.integers(0, w)
        ry, rx = rng.integers(1, max(2, h // 3)), rng.integers(1, max(2, w // 3))
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
    return m


# ------------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (64, 33), (480, 854)])
def test_rle_decode_inverts_the_boundary_kernel_and_the_host_codec(h, w):
    from premvos_amd import _lib, track
    rng = np.random.default_rng(h * 1000 + w)
    masks = [_blobs(rng, h, w, 3), np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8),
             _blobs(rng, h, w, 1)]
    m = torch.from_numpy(np.stack(masks)).cuda()
    n = len(masks)
    lib = _lib.load()
    ws = torch.empty((int(lib.premvos_rle_workspace_bytes(n, h, w)) + 3) // 4, dtype=torch.int32, device=m.device)
    cap = n * h * w + 16
    pool = torch.full((cap,), -1, dtype=torch.int32, device=m.device)
    off = torch.empty((n + 1,), dtype=torch.int32, device=m.device)
    _lib.check(lib.premvos_rle_boundaries_pooled_u8(m.data_ptr(), n, h, w, h * w, w, pool.data_ptr(), cap, off.data_ptr(), ws.data_ptr(),
                                                    _lib.current_stream()), "rle_boundaries_pooled")
    total = int(off[-1])
    assert total <= cap
    got = track.decode_boundaries(pool[:total].contiguous(), off, h, w)                      # device pool, device offsets
    assert got.dtype == torch.uint8 and got.shape == (n, h, w) and torch.equal(got, m)
    segs = [rle.encode(x) for x in masks]
    got2 = track.decode_segmentations(segs).cpu().numpy()                                     # strings -> host boundaries -> device
    assert np.array_equal(got2, np.stack([rle.decode(s) for s in segs])) and np.array_equal(got2, np.stack(masks))
    # into a view of a larger tensor (how the tracker appends the fresh proposals to the resident candidates)
    buf = torch.full((n + 2, h, w), 7, dtype=torch.uint8, device=m.device)
    track.decode_segmentations(segs, out=buf[2:])
    assert torch.equal(buf[2:], m) and bool((buf[:2] == 7).all())


def test_rle_decode_of_no_masks():
    from premvos_amd import track
    out = track.decode_boundaries(np.zeros((0,), np.int32), np.zeros((1,), np.int32), 6, 9)
    assert out.shape == (0, 6, 9) and out.is_cuda


# ------------------------------------------------------------------------------------------------------------------- scores
def _score_inputs(seed, T, P, no_reid=()):
    rng = np.random.default_rng(seed)
    area_p, area_t = rng.integers(0, 5000, P), rng.integers(1, 5000, T)
    inter = np.minimum(rng.integers(0, 5000, (T, P)), np.minimum(area_p[None, :], area_t[:, None]))
    inter[rng.random((T, P)) < 0.3] = 0
    ts = np.round(rng.uniform(0.3, 1.0, T), 3)
    ps = np.round(rng.uniform(0.3, 1.0, P), 2)
    et = rng.normal(0, 0.8, (T, 128))
    ep = et[rng.integers(0, T, P)] + rng.normal(0, 0.6, (P, 128)) * rng.uniform(0.1, 3.0, (P, 1))
    for j in no_reid:
        ep[j] = np.inf
    return inter.astype(np.int64), area_p.astype(np.int64), area_t.astype(np.int64), ts, ps, ep, et


def _run_scores(args, **kw):
    from premvos_amd import track
    inter, area_p, area_t, ts, ps, ep, et = args
    dev = torch.device("cuda", torch.cuda.current_device())
    out = track.track_scores(torch.from_numpy(inter).to(dev), torch.from_numpy(area_p).to(dev), torch.from_numpy(area_t).to(dev), ts, ps, ep, et, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_scores(got, args, thresh=R.SCORE_THRESH, need_margin=True):
    planes = R.scores_from_arrays(*args)
    full, index, best = R.select_from_weighted(R.weighted_from_planes(planes), thresh)
    for k in (0, 3, 4):
        assert np.array_equal(got["planes"][k], planes[k], equal_nan=True), k
    d12 = max(float(np.nanmax(np.abs(got["planes"][k] - planes[k]))) for k in (1, 2))
    dw = float(np.abs(got["weighted"] - full).max())
    with np.errstate(invalid="ignore"):
        obj = (planes[0] + planes[1]).max(axis=1)
    do = float(np.nanmax(np.abs(got["object_score"] - obj)))
    print(f"T={planes.shape[1]} P={planes.shape[2]}: max |d| planes 1,2 {d12:.3e}  weighted {dw:.3e}  object {do:.3e}")
    assert np.array_equal(np.isnan(got["planes"]), np.isnan(planes))
    assert d12 <= TOL and dw <= TOL and do <= TOL and np.abs(got["final_score"] - best).max() <= TOL
    assert np.array_equal(np.isnan(got["object_score"]), np.isnan(obj))
    if need_margin:
        srt = np.sort(full, axis=1)
        assert float((srt[:, -1] - srt[:, -2]).min()) >= 1e-6, "the inputs of this case must have a margin: pick another seed"
    assert got["selected"].tolist() == index.tolist()
    assert np.array_equal(got["final_score"], got["weighted"][np.arange(len(index)), got["selected"]])


@pytest.mark.parametrize("T,P,seed", [(1, 1, 3), (1, 40, 4), (3, 17, 5), (10, 110, 6), (32, 512, 7), (7, 300, 8)])
def test_track_scores_equal_the_restatement(T, P, seed):
    args = _score_inputs(seed, T, P, no_reid=[j for j in (1, P - 2) if 0 <= j < P and P > 4])
    got = _run_scores(args)
    _check_scores(got, args)
    again = _run_scores(args)                                                                   # two launches: the same bits
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_track_scores_special_values():
    """The fixture's special values through the kernel: a proposal without ReID (all inf -> score 0), a template score below 0.5
    (warp plane off), a distance above MAX_REID_DISTANCE (0), a row entirely below the threshold (-> the empty proposal P), a value
    equal to the threshold (first maximum: the proposal, not the empty one), NaN (a template without ReID) counted as 0."""
    a, g = R.load_fixture()
    props = R.with_embeddings(g["scores3"]["proposals"], a["scores3_emb_p"])
    templs = R.with_embeddings(g["scores3"]["templates"], a["scores3_emb_t"])
    from premvos_amd import track
    planes = track.calculate_scores(props, templs)                                              # the dict form: decode + overlap + scores
    ref = a["scores3_planes"]
    for k in (0, 3, 4):
        assert np.array_equal(planes[k], ref[k]), k
    assert np.abs(planes[1] - ref[1]).max() <= TOL and np.abs(planes[2] - ref[2]).max() <= TOL
    assert (planes[1][:, -2] == 0).all() and (planes[1][:, -1] == 0).all() and (planes[3][1] == 0).all()
    args = list(_score_inputs(21, 4, 9))
    base = _run_scores(args)
    # a threshold above every score of a row: the empty proposal (index P) wins everywhere
    hi = _run_scores(args, score_thresh=10.0)
    assert hi["selected"].tolist() == [9] * 4 and (hi["final_score"] == 10.0).all() and (hi["weighted"][:, -1] == 10.0).all()
    _check_scores(hi, args, thresh=10.0)
    # a threshold EQUAL to row 2's best score: the first maximum is the proposal
    t2 = float(base["final_score"][2])
    eq = _run_scores(args, score_thresh=t2)
    assert eq["selected"][2] == base["selected"][2] < 9 and eq["final_score"][2] == t2
    # a template without ReID: its ReID row is NaN (inf - inf), so is every other template's 'other ReID'; NaN counts as 0
    args[6] = args[6].copy()
    args[6][1] = np.inf
    args[5] = args[5].copy()
    args[5][3] = np.inf
    nan = _run_scores(args)
    assert np.isnan(nan["planes"][1][1, 3]) and nan["planes"][1][1, 0] == 0 and np.isnan(nan["planes"][2][0, 3])
    assert nan["weighted"][1, 3] == 0 and np.isfinite(nan["weighted"]).all() and np.isnan(nan["object_score"][1])
    _check_scores(nan, args, need_margin=False)


def test_track_scores_limits():
    from premvos_amd import _lib, track
    dev = torch.device("cuda", torch.cuda.current_device())
    T, P = 256, 4
    with pytest.raises(_lib.PremvosError, match="255"):
        track.track_scores(torch.zeros((T, P), dtype=torch.int64, device=dev), torch.zeros((P,), dtype=torch.int64, device=dev),
                           torch.zeros((T,), dtype=torch.int64, device=dev), np.ones(T), np.ones(P), np.zeros((P, 128)), np.zeros((T, 128)))


# -------------------------------------------------------------------------------------------------------------------- paint
def _run_paint(masks, selected, scores, ids):
    from premvos_amd import track
    dev = torch.device("cuda", torch.cuda.current_device())
    out = track.track_paint(torch.from_numpy(masks).to(dev), torch.tensor(selected, dtype=torch.int32, device=dev),
                            torch.tensor(scores, dtype=torch.float64, device=dev), torch.tensor(ids, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("T,P,h,w", [(1, 3, 9, 7), (5, 12, 40, 56), (255, 300, 31, 45), (10, 30, 480, 854)])
def test_track_paint_equals_the_restatement(T, P, h, w):
    rng = np.random.default_rng(T * 7 + P)
    masks = np.stack([_blobs(rng, h, w, 2) * rng.integers(1, 256) for _ in range(P)]).astype(np.uint8)   # nonzero = foreground
    selected = rng.integers(0, P + 1, T).tolist()                                                          # P = the empty proposal
    if T > 1:
        selected[1] = P
    scores = rng.permutation(T).astype(np.float64) / T + 1e-3                                              # distinct
    ids = rng.permutation(255)[:T] + 1
    got = _run_paint(masks, selected, scores.tolist(), ids.tolist())
    ref = R.paint_from_arrays(masks, selected, scores, ids)
    for a, b, name in zip(got, ref, ("labels", "idmap", "refined")):
        assert a.dtype == np.uint8 and np.array_equal(a, b), name
    assert got[2].shape == (T, h, w) and set(np.unique(got[2])) <= {0, 1}
    if T > 1:
        assert not got[2][1].any()


def test_track_paint_tie_rule_and_fixture_case():
    """Equal final scores: the higher index wins (this package's rule; the reference leaves it to an unstable argsort).  And the
    fixture's remove_mask_overlap case through the dict form."""
    from premvos_amd import track
    h, w = 20, 32
    masks = np.zeros((3, h, w), np.uint8)
    masks[0, 2:12, 2:20] = 1
    masks[1, 6:16, 10:28] = 1
    masks[2, 0:20, 15:18] = 1
    got = _run_paint(masks, [0, 1, 2], [0.5, 0.5, 0.25], [4, 9, 2])
    ref = R.paint_from_arrays(masks, [0, 1, 2], [0.5, 0.5, 0.25], [4, 9, 2])
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    assert got[0][8, 12] == 2 and got[0][8, 16] == 2 and got[0][3, 16] == 1 and got[0][0, 16] == 3 and got[1][8, 12] == 9
    a, g = R.load_fixture()
    sel = [{"segmentation": rle.encode(m), "final_score": float(s), "object_score": 0.1 * i, "id": i + 2}
           for i, (m, s) in enumerate(zip(a["overlap_in"], a["overlap_scores"]))]
    out = track.remove_mask_overlap(sel)
    assert np.array_equal(np.array([p["mask"] for p in out]), a["overlap_out"])
    assert np.array_equal(np.array([p["bbox"] for p in out]), a["overlap_bbox"])
    for p, q in zip(out, g["overlap"]["out"]):
        assert p["segmentation"] == q["segmentation"] and p["final_score"] == q["final_score"] and p["id"] == q["id"]


def test_track_paint_limits():
    from premvos_amd import _lib
    with pytest.raises(_lib.PremvosError, match="255"):
        _run_paint(np.zeros((2, 4, 4), np.uint8), [0] * 256, [0.0] * 256, [1] * 256)


# ----------------------------------------------------------------------------------------------- do_video, the fixture's stubs
@pytest.mark.parametrize("name", ["alpha", "beta"])
def test_do_video_with_the_fixtures_stub_engines(tmp_path, name):
    from PIL import Image
    from premvos_amd import track
    a, g = R.load_fixture()
    frames = g["videos"][name]["frames"]
    with_ann = g["videos"][name]["with_annotation"]
    logs = {}
    for form, resident in (("resident", True), ("dicts", False)):
        d = R.make_video_tree(tmp_path / form, name, a, g)
        eng = R.ReplayEngines(a[f"v_{name}_refine_mask"], a[f"v_{name}_reid"], a[f"v_{name}_refine_bbox"]) if with_ann else R.ReplayEngines([], [])
        logs[form] = track.do_video(os.path.join(d["images"], name) + "/", d["images"], d["anns"], d["props"], d["flows"], d["out"],
                                    None, None, do_refinement=eng.do_refinement, add_ReID=eng.add_ReID, resident=resident, record=True)
        assert len(logs[form]) == frames and eng.n_reid == (frames if with_ann else 0) and eng.n_refine == (frames - 1 if with_ann else 0)
        for t, rec in enumerate(logs[form]):
            im = Image.open(rec["png_fn"])
            assert im.mode == "P" and np.array_equal(np.array(im.getpalette(), np.uint8), a["png_palette"])
            assert np.array_equal(np.array(im), a[f"v_{name}_png"][t]), (form, t)                # the reference's PNG, index for index
            assert np.array_equal(rec["png"], a[f"v_{name}_png"][t])
            if with_ann:
                assert rec["selected"].tolist() == a[f"v_{name}_selected"][t].tolist(), (form, t)
                assert np.abs(rec["weighted"][:, :-1] - a[f"v_{name}_weighted_{t}"]).max() <= TOL
                for k in range(5):
                    assert np.abs(rec["planes"][k] - a[f"v_{name}_planes_{t}"][k]).max() <= TOL, (form, t, k)
                if t == 0:
                    for k in (0, 3, 4):
                        assert np.array_equal(rec["planes"][k], a[f"v_{name}_planes_{t}"][k])
    if with_ann:
        for t, (x, y) in enumerate(zip(logs["resident"], logs["dicts"])):                         # the two forms: the same bits
            for k in ("selected", "weighted", "planes", "png"):
                assert x[k].tobytes() == y[k].tobytes(), k
            assert np.abs(x["final_score"] - a[f"v_{name}_final_score"][t]).max() <= TOL
            assert np.abs(x["object_score"] - a[f"v_{name}_object_score"][t]).max() <= TOL


# ------------------------------------------------------------------------------------------------------ real engines, 480x854
REAL_SEED = 5


def _real_tree(root, T_frames, n_obj, seed):
    """8 frames of 480x854 with 3 objects drifting by sub-pixel flows (inside the frame), a first-frame annotation, fresh proposals
    per frame (near the objects and elsewhere, embeddings spread around), flows with sub-pixel parts."""
    from PIL import Image
    from premvos_amd import synth
    H, W = 480, 854
    rng = np.random.default_rng(seed)
    dirs = {k: os.path.join(str(root), k) + "/" for k in ("images", "anns", "props", "flows", "out")}
    for k in ("images", "anns", "props", "flows"):
        os.makedirs(os.path.join(dirs[k], "clip"))
    frames = synth.clip_frames(0, T_frames, H, W).numpy()
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    centres = [(140, 200), (300, 430), (200, 660)][:n_obj]
    radii = [(50, 70), (60, 90), (45, 60)][:n_obj]
    vel = [(1.75, 2.5), (-1.25, 3.25), (2.5, -2.75)][:n_obj]
    ann = np.zeros((H, W), np.uint8)
    for i, ((cy, cx), (ry, rx)) in enumerate(zip(centres, radii)):
        ann[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = (1, 2, 3)[i]
    R.write_index_png(os.path.join(dirs["anns"], "clip", "00000.png"), ann)
    for t in range(T_frames):
        Image.fromarray(frames[t]).save(os.path.join(dirs["images"], "clip", f"{t:05d}.jpg"), quality=95)
        if t < T_frames - 1:
            flow = np.stack([2.5 * np.sin(yy / 97.0 + 0.1 * t) + 1.25, 1.5 * np.cos(xx / 131.0 - 0.07 * t) - 0.5], -1).astype(np.float32)
            R.write_flo(os.path.join(dirs["flows"], "clip", f"{t:05d}.flo"), flow)
        fresh = []
        for i, ((cy, cx), (ry, rx), (vy, vx)) in enumerate(zip(centres, radii, vel)):
            m = (((yy - cy - vy * t) / (ry + 3 * i)) ** 2 + ((xx - cx - vx * t) / (rx - 2 * i)) ** 2 <= 1).astype(np.uint8)
            seg = rle.encode(m)
            fresh.append({"bbox": rle.to_bbox(seg), "score": round(float(rng.uniform(0.6, 0.99)), 2), "segmentation": seg,
                          "conf_score": "0.5", "ReID": rng.normal(0, 0.05, 128).round(4).tolist()})
        for _ in range(4):
            cy, cx = rng.uniform(60, 420), rng.uniform(80, 780)
            m = (((yy - cy) / rng.uniform(20, 60)) ** 2 + ((xx - cx) / rng.uniform(20, 80)) ** 2 <= 1).astype(np.uint8)
            seg = rle.encode(m)
            fresh.append({"bbox": rle.to_bbox(seg), "score": round(float(rng.uniform(0.5, 0.95)), 2), "segmentation": seg,
                          "conf_score": "0.5", "ReID": rng.normal(0, 0.3, 128).round(4).tolist()})
        del fresh[-1]["ReID"]
        with open(os.path.join(dirs["props"], "clip", f"{t:05d}.json"), "w") as f:
            json.dump(fresh, f)
    return dirs


def test_do_video_with_the_real_engines_against_the_replayed_restatement(tmp_path):
    """480x854, 3 objects, 8 frames, sub-pixel flows, the package's refinement and ReID engines (synthetic weights, reduced depth):
    what the engines returned is recorded and replayed into the restatement; selections and PNG index arrays are equal, scores within
    1e-12.  Both margins of the run are asserted (REAL_SEED was chosen so that they hold)."""
    from oracle import refinement_oracle as RO
    from oracle import reid_oracle as QO
    from test_gpu_plumbing import MIDDLE, REID_UNITS
    from premvos_amd import track
    from premvos_amd.refinement import RefinementNet
    from premvos_amd.refinement.driver import RefinementEngine
    from premvos_amd.reid import ReIDEngine, ReIDNet
    d = _real_tree(tmp_path, 8, 3, REAL_SEED)
    ref_eng = RefinementEngine(RefinementNet(RO.synth_weights(0, MIDDLE), MIDDLE))
    reid_eng = ReIDEngine(ReIDNet(QO.synth_weights(0, REID_UNITS), units=[(n_, f, k, s) for n_, _, f, k, s in REID_UNITS]))
    tr = track.Tracker(ref_eng, reid_eng, record=True)
    assert tr._direct                                                                           # masks stay in HBM through the engines
    log = track.do_video(os.path.join(d["images"], "clip") + "/", d["images"], d["anns"], d["props"], d["flows"], d["out"], ref_eng, reid_eng,
                         record=True, tracker=tr)
    calls = tr.engine_log
    eng = R.ReplayEngines([c["mask"] for c in calls if c["call"] == "refine"], [c["ReID"] for c in calls if c["call"] == "reid"],
                          [c["bbox"] for c in calls if c["call"] == "refine"])
    ref = R.do_video(os.path.join(d["images"], "clip") + "/", d["images"], d["anns"], d["props"], d["flows"], eng.do_refinement, eng.add_ReID)
    assert len(log) == len(ref) == 8 and eng.n_refine == 7 and eng.n_reid == 8
    mw, mp = R.margins(ref)
    print(f"real engines: weighted margin {mw:.3e}, paint margin {mp:.3e}, selections {[r['selected'].tolist() for r in ref]}")
    assert mw >= 1e-6 and mp >= 1e-6
    for t, (x, y) in enumerate(zip(log, ref)):
        assert x["selected"].tolist() == y["selected"].tolist(), t
        assert np.abs(x["weighted"] - y["weighted"]).max() <= TOL and np.abs(x["planes"] - y["planes"]).max() <= TOL
        assert np.array_equal(x["png"], y["png"]), t
        assert set(np.unique(x["png"])) <= {0, 1, 2, 3}


# ------------------------------------------------------------------------------- the loops' output files (premvos_amd.merge_out)
def test_three_loops_write_the_same_files_for_a_video_without_annotation(tmp_path, capsys):
    """Three 48x64 frames, no annotation, eval_dir and overlay_dir set: ``do_video`` (resident), ``do_videos_lockstep`` with two seats and
    ``prewarp.run_tree`` write the same all-zero PNGs, overlay JPEGs that are the plain encode of the frame, and no eval file."""
    from PIL import Image
    from premvos_amd import io_pipeline as iop
    from premvos_amd import jpeg, overlay, prewarp, track
    rng = np.random.default_rng(48)
    lay = {k: os.path.join(str(tmp_path), k) + "/" for k in ("images", "anns", "props", "flows")}
    for k in lay:
        os.makedirs(os.path.join(lay[k], "nobody"))
    for t in range(3):
        Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(os.path.join(lay["images"], "nobody", f"{t:05d}.jpg"), quality=95)
        if t < 2:
            R.write_flo(os.path.join(lay["flows"], "nobody", f"{t:05d}.flo"), np.zeros((48, 64, 2), np.float32))
    where = {p: {k: os.path.join(str(tmp_path), p, k) + "/" for k in ("out", "eval", "overlay")} for p in ("video", "lockstep", "prewarp")}
    w = where["video"]
    log = track.do_video(os.path.join(lay["images"], "nobody") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], w["out"], None, None,
                         eval_dir=w["eval"], overlay_dir=w["overlay"])
    assert [r["png_fn"] for r in log] == [os.path.join(w["out"], "nobody", f"{t:05d}.png") for t in range(3)]
    w = where["lockstep"]
    eng = type("E", (), {"max_boxes": 40})()                                                    # (no video takes a seat: no net runs)
    with iop.Writer() as writer:
        logs = track.do_videos_lockstep(["nobody"], dict(lay, out=w["out"]), 2, eng, eng, writer, eval_dir=w["eval"], overlay_dir=w["overlay"])
    assert len(logs["nobody"]) == 3
    w = where["prewarp"]
    r = prewarp.run_tree(str(tmp_path), ["nobody"], add_ReID=lambda props, fn, net: props, eval_dir=w["eval"], overlay_dir=w["overlay"],
                         lay=dict(lay, out=w["out"]))
    assert r["frames"] == 3
    assert capsys.readouterr().out.count("premvos_amd.track: nobody: no templates, not evaluated\n") == 3
    for t in range(3):
        plain = os.path.join(str(tmp_path), "plain.jpg")
        overlay.write_jpg(plain, overlay.forward(jpeg.imread(os.path.join(lay["images"], "nobody", f"{t:05d}.jpg"), torch.device("cuda", 0)), None))
        pngs = [open(os.path.join(where[p]["out"], "nobody", f"{t:05d}.png"), "rb").read() for p in where]
        jpgs = [open(os.path.join(where[p]["overlay"], "nobody", f"{t:05d}.jpg"), "rb").read() for p in where]
        assert pngs[0] == pngs[1] == pngs[2] and jpgs[0] == jpgs[1] == jpgs[2] == open(plain, "rb").read(), t
        im = Image.open(os.path.join(where["video"]["out"], "nobody", f"{t:05d}.png"))
        assert im.mode == "P" and im.size == (64, 48) and not np.array(im).any()
    for p in where:
        assert sorted(os.listdir(os.path.join(where[p]["out"], "nobody"))) == [f"{t:05d}.png" for t in range(3)]
        assert sorted(os.listdir(os.path.join(where[p]["overlay"], "nobody"))) == [f"{t:05d}.jpg" for t in range(3)]
        assert not os.path.exists(where[p]["eval"]) or os.listdir(where[p]["eval"]) == [], p


@pytest.mark.parametrize("n_ann", [2, 3])
def test_do_video_writes_an_eval_file_iff_three_frames_are_annotated(tmp_path, n_ann):
    """Three frames, one object, the reduced-depth engines: the video's count file exists iff its annotation folder holds three PNGs."""
    from test_gpu_track_lockstep import _engines, _lay, _video
    from premvos_amd import evaluate as ev
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(tmp_path)
    _video(lay, "clip", 3, 1, seed=11)
    for t in range(n_ann, 3):
        os.remove(os.path.join(lay["anns"], "clip", f"{t:05d}.png"))
    eval_dir = os.path.join(str(tmp_path), "eval")
    log = track.do_video(os.path.join(lay["images"], "clip") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"], ref_eng, reid_eng,
                         record=True, eval_dir=eval_dir, overlay_dir=lay["overlay"])
    assert len(log) == 3 and np.unique(log[0]["png"]).tolist() == [0, 1]
    assert sorted(os.listdir(os.path.join(lay["out"], "clip"))) == [f"{t:05d}.png" for t in range(3)]
    assert sorted(os.listdir(os.path.join(lay["overlay"], "clip"))) == [f"{t:05d}.jpg" for t in range(3)]
    assert os.path.isfile(os.path.join(eval_dir, "clip.json")) == (n_ann == 3)
    if n_ann == 3:
        assert ev.summarise(eval_dir, ["clip"]) == ev.evaluate(lay["out"], lay["anns"], ["clip"])


# ------------------------------------------------------------------------------------------------------------ the command
def test_the_command_on_a_tree_written_by_the_stream_and_reid_stages(tmp_path):
    """python -m premvos_amd.stream, the ReID stage, then python -m premvos_amd.track --root, all in this process, on a synthetic tree
    (reduced-depth nets, random weights): one PNG per frame, mode P, the VOC palette, pixel values within {0} + the annotation's ids;
    a video without annotation gets all-zero PNGs."""
    from PIL import Image
    from test_gpu_plumbing import REID_NETWORK, _make_tree
    from premvos_amd import stream, track
    from premvos_amd.reid import driver as qd
    root = tmp_path / "premvos"
    root.mkdir()
    videos = {"bear": 4, "camel": 3}
    _make_tree(root, videos=videos)
    (root / "code" / "refinement_net" / "configs").mkdir(parents=True)
    (root / "code" / "refinement_net" / "configs" / "live").write_text(json.dumps({"model": "live", "load": "../weights/refinement_specific_weights"}))
    reid_cfg = {"model": "Re-ID", "load": "../weights/ReID_general_weights", "input_size": [128, 128], "network": REID_NETWORK}
    (root / "code" / "ReID_net" / "configs" / "live").write_text(json.dumps(reid_cfg))
    (root / "code" / "ReID_net" / "configs" / "run").write_text(json.dumps(dict(
        reid_cfg, image_input_dir="../data/DAVIS/JPEGImages/480p/", bb_input_dir="../output/intermediate/refined_proposals/",
        output_dir="../output/intermediate/ReID_proposals/")))
    ann_dir = root / "data" / "DAVIS" / "Annotations" / "480p" / "bear"
    ann_dir.mkdir(parents=True)
    ann = np.zeros((120, 200), np.uint8)
    ann[20:70, 30:90] = 1
    ann[60:110, 120:180] = 3
    R.write_index_png(str(ann_dir / "00000.png"), ann)
    cwd = os.getcwd()
    try:
        assert track.main(["--root", str(root), "--check-only"]) == 2                         # nothing to merge yet: says what is missing
        assert stream.main(["--root", str(root), "--batch", "2", "--flow_weights", "weights/pwc.pth.tar", "--general_weights",
                            "weights/proposal_general_weights", "--specific_weights", "weights/specific.pt", "--refinement_weights",
                            "weights/refinement_specific_weights"]) == 0
        os.chdir(root / "code")
        assert qd.main(["ReID_net/configs/run"]) == 0
        os.chdir(cwd)
        assert track.main(["--root", str(root), "--check-only"]) == 0
        assert track.main(["--root", str(root)]) == 0
    finally:
        os.chdir(cwd)
    pal = track.voc_palette().reshape(-1)
    for name, n in videos.items():
        files = sorted(os.listdir(root / "output" / "final" / name))
        assert files == [f"{t:05d}.png" for t in range(n)]
        for t, fn in enumerate(files):
            im = Image.open(root / "output" / "final" / name / fn)
            px = np.array(im)
            assert im.mode == "P" and px.shape == (120, 200) and np.array_equal(np.array(im.getpalette(), np.uint8), pal)
            if name == "bear":
                assert set(np.unique(px)) <= {0, 1, 3}
                if t == 0:
                    assert np.array_equal(px, ann)          # the annotation objects are their own best candidates in their own frame
            else:
                assert not px.any()
