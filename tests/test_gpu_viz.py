"""csrc/viz_ops.hip on the GPU against tests/viz_restated.py (itself pinned to the executed reference by tests/test_cpu_viz.py):
premvos_viz_scores_u8 and premvos_reid_max_distance_f64 bit for bit, the sheet's JPEG against PIL, and the sheets of the loop
(``Tracker(viz=True)``, ``do_video(viz_dir=...)``, ``track --viz``), which must leave the loop's own outputs as they are.

Bounds: none.  Every byte of a sheet is a chain of float64 operations on the same operands in the same order (no contraction in the
kernel, no sum whose order could differ), and the distance sums run over the embedding index ascending on both sides."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_merge_modes as TM  # noqa: E402  (its synthetic tree and stub engines; nothing of it is collected here)
import viz_restated as V  # noqa: E402

TINT = np.array([0, 128, 0], np.uint8)


def _dev():
    from premvos_amd import _lib
    return _lib.resolve_device(None)


def _sheet(frame, masks, boxes, planes, weighted, gt, tint=None):
    from premvos_amd import viz
    dev = _dev()
    return viz.sheet(torch.from_numpy(np.ascontiguousarray(frame)).to(dev), torch.from_numpy(np.ascontiguousarray(masks)).to(dev), boxes,
                     planes, weighted, gt, tint)


@pytest.fixture(scope="module")
def fixture():
    return V.load_fixture()


@pytest.mark.parametrize("tag", ["t1p4", "t3p6", "dark"])
def test_the_kernel_writes_the_golden_sheets(fixture, tag):
    a = fixture
    args = [a[f"{tag}_{k}"] for k in ("frame", "masks", "boxes", "planes", "weighted", "gt")]
    want = V.bytescale(a[f"{tag}_canvas"])                                      # the executed reference's canvas, restated bytescale
    got = _sheet(*args).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, V.sheet_u8(*args, TINT))
    assert np.array_equal(_sheet(*args, tint=TINT).cpu().numpy(), got)          # the default tint; a second launch: the same bytes


def _seeded(seed, h, w, T, P, ours=False):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    masks, boxes = [], []
    for j in range(P):
        bw, bh = int(rng.integers(3, max(4, w // 2))), int(rng.integers(3, max(4, h // 2)))
        x, y = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        m = ((((yy - (y + bh / 2)) / (bh / 2)) ** 2 + ((xx - (x + bw / 2)) / (bw / 2)) ** 2) <= 1).astype(np.uint8) * (255 if j % 2 else 1)
        masks.append(m)
        boxes.append([x + rng.uniform(0, 0.99), y + rng.uniform(0, 0.99), bw + rng.uniform(0, 0.99), bh + rng.uniform(0, 0.99)])
    boxes[0] = [w - 7.0, h - 5.0, 20.0, 30.0]                                   # past the right and bottom edge: clipped to the frame
    boxes[1] = [3.0, 4.0, 102.0, 102.0] if min(h, w) > 110 else [0.0, 0.0, float(w + 1), float(h + 1)]   # a crop of exactly 101 / the frame
    if P > 3:
        boxes[3] = [5.0, 6.0, 1.5, 9.0]                                         # min(h, w) < 2: a black tile
    planes = rng.uniform(0, 1, (5, T, P))
    weighted = rng.uniform(0, 1, (T, P + 1))                                    # track_scores' layout: a threshold column behind the rows
    gt = rng.uniform(0, 1, (T, P))
    if ours:                                                                    # this package's rules, and a canvas with cmin < 0
        planes[1, 0, 2], planes[3, T - 1, 0], planes[0, 0, 1] = np.nan, np.inf, 1.25
        weighted[0, 1], weighted[T - 1, 0] = np.inf, np.nan
        gt[0, 0] = np.nan
        boxes[2] = [float(w + 3), 2.0, 9.0, 9.0]                                # outside the frame: empty after clipping
        boxes[P - 1] = [np.nan, 0.0, 5.0, 5.0]
    return frame, np.array(masks, np.uint8), np.array(boxes, np.float64), planes, weighted, gt


@pytest.mark.parametrize("h,w,T,P,ours", [(31, 45, 2, 5, False), (31, 45, 2, 5, True), (480, 854, 3, 8, False), (480, 854, 3, 8, True)])
def test_the_kernel_equals_the_restatement_on_seeded_cases(h, w, T, P, ours):
    frame, masks, boxes, planes, weighted, gt = _seeded(h * 7 + int(ours), h, w, T, P, ours)
    tint = np.array([200, 30, 90], np.uint8)
    want = V.sheet_u8(frame, masks, boxes, planes, weighted, gt, tint)
    got = _sheet(frame, masks, boxes, planes, weighted, gt, tint)
    again = _sheet(frame, masks, boxes, planes, weighted, gt, tint)
    assert tuple(got.shape) == (100 * (T + 1), 100 * P, 3)
    got, again = got.cpu().numpy(), again.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(again, got)
    if ours:
        assert want.min() == 0 and want.max() == 255 and np.nanmin(V.float_sheet(frame, masks, boxes, planes, weighted, gt, tint)) < 0
        zero = want[0, 0, 0]                                                    # what a 0 of the canvas becomes (a separator; cmin < 0)
        assert zero > 0 and (want[:100, 200:300] == zero).all() and (want[:100, 100 * (P - 1):] == zero).all()      # our rules' black tiles


def test_the_sheets_jpeg_is_the_file_pil_writes(fixture):
    from PIL import Image
    from premvos_amd import jpeg, viz
    a = fixture
    sheet = _sheet(*[a[f"t3p6_{k}"] for k in ("frame", "masks", "boxes", "planes", "weighted", "gt")])
    buf = io.BytesIO()
    Image.fromarray(sheet.cpu().numpy()).save(buf, "JPEG", quality=75)
    assert jpeg.encode(sheet, 75, "4:2:0") == buf.getvalue()
    assert jpeg.entropy_encode(viz.forward(sheet)) == buf.getvalue()


def test_viz_scores_takes_dicts_and_writes_the_file(fixture, tmp_path):
    """The reference's call shape: proposal dicts and an image file in, ``out_dir``/<video>/<frame>.jpg out."""
    from PIL import Image
    from premvos_amd import rle, viz
    a = fixture
    frame, masks, boxes, planes, weighted, gt = [a[f"t3p6_{k}"] for k in ("frame", "masks", "boxes", "planes", "weighted", "gt")]
    images, out_dir = os.path.join(str(tmp_path), "images") + "/", os.path.join(str(tmp_path), "viz") + "/"
    os.makedirs(os.path.join(images, "v"))
    image_fn = os.path.join(images, "v", "00007.jpg")
    Image.fromarray(frame).save(image_fn, quality=95)
    frame = np.asarray(Image.open(image_fn).convert("RGB"))                     # (what both sides read back)
    props = [{"bbox": b, "segmentation": rle.encode(m)} for b, m in zip(boxes, masks)]
    out_fn = viz.viz_scores(planes, weighted, props, image_fn, images, np.array([gt] * 5), out_dir)
    assert out_fn == out_dir + "v/00007.jpg"
    buf = io.BytesIO()
    Image.fromarray(V.sheet_u8(frame, masks, boxes, planes, weighted, gt, TINT)).save(buf, "JPEG", quality=75)
    assert open(out_fn, "rb").read() == buf.getvalue()


def test_sheet_refuses_wrong_inputs(fixture):
    from premvos_amd import _lib, viz
    a = fixture
    frame, masks, boxes, planes, weighted, gt = [a[f"t1p4_{k}"] for k in ("frame", "masks", "boxes", "planes", "weighted", "gt")]
    dev = _dev()
    f, m = torch.from_numpy(frame).to(dev), torch.from_numpy(masks).to(dev)
    with pytest.raises(ValueError):
        viz.sheet(f.cpu(), m, boxes, planes, weighted, gt)
    with pytest.raises(ValueError):
        viz.sheet(f, m[:, :-1], boxes, planes, weighted, gt)
    with pytest.raises(ValueError):
        viz.sheet(f, m, boxes[:-1], planes, weighted, gt)
    with pytest.raises(ValueError):
        viz.sheet(f, m, boxes, planes[:4], weighted, gt)
    big = np.zeros((5, 256, 4))
    with pytest.raises(_lib.PremvosError, match="255"):
        viz.sheet(f, m, boxes, big, np.zeros((256, 4)), np.zeros((256, 4)))


@pytest.mark.parametrize("T,N", [(1, 0), (1, 1), (3, 700), (5, 37)])
def test_max_reid_distance_equals_the_restatement(T, N):
    from premvos_amd import viz
    rng = np.random.default_rng(T * 1000 + N)
    t = rng.normal(0, 1.6, (T, 128))
    p = rng.normal(0, 1.6, (N, 128))
    if N > 2:
        p[1] = np.inf                                                           # a proposal without 'ReID'
        p[2] = t[0]                                                             # a distance of exactly 0
    want, over = V.max_distances_ordered(t, p)
    got, got_over = viz.max_reid_distance(t, p)
    again, _ = viz.max_reid_distance(torch.from_numpy(t).to(_dev()), torch.from_numpy(p).to(_dev()))
    assert got.dtype == torch.float64 and tuple(got.shape) == (T,)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(again.cpu().numpy(), want)
    assert np.array_equal(got_over.cpu().numpy(), over)
    if N == 700:
        assert 0 < over.sum() < T * N                                           # distances on both sides of 25
    if N == 0:
        assert not want.any()


def test_max_reid_distance_of_the_fixture_and_of_a_tree(fixture, tmp_path, capsys):
    import json
    from premvos_amd import viz
    a = fixture
    for v in a["mrd_videos"]:
        got, over = viz.max_reid_distance(a[f"mrd_{v}_templates"], a[f"mrd_{v}_props"])
        want, want_over = V.max_distances_ordered(a[f"mrd_{v}_templates"], a[f"mrd_{v}_props"])
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(over.cpu().numpy(), want_over)
        assert np.abs(want - a[f"mrd_{v}_max"]).max() <= 1e-12 * np.abs(a[f"mrd_{v}_max"]).max()
    # the host layer on a tree: templates from EVERY annotated frame, a frame without a proposal file, a proposal without 'ReID'
    TM._make_tree(tmp_path)
    root = str(tmp_path)
    os.remove(os.path.join(root, "output/intermediate/ReID_proposals/va/00001.json"))
    fn = os.path.join(root, "output/intermediate/ReID_proposals/vb/00002.json")
    props = json.load(open(fn))
    del props[0]["ReID"]
    json.dump(props, open(fn, "w"))
    eng = TM._StubEngines()
    res = viz.max_reid_distance_tree(root, ["va", "vb"], "stub ReID engine", eng.add_ReID)
    out = capsys.readouterr().out
    assert "va: max ReID distance per template" in out and "compiled in: 25" in out
    saved = json.load(open(os.path.join(root, "output", "max_reid_distance.json")))
    assert saved == res and saved["compiled_in"] == 25 and sorted(saved["videos"]) == ["va", "vb"]
    assert not os.path.exists(os.path.join(root, "output", "final"))
    for v, n_obj in (("va", 2), ("vb", 1)):
        embs = []
        for t in range(TM.FRAMES):
            pf = os.path.join(root, f"output/intermediate/ReID_proposals/{v}/{t:05d}.json")
            for p in (json.load(open(pf)) if os.path.exists(pf) else []):
                embs.append(np.asarray(p["ReID"], np.float64) if "ReID" in p else np.full(128, np.inf))
        templ = np.concatenate(eng.reid[:TM.FRAMES] if v == "va" else eng.reid[TM.FRAMES:])     # every frame is annotated: FRAMES x objects
        assert templ.shape == (TM.FRAMES * n_obj, 128)
        want, over = V.max_distances_ordered(templ, np.array(embs))
        assert saved["videos"][v]["per_template"] == want.tolist() and saved["videos"][v]["over"] == int(over.sum())
        assert saved["videos"][v]["pairs"] == len(templ) * len(embs) and saved["videos"][v]["max"] == want.max()
    assert saved["max"] == max(saved["videos"][v]["max"] for v in ("va", "vb"))


def _texture_frames(root, name, n):
    """frames with something in them (the tree's are flat grey), as JPEG files: both sides read them back through PIL"""
    from PIL import Image
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[:TM.H, :TM.W]
    for t in range(n):
        f = np.stack([(yy * 9 + xx * 5 + 11 * t) % 256, (yy * 4 + xx * 7) % 256, (yy * xx + 40 * t) % 256], axis=2) + rng.integers(0, 20, (TM.H, TM.W, 3))
        Image.fromarray(np.clip(f, 0, 255).astype(np.uint8)).save(os.path.join(root, f"data/DAVIS/JPEGImages/480p/{name}/{t:05d}.jpg"), quality=95)


@pytest.mark.parametrize("oracle", [False, True])
def test_do_video_with_sheets_leaves_the_loop_as_it_is(tmp_path, oracle):
    from PIL import Image
    from premvos_amd import track
    TM._make_tree(tmp_path)
    root = str(tmp_path)
    os.remove(os.path.join(root, "data/DAVIS/JPEGImages/480p/va/00003.jpg"))                  # a 3-frame video
    _texture_frames(root, "va", 3)
    lay = track._layout(root)
    runs = {}
    for key, viz_dir in (("plain", None), ("viz", os.path.join(root, "sheets") + "/")):
        eng = TM._StubEngines()
        out = os.path.join(root, "out_" + key) + "/"
        runs[key] = (track.do_video(os.path.join(lay["images"], "va") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], out,
                                    "stub refinement engine", "stub ReID engine", eng.do_refinement, eng.add_ReID, record=True,
                                    oracle=oracle, viz_dir=viz_dir), out, eng)
    (plain, out_p, eng_p), (withviz, out_v, eng_v) = runs["plain"], runs["viz"]
    assert len(plain) == len(withviz) == 3
    T = 2
    for t, (a, b) in enumerate(zip(plain, withviz)):
        assert open(os.path.join(out_p, "va", f"{t:05d}.png"), "rb").read() == open(os.path.join(out_v, "va", f"{t:05d}.png"), "rb").read()
        for k in ("selected", "weighted", "planes", "final_score", "object_score", "labels", "png"):
            assert np.array_equal(a[k], b[k]), (t, k)
        assert "sheet" not in a
        P = b["planes"].shape[2]
        frame = np.asarray(Image.open(os.path.join(lay["images"], "va", f"{t:05d}.jpg")).convert("RGB"))
        assert b["viz_masks"].shape == (P, TM.H, TM.W) and b["viz_boxes"].shape == (P, 4) and b["viz_gt"].shape == (T, P)
        want = V.sheet_u8(frame, b["viz_masks"], b["viz_boxes"], b["planes"], b["weighted"], b["viz_gt"], TINT)
        assert b["sheet"].shape == (100 * (T + 1), 100 * P, 3) and np.array_equal(b["sheet"], want), t
        # the boxes: the fresh proposals' are the JSON's; frame 0's carried ones read_ann's, later the warped masks' (what the engines saw)
        fresh = track.read_props(os.path.join(lay["props"], "va", f"{t:05d}.json"))
        assert np.array_equal(b["viz_boxes"][T:], np.array([p["bbox"] for p in fresh], np.float64))
        carried = np.array([p["bbox"] for p in track.read_ann(os.path.join(lay["anns"], "va", "00000.png"))]) if t == 0 else eng_v.bbox[t - 1]
        assert np.array_equal(b["viz_boxes"][:T], carried)
        # gt: the IoU of every candidate with the annotation's object k + 1; with the oracle the planes ARE that
        import merge_modes_restated as MM
        gt_planes = MM.gt_planes_from_counts(*MM.label_overlap(b["viz_masks"], np.array(Image.open(os.path.join(lay["anns"], "va", f"{t:05d}.png"))), T))
        assert np.abs(b["viz_gt"] - gt_planes[0]).max() <= 1e-12
        if oracle:
            assert np.array_equal(b["viz_gt"], b["planes"][0]) and np.array_equal(b["planes"][0], b["planes"][4])
        buf = io.BytesIO()
        Image.fromarray(b["sheet"]).save(buf, "JPEG", quality=75)
        assert open(os.path.join(root, "sheets", "va", f"{t:05d}.jpg"), "rb").read() == buf.getvalue()
    assert sorted(os.listdir(os.path.join(root, "sheets", "va"))) == [f"{t:05d}.jpg" for t in range(3)]
    for x, y in zip(eng_p.masks + eng_p.reid + eng_p.bbox, eng_v.masks + eng_v.reid + eng_v.bbox):
        assert np.array_equal(x, y)


def test_do_video_refuses_sheets_it_cannot_draw(tmp_path):
    from premvos_amd import _lib, track
    TM._make_tree(tmp_path)
    root = str(tmp_path)
    lay = track._layout(root)
    os.remove(os.path.join(lay["anns"], "va", "00002.png"))
    eng = TM._StubEngines()
    args = (os.path.join(lay["images"], "va") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], os.path.join(root, "o") + "/",
            "r", "q", eng.do_refinement, eng.add_ReID)
    with pytest.raises(_lib.PremvosError, match="annotation for every frame"):
        track.do_video(*args, viz_dir=os.path.join(root, "s") + "/")
    with pytest.raises(_lib.PremvosError, match="resident"):
        track.do_video(*args, resident=False, viz_dir=os.path.join(root, "s") + "/")
    assert not os.path.exists(os.path.join(root, "s")) and not os.path.exists(os.path.join(root, "o"))
    tr = track.Tracker("r", "q", eng.do_refinement, eng.add_ReID, viz=True)
    tr.add_templates(track.read_ann(os.path.join(lay["anns"], "va", "00000.png")), os.path.join(lay["images"], "va", "00000.jpg"))
    with pytest.raises(_lib.PremvosError, match="frame"):
        tr.step([], None, None, gt=np.zeros((TM.H, TM.W), np.uint8))


def test_the_gt_row_follows_the_templates_ids():
    """Template ids 1, 2, 4 (the golden track's): row k is the IoU with the annotation's object ids[k], not with label k + 1."""
    import merge_modes_restated as MM
    from premvos_amd import rle, track
    eng = TM._StubEngines()
    ann = np.zeros((TM.H, TM.W), np.uint8)
    objs = [TM._ell(6, 7, 4, 5), TM._ell(15, 20, 5, 6), TM._ell(18, 8, 3, 4)]
    for i, m in zip((1, 2, 4), objs):
        ann[m != 0] = i
    templates = [{"id": i, "segmentation": rle.encode((ann == i).astype(np.uint8)), "score": 1.0, "bbox": np.array(rle.to_bbox(rle.encode((ann == i).astype(np.uint8))))}
                 for i in (1, 2, 4)]
    tr = track.Tracker("r", "q", eng.do_refinement, eng.add_ReID, record=True, viz=True)
    tr.add_templates(templates, "frame 0")
    shifted = np.roll(ann, 1, axis=1)                                           # the frame's annotation: everything one pixel to the right
    frame = np.random.default_rng(1).integers(0, 256, (TM.H, TM.W, 3), dtype=np.uint8)
    r = tr.step([], None, None, gt=shifted, frame=frame)
    lut = np.zeros(256, np.uint8)
    lut[[1, 2, 4]] = [1, 2, 3]
    want = MM.gt_planes_from_counts(*MM.label_overlap(r["viz_masks"], lut[shifted], 3))[0]
    assert r["viz_gt"].shape == (3, 3) and np.abs(r["viz_gt"] - want).max() <= 1e-12 and (np.diag(want) > 0.5).all()
    assert np.array_equal(r["sheet"], V.sheet_u8(frame, r["viz_masks"], r["viz_boxes"], r["planes"], r["weighted"], r["viz_gt"], TINT))


def test_the_command_writes_the_sheets(tmp_path, monkeypatch):
    from PIL import Image
    from premvos_amd import track
    TM._make_tree(tmp_path)
    root = str(tmp_path)
    TM._run_command(tmp_path, monkeypatch, ["--viz"])
    lay = track.mode_layout(root)
    for name, objs in TM.VIDEOS.items():
        T = len(objs)
        for t in range(TM.FRAMES):
            P = T + len(track.read_props(os.path.join(lay["props"], name, f"{t:05d}.json")))
            im = Image.open(os.path.join(root, "output", "viz", name, f"{t:05d}.jpg"))
            assert im.format == "JPEG" and im.size == (100 * P, 100 * (T + 1))
            assert os.path.isfile(os.path.join(lay["out"], name, f"{t:05d}.png"))
    assert sorted(os.listdir(os.path.join(root, "output"))) == ["final", "intermediate", "viz"]
