"""The merge stage without a GPU: the numpy restatement (tests/track_restated.py) reproduces the reference EXECUTED
(tests/golden/track_ref.npz + track_host_refs.json, written by tools/make_golden_track.py from MergeTrack/merge.py and
merge_functions.py unmodified), and the host side of premvos_amd.track -- files, palette, templates, the command line -- against the
same fixture.  Exact: planes 0 / 3 / 4, selections, labels, masks, PNG indices.  Within 1e-12: planes 1 / 2 and the weighted scores
(numpy's norm / dot go through BLAS, whose summation order is its own).  In ``do_video`` a warped candidate's 'score' is 0.5 * (its
final score + 1), i.e. a function of the previous frame's weighted score, so from the second frame on planes 0 / 3 / 4 inherit that
1e-12; they are exact in the first frame and in every direct case.  No case is skipped for being close: the generator only
writes a fixture whose margins are >= 1e-6, and that is asserted here."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import track_restated as R
from premvos_amd import rle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def _close_planes(got, ref, exact=True):
    assert got.shape == ref.shape
    for k in (0, 3, 4):
        assert np.array_equal(got[k], ref[k]) if exact else np.abs(got[k] - ref[k]).max() <= TOL, k
    for k in (1, 2):
        assert np.abs(got[k] - ref[k]).max() <= TOL, (k, np.abs(got[k] - ref[k]).max())


def test_fixture_margins_hold(fx):
    _, g = fx
    assert g["min_margin_weighted"] >= 1e-6 and g["min_margin_paint"] >= 1e-6
    assert g["videos"]["alpha"]["fresh_beats_warped_frames"] and g["videos"]["alpha"]["object_left_frames"]
    assert "00003" not in g["videos"]["alpha"]["proposals"]                     # the missing proposal file
    assert any("ReID" not in p for p in g["videos"]["alpha"]["proposals"]["00002"])


def test_constants_are_the_references(fx):
    from premvos_amd import track
    _, g = fx
    assert track.WEIGHTS.tolist() == g["weights"] == R.WEIGHTS.tolist()
    assert track.NORMALISED_WEIGHTS.tolist() == g["normalised_weights"]
    assert track.SCORE_THRESH == g["score_thresh"] == R.SCORE_THRESH and track.MAX_REID_DISTANCE == g["max_reid_distance"]


@pytest.mark.parametrize("tag", ["scores1", "scores3"])
def test_restated_calculate_scores(fx, tag):
    a, g = fx
    props = R.with_embeddings(g[tag]["proposals"], a[f"{tag}_emb_p"])
    templs = R.with_embeddings(g[tag]["templates"], a[f"{tag}_emb_t"])
    planes = R.calculate_scores(props, templs)
    _close_planes(planes, a[f"{tag}_planes"])
    assert np.abs(R.weighted_from_planes(planes) - a[f"{tag}_weighted"]).max() <= TOL
    if tag == "scores3":
        ref = a[f"{tag}_planes"]
        assert (ref[1][:, -2] == 0).all() and (ref[1][:, -1] == 0).all()         # no ReID; farther than MAX_REID_DISTANCE
        assert (ref[3][1] == 0).all()                                             # a template score below 0.5 switches the warp score off


def test_restated_selection_on_crafted_scores(fx):
    a, g = fx
    props = [dict(p) for p in g["select"]["proposals"]]
    templs = [{"id": i} for i in g["select"]["template_ids"]]
    sel, index = R.calculate_selected_props(props, a["select_weighted"], templs, g["score_thresh"], a["select_object"])
    assert index.tolist() == a["select_index"].tolist() == [2, 4, 1, 0]
    assert np.array_equal([p["final_score"] for p in sel], a["select_final"])
    assert np.array_equal([p["object_score"] for p in sel], a["select_objscore"])
    assert [p["id"] for p in sel] == g["select"]["ids"]
    assert props[-1]["segmentation"]["counts"] == g["select"]["empty_counts"] and list(props[-1]["bbox"]) == g["select"]["empty_bbox"]


def test_restated_remove_mask_overlap(fx):
    a, g = fx
    sel = [{"segmentation": rle.encode(m), "final_score": float(s), "object_score": 0.1 * i, "id": i + 2}
           for i, (m, s) in enumerate(zip(a["overlap_in"], a["overlap_scores"]))]
    out = R.remove_mask_overlap(sel)
    assert np.array_equal(np.array([p["mask"] for p in out]), a["overlap_out"])
    assert np.array_equal(np.array([p["bbox"] for p in out]), a["overlap_bbox"])
    assert sorted(out[0].keys()) == g["overlap"]["keys"]
    for p, q in zip(out, g["overlap"]["out"]):
        assert p["segmentation"] == q["segmentation"] and p["final_score"] == q["final_score"] and p["id"] == q["id"]
        assert p["object_score"] == q["object_score"]
    assert (a["overlap_in"][0] & a["overlap_in"][1]).any()                       # the case does overlap


@pytest.mark.parametrize("name", ["alpha", "beta"])
def test_restated_do_video(fx, tmp_path, name):
    a, g = fx
    d = R.make_video_tree(tmp_path, name, a, g)
    with_ann = g["videos"][name]["with_annotation"]
    eng = R.ReplayEngines(a[f"v_{name}_refine_mask"], a[f"v_{name}_reid"], a[f"v_{name}_refine_bbox"]) if with_ann else R.ReplayEngines([], [])
    log = R.do_video(os.path.join(d["images"], name) + "/", d["images"], d["anns"], d["props"], d["flows"], eng.do_refinement, eng.add_ReID)
    assert len(log) == g["videos"][name]["frames"]
    assert np.array_equal(np.array([r["png"] for r in log]), a[f"v_{name}_png"])
    if not with_ann:
        assert not a[f"v_{name}_png"].any() and eng.n_reid == 0
        return
    assert eng.n_refine == len(log) - 1 and eng.n_reid == len(log)
    for t, r in enumerate(log):
        assert r["selected"].tolist() == a[f"v_{name}_selected"][t].tolist(), t
        _close_planes(r["planes"], a[f"v_{name}_planes_{t}"], exact=(t == 0))
        assert np.abs(r["weighted"][:, :-1] - a[f"v_{name}_weighted_{t}"]).max() <= TOL
        assert np.abs(r["final_score"] - a[f"v_{name}_final_score"][t]).max() <= TOL
        assert np.abs(r["object_score"] - a[f"v_{name}_object_score"][t]).max() <= TOL
    mw, mp = R.margins(log)
    assert mw >= 1e-6 and mp >= 1e-6


def test_track_read_ann_read_props_update_templates(fx, tmp_path):
    from premvos_amd import track
    a, g = fx
    R.write_index_png(str(tmp_path / "a.png"), a["ann"])
    got = track.read_ann(str(tmp_path / "a.png"))
    assert len(got) == len(g["read_ann"]) == 3
    for p, q in zip(got, g["read_ann"]):
        assert int(p["id"]) == q["id"] and list(p["bbox"]) == q["bbox"] and p["segmentation"] == q["segmentation"]
        assert p["conf_score"] == q["conf_score"] and p["score"] == q["score"] and set(p) == set(q)
    # read_props: all-inf embedding for a proposal without 'ReID'; a missing or broken file is an empty list
    d = R.make_video_tree(tmp_path / "t", "alpha", a, g)
    props = track.read_props(os.path.join(d["props"], "alpha", "00002.json"))
    assert np.isinf(props[-1]["ReID"]).all() and len(props[-1]["ReID"]) == 128 and isinstance(props[0]["ReID"], list)
    assert track.read_props(os.path.join(d["props"], "alpha", "00003.json")) == []
    (tmp_path / "broken.json").write_text("[{")
    assert track.read_props(str(tmp_path / "broken.json")) == []
    u = g["update_templates"]
    nxt = json.loads(json.dumps(u["next_props"]))
    assert track.update_templates(u["templates"], nxt) == u["out"] and nxt == u["next_props_after"] == u["next_props"]


def test_palette_and_png_writer(fx, tmp_path):
    from PIL import Image
    from premvos_amd import track
    a, g = fx
    assert np.array_equal(track.voc_palette().reshape(-1), a["png_palette"])
    props = [{"mask": (a["ann"] == i).astype(np.uint8), "id": i} for i in g["save_pngs"]["ids"]]
    fn = str(tmp_path / "out" / "sub" / "00003.png")                              # the folder does not exist yet
    track.save_pngs(props, fn)
    im = Image.open(fn)
    assert im.mode == g["save_pngs"]["mode"] == "P"
    assert np.array_equal(np.array(im), a["png_index"]) and np.array_equal(np.array(im.getpalette(), np.uint8), a["png_palette"])
    track.save_pngs([{"mask": np.zeros_like(a["ann"])}], str(tmp_path / "out" / "sub" / "00004.png"), empty=True)
    assert np.array_equal(np.array(Image.open(str(tmp_path / "out" / "sub" / "00004.png"))), a["png_empty_index"])


def test_boundaries_from_segmentations_are_the_pooled_layout():
    from premvos_amd import track
    rng = np.random.default_rng(2)
    masks = [(rng.random((7, 5)) < 0.5).astype(np.uint8), np.zeros((7, 5), np.uint8), np.ones((7, 5), np.uint8)]
    pool, off = track.boundaries_from_segmentations([rle.encode(m) for m in masks])
    assert off[0] == 0 and off[-1] == len(pool) and pool.dtype == np.int32
    for i, m in enumerate(masks):
        flat = m.reshape(-1, order="F")
        q = np.arange(flat.size)
        b = pool[off[i]:off[i + 1]]
        assert np.array_equal((np.searchsorted(b, q, side="right") & 1).astype(np.uint8), flat)


def test_vectorised_counts_decoder_equals_the_plain_one():
    from premvos_amd import track
    rng = np.random.default_rng(9)
    masks = [np.zeros((7, 5), np.uint8), np.ones((7, 5), np.uint8), (rng.random((64, 33)) < 0.5).astype(np.uint8),
             (rng.random((480, 854)) < 0.01).astype(np.uint8), np.pad(np.ones((300, 500), np.uint8), ((90, 90), (177, 177)))]
    masks[3][:, 400:] = 0                                                          # a long run: counts above 2^15, negative differences
    for m in masks:
        s = rle.encode(m)["counts"]
        assert track.counts_from_string(s).tolist() == rle.string_to_counts(s) == rle.counts_from_mask(m).tolist()
        assert track.counts_from_string(s.encode("ascii")).tolist() == rle.string_to_counts(s)
    assert track.counts_from_string("").tolist() == []


def test_device_functions_raise_without_a_gpu(fx):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from premvos_amd import _lib, track
    a, g = fx
    props = R.with_embeddings(g["scores1"]["proposals"], a["scores1_emb_p"])
    templs = R.with_embeddings(g["scores1"]["templates"], a["scores1_emb_t"])
    with pytest.raises(_lib.PremvosError):
        track.calculate_scores(props, templs)
    with pytest.raises(_lib.PremvosError):
        track.remove_mask_overlap([{"segmentation": rle.encode(a["overlap_in"][0]), "final_score": 0.5, "object_score": 0.1, "id": 1}])
    with pytest.raises(_lib.PremvosError):
        track.decode_segmentations([rle.encode(a["overlap_in"][0])])
    with pytest.raises(_lib.PremvosError):
        track.Tracker(None, None)


def test_entry_points_validate_before_any_hip_call():
    import ctypes as C
    from premvos_amd import _lib
    lib = _lib.load()
    assert lib.premvos_rle_decode_u8(None, 0, None, 0, 4, 4, None, None) == 0           # n = 0: nothing to do
    assert lib.premvos_rle_decode_u8(None, 0, None, 2, 4, 4, None, None) == -1 and b"null" in lib.premvos_last_error()
    w = (C.c_double * 5)()
    assert lib.premvos_track_scores_f64(None, None, None, None, None, None, None, 1, 1, w, 1e-10, None, None, None, None, None, None) == -1
    one = C.c_void_p(16)                                                                 # non-null, never dereferenced: the limits come first
    assert lib.premvos_track_scores_f64(one, one, one, one, one, one, one, 256, 4, w, 1e-10, one, one, one, one, one, None) == -1
    assert b"255" in lib.premvos_last_error()
    assert lib.premvos_track_paint_u8(one, 4, 8, 8, one, one, one, 256, one, one, one, None) == -1 and b"255" in lib.premvos_last_error()
    assert lib.premvos_track_paint_u8(one, 4, 8, 8, None, one, one, 3, one, one, one, None) == -1


def test_header_and_signatures_carry_the_three_names():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "track_ops.hip")).read()
    for name in ("premvos_rle_decode_u8", "premvos_track_scores_f64", "premvos_track_paint_u8"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES and f'extern "C" int {name}(' in src
    assert src.startswith("// hipcc-flags: -ffp-contract=off")
    from premvos_amd import build
    assert "-ffp-contract=off" in build._file_flags(os.path.join(ROOT, "premvos_amd", "csrc", "track_ops.hip"))


def test_check_only_names_what_is_missing(tmp_path, capsys):
    from premvos_amd import track
    assert track.main(["--root", str(tmp_path), "--check-only"]) == 2
    out = capsys.readouterr().out
    for piece in ("JPEGImages/480p", "ReID_proposals", "intermediate/flow", "refinement_net/configs/live", "ReID_net/configs/live"):
        assert piece in out, piece
    for sub in ("data/DAVIS/JPEGImages/480p", "output/intermediate/ReID_proposals", "output/intermediate/flow", "code/refinement_net/configs",
                "code/ReID_net/configs"):
        (tmp_path / sub).mkdir(parents=True)
    (tmp_path / "code/refinement_net/configs/live").write_text("{}")
    assert track.main(["--root", str(tmp_path), "--check-only"]) == 2
    out = capsys.readouterr().out
    assert "ReID_net/configs/live" in out and "JPEGImages" not in out
    (tmp_path / "code/ReID_net/configs/live").write_text("{}")
    assert track.main(["--root", str(tmp_path), "--check-only"]) == 0


def test_accept_davis_takes_merge_package(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("accept_davis", os.path.join(ROOT, "tools", "accept_davis.py"))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    assert A.main(["--root", str(tmp_path), "--merge", "package", "--check-only"]) == 2          # parses; the empty tree lacks its inputs
    assert "inputs are not ready" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        A.main(["--root", str(tmp_path), "--merge", "nothing-like-it"])
