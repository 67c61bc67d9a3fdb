"""The host side of the oracle merge and the probabilistic combination (no GPU): the numpy restatement (tests/merge_modes_restated.py)
against the reference executed (tests/golden/merge_modes_ref.npz, tools/make_golden_merge_modes.py); header / binding / document
agreement of the three entries of merge_modes_ops.hip; their argument checks (before any HIP call, so they run here); the command line.

Bounds.  The IoU planes are one correctly rounded division of the same integers and the probabilities the same chain of operations in
the same order (the fixture's P < 8, below numpy's pairwise blocking): 1e-12 leaves room for another libm's exp only.  Labels, masks,
ids, boxes: exact."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ENTRIES = (("premvos_mask_label_overlap_u8", 9), ("premvos_track_gt_scores_f64", 13), ("premvos_track_combine_f64", 15))
CASES = ("t1p1", "tie", "t3p6", "edge")
TOL = 1e-12


@pytest.mark.parametrize("tag", CASES)
def test_the_restatement_reproduces_the_reference(tag):
    import merge_modes_restated as MM
    from premvos_amd import rle
    a = MM.load_fixture()
    masks, ws, labels = a[f"{tag}_masks"], a[f"{tag}_weighted"], a[f"{tag}_labels"]
    T, P = ws.shape
    templates = [{"id": t + 1} for t in range(T)]
    props = [{"segmentation": s} for s in MM.segs_of(masks)]
    gt_props = [{"id": int(i), "segmentation": rle.encode((labels == i).astype(np.uint8))} for i in np.unique(labels) if i != 0]
    planes = MM.calculate_gt_scores(props, gt_props, templates)
    assert planes.shape == (5, T, P) and np.abs(planes - a[f"{tag}_gt_planes"]).max() <= TOL
    assert np.array_equal(planes, MM.gt_planes_from_counts(*MM.label_overlap(masks, labels, T)))
    out, probs, full = MM.probabilitic_combination(props, ws, templates, 1e-10)
    assert MM.gap_violations(full) == 0
    assert np.abs(probs - a[f"{tag}_probs"]).max() <= TOL
    assert np.array_equal(np.array([p["mask"] for p in out]), a[f"{tag}_out_masks"])
    assert [p["id"] for p in out] == a[f"{tag}_out_ids"].tolist()                      # ids 1 .. T: the template's id IS index + 1
    assert np.array_equal(np.array([p["final_score"] for p in out]), a[f"{tag}_out_final_score"])
    assert np.array_equal(np.array([p["bbox"] for p in out], np.float64), a[f"{tag}_out_bbox"])
    assert set(out[0]) == {"segmentation", "bbox", "final_score", "mask", "id"}


def test_the_fixture_holds_the_crafted_cases():
    import merge_modes_restated as MM
    a = MM.load_fixture()
    assert a["t1p1_weighted"].shape == (1, 1) and a["tie_weighted"].tolist() == [[0.5, 0.5]] and a["t3p6_masks"].shape == (6, 24, 32)
    m = a["tie_masks"] != 0
    one, both = m[0] ^ m[1], m[0] & m[1]
    assert one.any() and both.any()
    assert not a["tie_out_masks"][0][one].any() and a["tie_out_masks"][0][both].all()   # 0.5 against 0.5: the background wins the tie
    assert a["edge_masks"][0].all() and not a["edge_masks"][1].any()                    # a full-frame proposal, an all-empty one
    assert 2 not in a["edge_labels"] and not a["edge_gt_planes"][:, 1].any()            # the annotation lacks object 2: its row is 0
    assert a["edge_gt_planes"][:, 0].any() and (a["edge_gt_planes"][:, :, 1] == 0).all()
    assert (a["smallest_gaps"] >= 1e-9).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "merge_modes_ref.npz")) < 100 * 1024
    assert all(v.dtype != object for v in a.values())                                   # arrays only


def test_our_rules_against_the_restatement():
    """Non-finite weighted scores count as 0; ids outside 1 .. T are refused by both sides."""
    import merge_modes_restated as MM
    from premvos_amd import _lib, rle, track
    probs, denom, best = MM.probs_from_weighted(np.array([[np.nan, 0.0, np.inf, -np.inf]]))
    assert np.array_equal(probs, np.full((1, 4), 0.25)) and denom[0] == 1.0 and best[0] == 0.0
    seg = rle.encode(np.ones((4, 5), np.uint8))
    with pytest.raises(_lib.PremvosError, match="annotation id 3"):
        track.label_map_of([{"id": 3, "segmentation": seg}], 2, 4, 5)
    with pytest.raises(_lib.PremvosError, match="overlap"):
        track.label_map_of([{"id": 1, "segmentation": seg}, {"id": 2, "segmentation": seg}], 2, 4, 5)
    lab = track.label_map_of([{"id": 2, "segmentation": seg}], 2, 4, 5)
    assert lab.dtype == np.uint8 and (lab == 2).all()
    with pytest.raises(AssertionError):
        MM.calculate_gt_scores([{"segmentation": seg}], [{"id": 3, "segmentation": seg}], [{"id": 1}, {"id": 2}])


def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    path = os.path.join(ROOT, "premvos_amd", "csrc", "merge_modes_ops.hip")
    src = open(path).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.premvos_abi_version() == 21                           # additive: the version stays
    for name, nargs in ENTRIES:
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert decl.count(",") + 1 == nargs, name
        assert f'extern "C" int {name}(' in src
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for cite in ("merge_functions.py:78-94", "merge_functions.py:151-195"):
        assert cite in hdr, cite
    assert src.startswith("// hipcc-flags: -ffp-contract=off\n") and "-ffp-contract=off" in build._file_flags(path)
    assert "#if" not in src
    assert not re.search(r"atomicAdd\([^;]*(float|double)", src) and "atomicAdd(&inter[" in src   # integer atomics only
    assert not re.search(r"atomic(Max|Min|Exch|CAS)|unsafeAtomic", src)
    # the selection pass is shared through a header, not copied
    sel = "premvos::track_select_rows("
    assert sel in src and sel in open(os.path.join(ROOT, "premvos_amd", "csrc", "track_ops.hip")).read()
    assert src.count("s_v[") == 0 and '#include "track_select.h"' in src


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.float64)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    def overlap(masks=one, P=2, labels=one, T=2, hw=35, inter=one, area_p=one, area_l=one):
        return lib.premvos_mask_label_overlap_u8(masks, P, labels, T, hw, inter, area_p, area_l, None)

    def scores(inter=one, area_p=one, area_l=one, T=2, P=3, wts=one, planes=one, weighted=one, selected=one, fs=one, obj=one):
        return lib.premvos_track_gt_scores_f64(inter, area_p, area_l, T, P, wts, 1e-10, planes, weighted, selected, fs, obj, None)

    def combine(masks=one, P=3, h=5, w=7, weighted=one, stride=4, ids=one, T=2, probs=one, denom=one, fs=one, labels=one, idmap=one,
                refined=one):
        return lib.premvos_track_combine_f64(masks, P, h, w, weighted, stride, ids, T, probs, denom, fs, labels, idmap, refined, None)

    for kw in ("masks", "labels", "inter", "area_p", "area_l"):
        refused(overlap(**{kw: None}), b"null")
    for kw in ({"P": 0}, {"T": 0}, {"hw": 0}, {"P": -1}, {"hw": 1 << 31}):
        refused(overlap(**kw), b"bad dims")
    refused(overlap(T=256), b"255")
    for kw in ("inter", "area_p", "area_l", "wts", "planes", "weighted", "selected", "fs", "obj"):
        refused(scores(**{kw: None}), b"null")
    for kw in ({"T": 0}, {"P": 0}, {"T": -3}):
        refused(scores(**kw), b"bad dims")
    refused(scores(T=256), b"255")
    refused(scores(P=65536), b"65535")
    for kw in ("masks", "weighted", "ids", "probs", "denom", "fs", "labels", "idmap", "refined"):
        refused(combine(**{kw: None}), b"null")
    for kw in ({"P": 0}, {"h": 0}, {"w": -1}, {"T": 0}, {"h": 1 << 16, "w": 1 << 15}):
        refused(combine(**kw), b"bad dims")
    refused(combine(T=256), b"255")
    refused(combine(stride=2), b"stride")


def test_command_line(tmp_path, capsys):
    from PIL import Image
    from premvos_amd import track
    import track_restated as R
    for argv, word in ((["--combine", "probabilistic", "--lockstep", "2"], "not with --lockstep"), (["--oracle", "--lockstep", "3"], "not with --lockstep"),
                       (["--oracle", "--prewarp"], "not with --prewarp"), (["--combine", "probabilistic", "--prewarp-search", "4"], "not with --prewarp"),
                       (["--combine", "softmax"], "--combine")):
        with pytest.raises(SystemExit) as e:
            track.main(["--root", "/nonexistent"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert track.main(["--root", "/nonexistent", "--combine", "argmax", "--lockstep", "2", "--check-only"]) == 2      # the default is no mode
    assert track.main(["--root", "/nonexistent", "--combine", "probabilistic", "--oracle", "--eval", "--overlay", "--check-only"]) == 2
    capsys.readouterr()
    with pytest.raises(SystemExit):
        track.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--combine", "--oracle", "merge_functions.py:151-195", "merge_functions.py:78-94", "output/final_prob", "output/final_oracle",
                 "output/final_oracle_prob"):
        assert word in text, word
    # the four places, none of them the live loop's
    assert track.mode_suffix() == "" and track.mode_layout("/r")["out"] == track._layout("/r")["out"] == "/r/output/final/"
    got = {(c, o): track.mode_layout("/r", c, o) for c in track.COMBINE_MODES for o in (False, True)}
    assert [got[k]["out"] for k in (("argmax", False), ("probabilistic", False), ("argmax", True), ("probabilistic", True))] == \
        ["/r/output/final/", "/r/output/final_prob/", "/r/output/final_oracle/", "/r/output/final_oracle_prob/"]
    for (c, o), lay in got.items():
        sfx = track.mode_suffix(c, o)
        if sfx:
            assert lay["eval"] == f"/r/output/eval_{sfx}" and lay["summary"] == f"/r/output/premvos_amd_davis_eval_{sfx}.json"
            assert lay["overlay"] == f"/r/output/overlay_{sfx}/"
        else:
            assert lay["eval"] == "/r/output/eval" and lay["summary"] == "/r/output/premvos_amd_davis_eval.json" and lay["overlay"] == "/r/output/overlay/"
    # --check-only names a missing annotation (and only with --oracle)
    root = str(tmp_path)
    for sub in ("data/DAVIS/JPEGImages/480p/v", "data/DAVIS/Annotations/480p/v", "output/intermediate/ReID_proposals/v", "output/intermediate/flow/v",
                "code/ReID_net/configs", "code/refinement_net/configs"):
        os.makedirs(os.path.join(root, sub))
    for net in ("ReID_net", "refinement_net"):
        open(os.path.join(root, "code", net, "configs", "live"), "w").write("{}")
    for t in range(3):
        Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(os.path.join(root, f"data/DAVIS/JPEGImages/480p/v/{t:05d}.jpg"))
    for t in (0, 2):
        R.write_index_png(os.path.join(root, f"data/DAVIS/Annotations/480p/v/{t:05d}.png"), np.zeros((8, 12), np.uint8))
    assert track.main(["--root", root, "--check-only"]) == 0
    assert track.main(["--root", root, "--combine", "probabilistic", "--check-only"]) == 0
    capsys.readouterr()
    assert track.main(["--root", root, "--oracle", "--check-only"]) == 2
    out = capsys.readouterr().out
    assert "Annotations/480p/v/00001.png is missing" in out and "00000.png" not in out and "00002.png" not in out
    assert track.main(["--root", root, "--oracle"]) == 2                                        # refused with the same message, nothing written
    assert "Annotations/480p/v/00001.png is missing" in capsys.readouterr().out and not os.path.exists(os.path.join(root, "output", "final_oracle"))
    assert track.missing_annotations([os.path.join(root, f"data/DAVIS/JPEGImages/480p/v/{t:05d}.jpg") for t in range(3)],
                                     os.path.join(root, "data/DAVIS/JPEGImages/480p") + "/", os.path.join(root, "data/DAVIS/Annotations/480p") + "/") == \
        [os.path.join(root, "data/DAVIS/Annotations/480p/v/00001.png")]
    R.write_index_png(os.path.join(root, "data/DAVIS/Annotations/480p/v/00001.png"), np.zeros((8, 12), np.uint8))
    assert track.main(["--root", root, "--oracle", "--check-only"]) == 0


def test_tracker_and_do_video_refuse_what_the_modes_do_not_run():
    from premvos_amd import _lib, track
    import inspect
    assert track.COMBINE_MODES == ("argmax", "probabilistic") and track.TEMPERATURE == 0.1
    sig = inspect.signature(track.Tracker.__init__).parameters
    assert sig["combine"].default == "argmax" and sig["oracle"].default is False
    for fn in (track.Tracker.step, track.Tracker.step_resident):
        assert inspect.signature(fn).parameters["gt"].default is None
    src = inspect.getsource(track.Tracker)
    assert src.count("self._score_select_paint(") == 2 and src.count("track_paint(") == 1 and src.count("track_scores(") == 1   # one shared helper
    assert "combine" not in inspect.signature(track.TrackerGroup.__init__).parameters             # lockstep is not touched
    with pytest.raises(_lib.PremvosError, match="resident"):
        track.do_video("/nonexistent/", "/a/", "/b/", "/c/", "/d/", "/e/", None, None, resident=False, combine="probabilistic")
    with pytest.raises(_lib.PremvosError, match="resident"):
        track.do_video("/nonexistent/", "/a/", "/b/", "/c/", "/d/", "/e/", None, None, resident=False, oracle=True)
