"""The host side of the score sheets and of the ReID distance calibration (no GPU): the numpy restatement (tests/viz_restated.py)
against the reference executed (tests/golden/viz_ref.npz, tools/make_golden_viz.py); header / binding / document agreement of the two
entries of csrc/viz_ops.hip; their argument checks (before any HIP call, so they run here); the command line.

Bounds.  The float canvas: EXACT -- every value is one float64 multiply of the same operands (or a uint8), nothing is summed.  The
distances: 1e-12 relative, the project's bound for the same quantity summed in BLAS's order (planes 1 and 2): the program's
``norm`` is BLAS's dot, the restatement's kernel order adds the 128 squares one by one."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ENTRIES = (("premvos_viz_scores_u8", 16), ("premvos_reid_max_distance_f64", 7))
CASES = ("t1p4", "t3p6", "dark")
TINT = np.array([0, 128, 0], np.uint8)


def _args(a, tag):
    return [a[f"{tag}_{k}"] for k in ("frame", "masks", "boxes", "planes", "weighted", "gt")]


@pytest.mark.parametrize("tag", CASES)
def test_the_restatement_reproduces_the_reference(tag):
    import viz_restated as V
    from premvos_amd import track
    a = V.load_fixture()
    assert a["tint_row"].tolist() == track.voc_palette()[2].tolist()            # the generator's palette stand-in: row 2
    canvas = V.float_sheet(*_args(a, tag), a["tint_row"][::-1])
    assert canvas.dtype == np.float64 and canvas.shape == a[f"{tag}_canvas"].shape and np.array_equal(canvas, a[f"{tag}_canvas"])
    u8 = V.sheet_u8(*_args(a, tag), TINT)
    assert u8.dtype == np.uint8 and np.array_equal(u8, V.bytescale(a[f"{tag}_canvas"]))
    T, P = a[f"{tag}_gt"].shape
    assert u8.shape == (100 * (T + 1), 100 * P, 3) and not u8[:, ::100].any() and not u8[100::100].any()       # the separators
    hi_w, hi_g = V.marks_of(a[f"{tag}_weighted"], a[f"{tag}_gt"])
    for i in range(T):
        for j in range(P):
            cell_w, cell_g = u8[100 * (i + 1) + 12:100 * (i + 1) + 37, 100 * j + 62:100 * j + 87], u8[100 * (i + 1) + 62:100 * (i + 1) + 87, 100 * j + 62:100 * j + 87]
            assert (not cell_w.any()) == (j == hi_w[i]) and (not cell_g.any()) == (j == hi_g[i]), (i, j)


def test_the_fixture_holds_the_crafted_cases():
    import viz_restated as V
    a = V.load_fixture()
    assert list(a["cases"]) == list(CASES) and all(v.dtype != object for v in a.values())                         # data only
    assert os.path.getsize(V.GOLDEN) < 512 * 1000
    assert a["t1p4_gt"].shape == (1, 4) and (a["t1p4_planes"][2] == 1).all() and (a["t1p4_planes"][4] == 1).all()   # T = 1: the "other" planes
    assert a["t3p6_gt"].shape == (3, 6) and a["t1p4_frame"].shape == (40, 56, 3)
    b = a["t1p4_boxes"]
    assert int(b[1, 2]) < 2 and not a["t1p4_canvas"][:100, 100:200].any()                                         # min(h, w) < 2: black
    assert b[2, 2:].tolist() == [2.0, 2.0] and len(np.unique(a["t1p4_canvas"][:100, 201:300].reshape(-1, 3), axis=0)) == 1   # a 1 x 1 crop
    b = a["t3p6_boxes"]
    assert b[1, 0] + b[1, 2] == 56 and b[1, 1] + b[1, 3] == 40                                                   # touches the right and bottom edge
    assert not a["t3p6_masks"][4].any()                                                                           # an all-zero mask: no tint
    assert a["t1p4_canvas"].max() == 255 and a["t3p6_canvas"].max() == 255 and 100 < a["dark_canvas"].max() < 255
    for k in ("planes", "weighted", "gt"):
        assert ((a[f"dark_{k}"] > 0) & (a[f"dark_{k}"] < 1)).all()
    u8 = V.bytescale(a["dark_canvas"])
    assert u8.max() == 255 and not np.array_equal(u8, (a["dark_canvas"] + 0.5).astype(np.uint8))                  # the factor is not 1
    ws = a["t3p6_weighted"]
    assert ws[1, 2] == ws[1, 4] == ws[1].max() and V.marks_of(ws, a["t3p6_gt"])[0][1] == 2                       # a tie: the first maximum
    assert not a["t3p6_gt"][2].any() and V.marks_of(ws, a["t3p6_gt"])[1][2] == 0
    # part 2: a proposal without 'ReID', a frame without a proposal file, an annotation on a later frame
    assert np.isinf(a["mrd_alpha_props"]).all(axis=1).sum() == 1 and 0 in a["mrd_alpha_counts"].tolist()
    assert a["mrd_alpha_templates"].shape == (3, 128) and a["mrd_beta_templates"].shape == (2, 128)
    assert a["mrd_dataset_max"] == max(a["mrd_alpha_max"].max(), a["mrd_beta_max"].max()) and a["mrd_dataset_max"] > 25 > a["mrd_alpha_max"].min()


def test_bytescale_and_our_rules():
    import viz_restated as V
    x = np.array([[-10.0, 0.0, 245.0], [117.5, 117.4, np.nan]])
    assert V.bytescale(x).tolist() == [[0, 10, 255], [128, 127, 0]]              # scale 1, + 0.5 and truncation; NaN -> 0, not in the extremes
    assert V.bytescale(np.full((2, 2), 7.0)).tolist() == [[0, 0], [0, 0]]        # a zero range counts as 1
    assert V.bytescale(np.array([0.0, 51.0, 102.0])).tolist() == [0, 128, 255]   # 127.5 + 0.5 -> 128
    frame = np.full((20, 30, 3), 200, np.uint8)
    mask = np.ones((20, 30), np.uint8)
    assert not V.tile_of(frame, mask, [40.0, 2.0, 9.0, 9.0], TINT).any()         # empty after clipping: black (cv2.resize would raise)
    assert not V.tile_of(frame, mask, [np.nan, 2.0, 9.0, 9.0], TINT).any()
    assert not V.tile_of(frame, mask, [3.0, 2.0, 1.9, 9.0], TINT).any()          # int(1.9) = 1 < 2
    t = V.tile_of(frame, mask, [25.0, 15.0, 50.0, 50.0], TINT)                   # clipped like a numpy slice
    assert t.shape == (100, 100, 3) and (t == np.array([140, 178, 140])).all()   # (uint8)(200 * 0.7 + (0, 128, 0) * 0.3)
    assert (V.tile_of(frame, mask * 0, [2.0, 2.0, 9.0, 9.0], TINT) == 200).all()
    planes = np.full((5, 1, 2), 0.5)
    planes[1, 0, 1] = np.nan
    ws = np.array([[np.nan, -np.inf]])
    c = V.float_sheet(frame, [mask, mask], [[0, 0, 9, 9]] * 2, planes, ws, np.array([[0.25, np.inf]]), TINT)
    assert (c[101:150, 51:100] == [255.0, 0.0, 0.0])[36:, :].all()               # non-finite weighted = 0: red (below the mark: first maximum 0)
    assert np.isnan(c[121:140, 101:150, :2]).all() and not np.isfinite(c[151:, 151:, :2]).any() and not c[121:140, 101:, 2].any()
    u8 = V.bytescale(c)
    assert not u8[121:140, 101:150].any() and not u8[151:, 151:].any() and u8.max() == 255
    assert V.marks_of(ws, np.array([[0.25, np.inf]])) == (0, 0)


def test_the_restated_distances_reproduce_the_program():
    import viz_restated as V
    a = V.load_fixture()
    best = []
    for v in a["mrd_videos"]:
        counts, pooled, templ = a[f"mrd_{v}_counts"], a[f"mrd_{v}_props"], a[f"mrd_{v}_templates"]
        o = np.concatenate([[0], np.cumsum(counts)])
        frames = [pooled[o[i]:o[i + 1]] for i in range(len(counts))]
        gold = a[f"mrd_{v}_max"]
        prog = V.max_distances_program(templ, frames)
        ordered, over = V.max_distances_ordered(templ, pooled)
        assert np.abs(prog - gold).max() <= 1e-12 * np.abs(gold).max() and np.abs(ordered - gold).max() <= 1e-12 * np.abs(gold).max()
        assert over.shape == (len(templ),) and int(over.sum()) == int((np.array([[np.linalg.norm(c - t) for c in pooled[np.isfinite(pooled).all(1)]] for t in templ]) > 25).sum())
        best.append(ordered.max())
    assert abs(max(best) - a["mrd_dataset_max"]) <= 1e-12 * a["mrd_dataset_max"]
    z, n = V.max_distances_ordered(np.ones((2, 128)), np.zeros((0, 128)))
    assert z.tolist() == [0.0, 0.0] and n.tolist() == [0, 0]
    z, n = V.max_distances_ordered(np.zeros((1, 128)), np.full((3, 128), np.inf))
    assert z.tolist() == [0.0] and n.tolist() == [0]                             # an infinite distance counts as 0


def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    path = os.path.join(ROOT, "premvos_amd", "csrc", "viz_ops.hip")
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
    for cite in ("merge_functions.py:547-611", "print_max_reid_distance.py"):
        assert cite in hdr, cite
    assert src.startswith("// hipcc-flags: -ffp-contract=off\n") and "-ffp-contract=off" in build._file_flags(path)
    assert "#if" not in src
    assert not re.search(r"\batomic[A-Z]|unsafeAtomic|__hip_atomic", src)                        # no atomics at all: slots and ordered folds
    assert '#include "resize_cv.h"' in src and "premvos::cv_lin_coef(" in src                   # cv2's rule is shared, not copied
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 8.7" in design and "unpinned" in design[design.index("### 8.7"):]


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.float64)
    one = buf.ctypes.data                                                                       # never dereferenced by the device: every call is refused

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    def sheet(frame=one, h=5, w=7, masks=one, boxes=one, P=3, planes=one, weighted=one, stride=4, gt=one, T=2, tint=one, work=one, nwork=4096,
              out=one):
        return lib.premvos_viz_scores_u8(frame, h, w, masks, boxes, P, planes, weighted, stride, gt, T, tint, work, nwork, out, None)

    def dist(templ=one, T=2, props=one, N=3, out=one, over=one):
        return lib.premvos_reid_max_distance_f64(templ, T, props, N, out, over, None)

    for kw in ("frame", "masks", "boxes", "planes", "weighted", "gt", "tint", "work", "out"):
        refused(sheet(**{kw: None}), b"null")
    for kw in ({"h": 0}, {"w": -1}, {"h": 1 << 16, "w": 1 << 15}):
        refused(sheet(**kw), b"bad dims")
    for kw in ({"T": 0}, {"T": 256}, {"T": -1}):
        refused(sheet(**kw), b"255")
    refused(sheet(P=0), b"at least one candidate")
    refused(sheet(P=656, stride=656), b"65535")
    refused(sheet(P=400, stride=400, T=200, nwork=1 << 20), b"64 Mi")
    refused(sheet(stride=2), b"stride")
    refused(sheet(nwork=16 * 4 + 8 * 2 - 1), b"workspace")
    refused(sheet(work=one + 4), b"workspace")
    for kw in ("templ", "out"):
        refused(dist(**{kw: None}), b"null")
    refused(dist(props=None), b"null")
    for kw in ({"T": 0}, {"N": -1}, {"T": 65536}, {"N": 1 << 31}):
        refused(dist(**kw), b"bad dims")


def test_command_line(tmp_path, capsys):
    from PIL import Image
    from premvos_amd import track
    import track_restated as R
    for argv, word in ((["--viz", "--lockstep", "2"], "not with --lockstep above 1"), (["--viz", "--prewarp"], "not with --prewarp"),
                       (["--viz", "--prewarp-search", "3"], "not with --prewarp"), (["--max-reid-distance", "--viz"], "not with a merge flag"),
                       (["--max-reid-distance", "--oracle"], "not with a merge flag"), (["--max-reid-distance", "--combine", "probabilistic"], "not with a merge flag"),
                       (["--max-reid-distance", "--prewarp"], "not with a merge flag"), (["--max-reid-distance", "--prewarp-search", "2"], "not with a merge flag"),
                       (["--max-reid-distance", "--lockstep", "2"], "not with a merge flag"), (["--max-reid-distance", "--eval"], "not with a merge flag"),
                       (["--max-reid-distance", "--overlay"], "not with a merge flag"), (["--max-reid-distance", "--weights", "1,1,1,1,1"], "not with a merge flag"),
                       (["--max-reid-distance", "--late-annotations"], "not with a merge flag"),
                       (["--viz", "--oracle", "--lockstep", "2"], "argument --combine / --oracle: not with --lockstep above 1")):      # an existing refusal, word for word
        with pytest.raises(SystemExit) as e:
            track.main(["--root", "/nonexistent"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert track.main(["--root", "/nonexistent", "--viz", "--combine", "probabilistic", "--oracle", "--eval", "--overlay", "--check-only"]) == 2
    assert track.main(["--root", "/nonexistent", "--max-reid-distance", "--check-only"]) == 2
    capsys.readouterr()
    with pytest.raises(SystemExit):
        track.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--viz", "--max-reid-distance", "merge_functions.py:547-611", "print_max_reid_distance.py", "output/viz/<video>/<frame>.jpg",
                 "output/max_reid_distance.json"):
        assert word in text, word
    got = {(c, o): track.mode_layout("/r", c, o)["viz"] for c in track.COMBINE_MODES for o in (False, True)}
    assert [got[k] for k in (("argmax", False), ("probabilistic", False), ("argmax", True), ("probabilistic", True))] == \
        ["/r/output/viz/", "/r/output/viz_prob/", "/r/output/viz_oracle/", "/r/output/viz_oracle_prob/"]
    assert "viz" not in track._layout("/r")
    # --check-only names a missing annotation, in --oracle's wording; a run without one returns 2 and writes nothing
    root = str(tmp_path)
    for sub in ("data/DAVIS/JPEGImages/480p/v", "data/DAVIS/Annotations/480p/v", "output/intermediate/ReID_proposals/v", "code/ReID_net/configs"):
        os.makedirs(os.path.join(root, sub))
    open(os.path.join(root, "code", "ReID_net", "configs", "live"), "w").write("{}")
    for t in range(3):
        Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(os.path.join(root, f"data/DAVIS/JPEGImages/480p/v/{t:05d}.jpg"))
    for t in (0, 2):
        R.write_index_png(os.path.join(root, f"data/DAVIS/Annotations/480p/v/{t:05d}.png"), np.zeros((8, 12), np.uint8))
    assert track.main(["--root", root, "--max-reid-distance", "--check-only"]) == 0              # neither the flow nor the refinement net
    assert track.main(["--root", root, "--check-only"]) == 2
    os.makedirs(os.path.join(root, "output/intermediate/flow/v"))
    os.makedirs(os.path.join(root, "code/refinement_net/configs"))
    open(os.path.join(root, "code", "refinement_net", "configs", "live"), "w").write("{}")
    assert track.main(["--root", root, "--check-only"]) == 0
    capsys.readouterr()
    assert track.main(["--root", root, "--viz", "--check-only"]) == 2
    out = capsys.readouterr().out
    assert "Annotations/480p/v/00001.png is missing (--viz scores every frame of v against its annotation)" in out
    assert "00000.png" not in out and "00002.png" not in out
    assert track.main(["--root", root, "--viz"]) == 2
    assert "Annotations/480p/v/00001.png is missing" in capsys.readouterr().out
    assert sorted(os.listdir(os.path.join(root, "output"))) == ["intermediate"]
    assert track.main(["--root", root, "--viz", "--oracle", "--check-only"]) == 2
    assert "(--oracle scores every frame of v against its annotation)" in capsys.readouterr().out
    R.write_index_png(os.path.join(root, "data/DAVIS/Annotations/480p/v/00001.png"), np.zeros((8, 12), np.uint8))
    assert track.main(["--root", root, "--viz", "--check-only"]) == 0


def test_the_python_layer_is_additive():
    from premvos_amd import track, viz
    sig = inspect.signature(track.Tracker.__init__).parameters
    assert sig["viz"].default is False and list(sig)[-1] == "viz"
    assert inspect.signature(track.do_video).parameters["viz_dir"].default is None and list(inspect.signature(track.do_video).parameters)[-1] == "viz_dir"
    assert inspect.signature(track.Tracker.step).parameters["frame"].default is None
    src = inspect.getsource(track.Tracker)
    assert src.count("self._score_select_paint(") == 2 and src.count("track_paint(") == 1 and src.count("track_scores(") == 1
    assert 'self._tick("sheet")' in src and "viz" not in inspect.getsource(track.TrackerGroup)
    assert list(inspect.signature(viz.sheet).parameters) == ["frame", "masks", "boxes", "planes", "weighted", "gt", "tint"]
    assert list(inspect.signature(viz.viz_scores).parameters)[:7] == ["all_scores", "weighted_scores", "proposals", "image_fn", "input_images",
                                                                      "gt_scores", "out_dir"]
    assert (viz.QUALITY, viz.SUBSAMPLING, viz.BOX, viz.COMPILED_IN) == (75, "4:2:0", 100, 25) and track.MAX_REID_DISTANCE == 25
    assert viz.default_tint().tolist() == [0, 128, 0] and viz.workspace_bytes(3, 8) == 16 * 9 + 24
    assert "premvos_amd.viz" not in open(os.path.join(ROOT, "premvos_amd", "stream.py")).read()
