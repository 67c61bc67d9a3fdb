"""The host side of the ensemble vote (no GPU): the restatement (tests/ensemble_restated.py) on hand-written pixels, the weight-set
parser and the selection behind ``--ensemble-from``, every refusal of ``track --ensemble`` / ``--ensemble-from`` and of
``python -m premvos_amd.ensemble`` at argument time, the places of the mode's outputs, header / binding / document agreement of
premvos_idmap_vote_u8, its argument checks (before any HIP call) and ``ensemble --check-only`` on two tiny PNG trees."""
import os
import re

import numpy as np
import pytest

import ensemble_restated as E
import track_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "premvos_idmap_vote_u8", 8
SETS3 = "1,1,1,1,1;1,0,0,0,0;0,0,0,2,2"


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_the_restatement_on_hand_written_pixels():
    # pixels: a 2-2 split | three of four | unanimous | background ties object (the earlier set wins) | label 255 against a pair
    maps = np.array([[7, 1, 4, 0, 255],
                     [9, 2, 4, 3, 6],
                     [7, 2, 4, 0, 6],
                     [9, 2, 4, 3, 255]], np.uint8)
    voted, votes, hist = E.vote(maps)
    assert voted.tolist() == [7, 2, 4, 0, 255] and votes.tolist() == [2, 3, 4, 2, 2] and hist.tolist() == [0, 0, 3, 1, 1]
    voted, votes, hist = E.vote(maps[[1, 0, 3, 2]])                                             # the list order is the priority
    assert voted.tolist() == [9, 2, 4, 3, 6] and votes.tolist() == [2, 3, 4, 2, 2]
    voted, votes, hist = E.vote(np.array([[5, 0], [6, 1], [7, 2]], np.uint8))                   # all different at K = 3: set 0
    assert voted.tolist() == [5, 0] and votes.tolist() == [1, 1] and hist.tolist() == [0, 2, 0, 0]
    voted, votes, hist = E.vote(np.array([[0, 3], [3, 0]], np.uint8))                           # background ties object, both ways
    assert voted.tolist() == [0, 3] and votes.tolist() == [1, 1]
    one = np.array([[[0, 255], [17, 1]]], np.uint8)                                             # K = 1: the identity
    voted, votes, hist = E.vote(one)
    assert np.array_equal(voted, one[0]) and (votes == 1).all() and hist.tolist() == [0, 4]
    voted, votes, hist = E.vote(np.array([[1], [255], [255]], np.uint8))                        # label 255 outvotes set 0
    assert voted.tolist() == [255] and votes.tolist() == [2] and hist.tolist() == [0, 0, 1, 0]
    rng = np.random.default_rng(0)                                                              # and by brute force on random labels
    maps = rng.integers(0, 3, (5, 4, 6)).astype(np.uint8)
    voted, votes, hist = E.vote(maps)
    for y in range(4):
        for x in range(6):
            col = maps[:, y, x].tolist()
            counts = [col.count(v) for v in col]
            k = counts.index(max(counts))
            assert (voted[y, x], votes[y, x]) == (col[k], counts[k])
    assert hist.sum() == 24 and hist[0] == 0


# ------------------------------------------------------------------------------------------- the sets and the selection from a search
def test_the_sets_parser():
    from premvos_amd import track
    ws = track.parse_ensemble_sets(SETS3)
    assert ws.shape == (3, 5) and ws.dtype == np.float64
    assert ws.tolist() == [[0.2] * 5, [1.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.5, 0.5]]       # each row / its sum, in list order
    assert np.array_equal(track.parse_ensemble_sets("2,1,1,0,0;1,1,1,1,1")[0], np.array([2.0, 1, 1, 0, 0]) / 4.0)
    assert track.parse_ensemble_sets(";".join(["1,2,3,4,5"] * 8)).shape == (8, 5)
    for bad in ("1,1,1,1,1", ";".join(["1,1,1,1,1"] * 9), "1,1,1,1,1;1,1,1,1", "1,1,1,1,1;0,0,0,0,0", "1,1,1,1,1;1,1,1,1,-1",
                "1,1,1,1,1;a,b,c,d,e", "1,1,1,1,1;1,1,1,1,nan", "1,1,1,1,1;", ""):
        with pytest.raises(ValueError):
            track.parse_ensemble_sets(bad)


def test_the_selection_from_a_search_result():
    from premvos_amd import track
    ws = [[float(i + 1), 1.0, 1.0, 1.0, 1.0] for i in range(6)]
    res = {"weights": ws, "mean": [0.5, 0.9, None, 0.7, 0.9, 0.6], "seed": 0}
    assert track.DEFAULT_TOP == 3
    assert track.select_ensemble(res).tolist() == [ws[1], ws[4], ws[3]]                         # descending mean, the tie to the lower index
    assert track.select_ensemble(res, 2).tolist() == [ws[1], ws[4]]
    assert track.select_ensemble(res, 5).tolist() == [ws[1], ws[4], ws[3], ws[5], ws[0]]        # the null mean is ignored
    with pytest.raises(ValueError, match="only 5"):
        track.select_ensemble(res, 6)                                                           # five scored rows
    for top in (1, 0, 9, -1):
        with pytest.raises(ValueError, match="--top"):
            track.select_ensemble(res, top)
    with pytest.raises(ValueError, match="at least 2"):
        track.select_ensemble({"weights": ws[:3], "mean": [None, 0.4, float("nan")]}, 2)
    with pytest.raises(ValueError, match="at least 2"):
        track.select_ensemble({"weights": ws[:1], "mean": [0.4]}, 2)
    with pytest.raises(ValueError, match="not a search result"):
        track.select_ensemble({"videos": {}}, 2)
    with pytest.raises(ValueError):
        track.select_ensemble({"weights": ws[:3], "mean": [0.1, 0.2]}, 2)
    live = track.live_search_result({"a": {"scores": np.array([[0.5], [0.75], [0.75]]), "frames": 3}}, track.live_search_weights(3, 1), 1)
    assert np.array_equal(track.select_ensemble(live, 2), track.live_search_weights(3, 1)[[1, 2]])   # live_search.json's own content
    r = track.ensemble_result({"a": {"frames": 2, "hist": np.array([0, 1, 2, 5])}, "b": {"frames": 1, "hist": [0, 0, 0, 4]}}, 3, ws[:3], "--ensemble")
    assert r == {"videos": {"a": {"frames": 2, "hist": [0, 1, 2, 5], "unanimous": 5 / 8}, "b": {"frames": 1, "hist": [0, 0, 0, 4], "unanimous": 1.0}},
                 "frames": 3, "sets": 3, "weights": ws[:3], "source": "--ensemble"}
    import json
    json.dumps(r)


# ------------------------------------------------------------------------------------------------------------------ the refusals
def _refused(capsys, parse, argv, *words):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    err = " ".join(capsys.readouterr().err.split())
    assert e.value.code == 2 and all(w in err for w in words), (argv, err)


OLD_KEYS = {"root", "videos", "check_only", "eval", "overlay", "lockstep", "prewarp", "weights", "late_annotations", "prewarp_search", "seed",
            "search", "live_weights", "combine", "oracle", "viz", "max_reid_distance", "merge_weights", "live", "parser"}
NEW_KEYS = {"ensemble", "ensemble_from", "top", "ensemble_sets"}


def test_the_track_commands_refusals_and_namespace(capsys, tmp_path):
    from premvos_amd import track
    p = track.parse_args
    for flag in (["--ensemble", SETS3], ["--ensemble-from", "/nonexistent/live_search.json"]):
        for extra, word in ((["--search", "3"], "--search"), (["--prewarp-search", "3"], "--prewarp-search"), (["--live-weights", "1,1,1,1,1"], "--live-weights"),
                            (["--weights", "1,1,1,1,1"], "--weights"), (["--prewarp", "--weights", "1,1,1,1,1"], "--weights"), (["--oracle"], "--oracle"),
                            (["--combine", "probabilistic"], "--combine"), (["--viz"], "--viz"), (["--max-reid-distance"], "--max-reid-distance"),
                            (["--lockstep", "2"], "--lockstep above 1"), (["--late-annotations"], "--late-annotations without --prewarp")):
            _refused(capsys, p, flag + extra, f"argument {flag[0]}: not with", word)
    _refused(capsys, p, ["--ensemble", SETS3, "--ensemble-from", "x.json"], "argument --ensemble: not with --ensemble-from")
    for bad in ("1,1,1,1,1", ";".join(["1,1,1,1,1"] * 9), "1,1,1,1,1;1,1,1,1", "1,1,1,1,1;0,0,0,0,0", "1,1,1,1,1;1,1,1,1,-1", "1,1,1,1,1;a,b,c,d,e"):
        _refused(capsys, p, ["--ensemble", bad], "argument --ensemble: invalid value")
    for top in ("1", "9", "0"):
        _refused(capsys, p, ["--ensemble-from", "x.json", "--top", top], "argument --top: invalid choice")
    _refused(capsys, p, ["--top", "3"], "argument --top: only with --ensemble-from")
    _refused(capsys, p, ["--ensemble", SETS3, "--top", "3"], "argument --top: only with --ensemble-from")
    # accepted, and no file was looked at: the file of --ensemble-from does not exist
    a = p(["--ensemble", SETS3, "--eval", "--overlay"])
    assert a.ensemble_sets.tolist() == track.parse_ensemble_sets(SETS3).tolist() and a.ensemble == SETS3 and a.ensemble_from is None and a.top is None
    a = p(["--ensemble-from", "/nonexistent/live_search.json", "--top", "4", "--prewarp", "--late-annotations"])
    assert a.ensemble_sets is None and a.top == 4 and a.prewarp and a.late_annotations
    assert p(["--prewarp", "--ensemble", SETS3]).ensemble_sets.shape == (3, 5)
    _refused(capsys, track.main, ["--ensemble-from", str(tmp_path / "none.json")], "argument --ensemble-from", "none.json")     # main reads it
    (tmp_path / "few.json").write_text('{"weights": [[1,1,1,1,1],[1,0,0,0,0]], "mean": [0.5, null]}')
    _refused(capsys, track.main, ["--ensemble-from", str(tmp_path / "few.json"), "--top", "2"], "argument --ensemble-from", "at least 2")
    assert track.main(["--root", "/nonexistent", "--ensemble", SETS3, "--check-only"]) == 2       # accepted; the inputs are what is missing
    capsys.readouterr()
    # existing flags alone: the namespace they always gave, the new keys inert
    for argv, want in (([], {"root": ".", "videos": None, "check_only": False, "eval": False, "overlay": False, "lockstep": 1, "prewarp": False,
                             "weights": None, "late_annotations": False, "prewarp_search": 0, "seed": 0, "search": 0, "live_weights": None,
                             "combine": "argmax", "oracle": False, "viz": False, "max_reid_distance": False, "merge_weights": None, "live": None}),
                       (["--search", "9", "--seed", "4", "--videos", "a,b"], {"search": 9, "seed": 4, "videos": "a,b", "live": None}),
                       (["--prewarp", "--weights", "1,2,3,4,5", "--late-annotations", "--eval"],
                        {"prewarp": True, "merge_weights": [1.0, 2.0, 3.0, 4.0, 5.0], "late_annotations": True, "eval": True}),
                       (["--lockstep", "3", "--overlay"], {"lockstep": 3, "overlay": True}), (["--oracle", "--combine", "probabilistic", "--viz"],
                                                                                             {"oracle": True, "combine": "probabilistic", "viz": True})):
        a = vars(p(argv))
        assert set(a) == OLD_KEYS | NEW_KEYS, set(a) ^ (OLD_KEYS | NEW_KEYS)
        assert all(a[k] is None for k in NEW_KEYS) and all(a[k] == v for k, v in want.items()), (argv, a)
    assert p(["--live-weights", "2,1,1,0,0"]).live.tolist() == [0.5, 0.25, 0.25, 0.0, 0.0]
    _refused(capsys, p, ["--weights", "1,1,1,1,1"], "only with --prewarp")                       # an old refusal, word for word
    _refused(capsys, p, ["--search", "3", "--max-reid-distance"], "argument --max-reid-distance: not with a merge flag")
    with pytest.raises(SystemExit):
        p(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--ensemble a,b,c,d,e;a,b,c,d,e;...", "--ensemble-from FILE", "--top K", "output/final_ensemble/", "output/ensemble.json",
                 "oldmerge.py:129-131,220-224", "output/final_prewarp_ensemble/", "listed FIRST"):
        assert word in text, word


def test_the_tree_tools_refusals(capsys):
    from premvos_amd import ensemble
    p = ensemble.parse_args
    _refused(capsys, p, ["--root", "r"], "--inputs")
    _refused(capsys, p, ["--inputs", "final"], "argument --inputs: 1 trees")
    _refused(capsys, p, ["--inputs", ",".join(f"t{i}" for i in range(9))], "argument --inputs: 9 trees")
    _refused(capsys, p, ["--inputs", "final,final"], "listed twice")
    _refused(capsys, p, ["--inputs", "final,final_prob", "--out", "final_prob"], "argument --out", "is an input")
    _refused(capsys, p, ["--inputs", "final_prewarp,final_prob", "--out", "final"], "argument --out: not final")
    _refused(capsys, p, ["--inputs", "final,../x"], "invalid value")
    _refused(capsys, p, ["--inputs", "final,"], "invalid value")
    a = p(["--inputs", "final,final_prewarp,final_prob"])
    assert a.names == ["final", "final_prewarp", "final_prob"] and a.out == "final_vote" and not (a.eval or a.overlay or a.check_only)


# --------------------------------------------------------------------------------------------------------------------- the places
def test_the_mode_never_writes_the_live_loops_places():
    from premvos_amd import track
    assert track.mode_suffix() == "" and track.mode_suffix("argmax", False, False) == ""
    assert track.mode_suffix("probabilistic", True) == "oracle_prob" and track.mode_suffix(live_weights=True) == "weights"
    assert track.mode_suffix(ensemble=True) == "ensemble"
    plain = track.mode_layout("/r")
    assert plain == track.mode_layout("/r", "argmax", False, False) == track.mode_layout("/r", ensemble=False)
    assert plain["out"] == "/r/output/final/" and plain["eval"] == "/r/output/eval" and plain["overlay"] == "/r/output/overlay/"
    assert plain["summary"] == "/r/output/premvos_amd_davis_eval.json"
    assert track.mode_layout("/r", live_weights=True)["out"] == "/r/output/final_weights/"
    lay = track.mode_layout("/r", ensemble=True)
    assert lay["out"] == "/r/output/final_ensemble/" and lay["eval"] == "/r/output/eval_ensemble" and lay["overlay"] == "/r/output/overlay_ensemble/"
    assert lay["summary"] == "/r/output/premvos_amd_davis_eval_ensemble.json"
    for k in ("images", "anns", "props", "flows"):
        assert lay[k] == plain[k]


# ----------------------------------------------------------------------------------------------------- header, binding, documents
def test_header_signature_and_documents_name_the_entry():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    assert NAME in declared and len(_lib.SIGNATURES[NAME]) == NARGS and _lib.ABI_VERSION == 21
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", hdr).group(1)
    assert decl.count(",") + 1 == NARGS
    assert "oldmerge.py:129-131,220-224" in hdr
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "ensemble_ops.hip")).read()
    assert f'extern "C" int {NAME}(' in src
    for bounds in re.findall(r"__launch_bounds__\((\w+)\)", src):
        n = int(bounds) if bounds.isdigit() else int(re.search(r"constexpr int %s = (\d+);" % bounds, src).group(1))
        assert n % 64 == 0, bounds
    assert "__launch_bounds__" in src and not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", src))      # integer work only
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8.9" in design and "--ensemble" in open(os.path.join(ROOT, "README.md")).read()


def test_library_built_for_gfx950_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21 and hasattr(lib, NAME)
    buf = np.zeros(4096, np.uint8)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused

    def vote(maps=one, K=3, stride=64, pixels=64, voted=one + 1024, votes=one + 2048, hist=one + 3072):
        return lib.premvos_idmap_vote_u8(maps, K, stride, pixels, voted, votes, hist, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, lib.premvos_last_error())

    refused(vote(maps=None), b"null")
    refused(vote(voted=None), b"null")
    refused(vote(K=0), b"1 to 8 sets")
    refused(vote(K=9), b"1 to 8 sets")
    refused(vote(pixels=-1), b"negative")
    refused(vote(stride=63), b"overlap")                                                        # set_stride < pixels with K > 1
    refused(vote(voted=one + 100), b"voted overlaps the maps")                                  # inside set 1
    refused(vote(voted=one + 3 * 64 - 1), b"voted overlaps the maps")                           # the last byte of set 2
    refused(vote(votes=one + 10), b"votes overlaps the maps")
    refused(vote(votes=one + 1024 + 63), b"votes overlaps voted")
    refused(vote(stride=500, voted=one + 1000 + 63), b"voted overlaps the maps")                # (the span is (K - 1) stride + pixels)
    assert vote(pixels=0) == 0 and vote(pixels=0, stride=0, votes=None, hist=None) == 0         # nothing to do: no launch
    assert vote(K=1, pixels=0, stride=-5) == 0                                                  # one set has no stride


# --------------------------------------------------------------------------------------------------------- the tree tool's check
def _png_tree(root, name, videos, edit=None):
    for video, (n, h, w) in videos.items():
        os.makedirs(os.path.join(root, "output", name, video))
        for t in range(n):
            a = np.zeros((h, w), np.uint8)
            a[1:3, 1 + t:4 + t] = 1 + t
            if edit is not None:
                edit(video, t, a)
            R.write_index_png(os.path.join(root, "output", name, video, f"{t:05d}.png"), a)


def test_check_only_names_what_differs(tmp_path, capsys):
    from premvos_amd import ensemble
    root = str(tmp_path)
    videos = {"a": (3, 6, 9), "b": (2, 5, 7)}
    _png_tree(root, "one", videos)
    _png_tree(root, "two", videos, edit=lambda v, t, a: a.__setitem__((0, 0), 9))
    assert ensemble.check_trees(root, ["one", "two"], ["a", "b"]) == []
    assert ensemble.tree_videos(root, ["one", "two"]) == ["a", "b"] and ensemble.tree_videos(root, ["one", "two"], "b,c") == ["b"]
    assert ensemble.main(["--root", root, "--inputs", "one,two", "--check-only"]) == 0
    assert "agree" in capsys.readouterr().out
    os.remove(os.path.join(root, "output", "two", "a", "00001.png"))                           # a frame is missing in one input
    assert ensemble.main(["--root", root, "--inputs", "one,two", "--check-only"]) == 2
    text = capsys.readouterr().out
    assert "a/00001.png: missing in two" in text and "b/" not in text
    R.write_index_png(os.path.join(root, "output", "two", "b", "00000.png"), np.zeros((5, 8), np.uint8))      # a size differs
    os.makedirs(os.path.join(root, "output", "one", "c"))                                       # a video only one input has (and empty)
    R.write_index_png(os.path.join(root, "output", "one", "c", "00000.png"), np.zeros((4, 4), np.uint8))
    problems = ensemble.check_trees(root, ["one", "two"], ensemble.tree_videos(root, ["one", "two"]))
    assert any("a/00001.png: missing in two" in p for p in problems) and any("b/00000.png: sizes differ" in p and "(5, 8)" in p for p in problems)
    assert any(p.startswith("c: no PNGs under") and "two" in p for p in problems) and len(problems) == 3
    assert ensemble.main(["--root", root, "--inputs", "one,three", "--check-only"]) == 2
    assert "three is missing" in capsys.readouterr().out
