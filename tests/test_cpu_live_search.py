"""The host side of ``track --search`` / ``--live-weights`` (no GPU): header / binding / document agreement of the two new entries and
their argument checks (before any HIP call), the command's refusals by ``parse_args``, the rounds, the JSON content, the places of the
``--live-weights`` outputs, and the restatement (tests/live_search_restated.py) against ``track_restated.do_video`` on the golden track
fixture.  Non-vacuity of the GPU kernel test is shown here: on its inputs the three hand-made weight sets do not select alike."""
import os
import re

import numpy as np
import pytest

import live_search_restated as L
import track_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("premvos_track_scores_sets_f64", 18), ("premvos_track_eval_seats_i64", 11))


def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.premvos_abi_version() == 21                           # additive: the version stays
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "track_ops.hip")).read()
    for name, nargs in ENTRIES:
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert decl.count(",") + 1 == nargs, name
        assert f'extern "C" int {name}(' in src
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for cite in ("oldmerge.py:225-227,253-255", "merge_functions.py:613-634", "merge.py:119"):
        assert cite in hdr
    assert src.startswith("// hipcc-flags: -ffp-contract=off\n")
    assert "8.8" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.int64)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused
    weights = np.ones((8, 5), np.float64)
    good = np.ascontiguousarray(np.array([(2, 3, 0, 6), (0, 9, 0, 0), (2, 3, 2, 6)], np.int32))
    first = np.array([0, 2, 4, 0, 0, 0, 0, 0], np.int32)

    def scores(seats=good, V=3, inter=one, fresh=one, w=weights.ctypes.data):
        return lib.premvos_track_scores_sets_f64(inter, one, one, one, one, one, fresh, fresh, None if seats is None else seats.ctypes.data, V, w,
                                                 1e-10, one, one, one, one, one, None)

    def evals(planes=one, R_=6, h=4, w=4, gt=one, V=3, T0=2, fp=first.ctypes.data, counts=one, stride=6):
        return lib.premvos_track_eval_seats_i64(planes, R_, h, w, gt, V, T0, fp, counts, stride, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, lib.premvos_last_error())

    refused(scores(inter=None), b"null")
    refused(scores(w=None), b"null")
    refused(scores(seats=None), b"null")
    refused(scores(fresh=None), b"null")                                                        # the seats have fresh rows
    refused(scores(V=0), b"seats")
    refused(scores(V=9), b"seats")
    uneven = np.ascontiguousarray(np.array([(2, 3, 0, 6), (2, 4, 2, 6)], np.int32))
    refused(scores(seats=uneven, V=2), b"share one block")                                      # every occupied seat carries the same F
    refused(scores(seats=np.array([(256, 0, 0, 0)], np.int32), V=1), b"255")
    refused(scores(seats=np.array([(1, -1, 0, 0)], np.int32), V=1), b"negative")
    empty = np.ascontiguousarray(np.array([(0, 7, -3, 99), (0, 0, 0, 0)], np.int32))
    assert scores(seats=empty, V=2, fresh=None) == 0                                            # nothing to do, nothing launched
    refused(evals(planes=None), b"null")
    refused(evals(gt=None), b"null")
    refused(evals(fp=None), b"null")
    refused(evals(counts=None), b"null")
    refused(evals(V=0), b"seats")
    refused(evals(V=9), b"seats")
    refused(evals(h=0), b"bad dims")
    refused(evals(T0=256), b"255")
    refused(evals(R_=5), b"outside")                                                            # seat 2: planes 4, 5 of 5
    refused(evals(stride=5), b"overlap")                                                        # 2 objects need 6 counts per seat
    late = np.array([0, -1, 0, 0, 0, 0, 0, 0], np.int32)
    refused(evals(fp=late.ctypes.data), b"outside")
    assert evals(T0=0, stride=0) == 0                                                           # no object: nothing launched


def _refused(capsys, argv, *words):
    from premvos_amd import track
    with pytest.raises(SystemExit) as e:
        track.parse_args(argv)
    err = " ".join(capsys.readouterr().err.split())
    assert e.value.code == 2 and all(w in err for w in words), (argv, err)


def test_the_commands_refusals_and_help(capsys):
    from premvos_amd import track
    for extra in (["--prewarp"], ["--prewarp-search", "2"], ["--lockstep", "2"], ["--combine", "probabilistic"], ["--oracle"], ["--viz"],
                  ["--eval"], ["--overlay"], ["--weights", "1,1,1,1,1"], ["--late-annotations"], ["--live-weights", "1,1,1,1,1"]):
        _refused(capsys, ["--search", "3"] + extra, "argument --search: not with", extra[0])
    _refused(capsys, ["--search", "3", "--max-reid-distance"], "argument --max-reid-distance", "--search")
    _refused(capsys, ["--live-weights", "1,1,1,1,1", "--max-reid-distance"], "argument --max-reid-distance", "--live-weights")
    _refused(capsys, ["--search", "-1"], "argument --search: invalid choice")
    _refused(capsys, ["--search", "two"], "argument --search")
    # --weights alone is still the pre-warp merge's flag
    _refused(capsys, ["--weights", "1,1,1,1,1"], "only with --prewarp")
    for extra in (["--prewarp"], ["--prewarp-search", "2"], ["--combine", "probabilistic"], ["--oracle"]):
        _refused(capsys, ["--live-weights", "1,1,1,1,1"] + extra, "argument --live-weights: not with", extra[0])
    for bad in ("1,1,1,1", "0,0,0,0,0", "1,1,1,1,-1", "a,b,c,d,e", "1,1,1,1,nan"):
        _refused(capsys, ["--live-weights", bad], "argument --live-weights: invalid value")
    a = track.parse_args(["--search", "9", "--seed", "4", "--videos", "a,b"])
    assert a.search == 9 and a.seed == 4 and a.live is None and a.merge_weights is None
    a = track.parse_args(["--live-weights", "2,1,1,0,0", "--lockstep", "3", "--eval", "--overlay"])
    assert a.live.tolist() == [0.5, 0.25, 0.25, 0.0, 0.0] and a.lockstep == 3 and a.search == 0
    assert track.parse_args(["--live-weights", "1,1,1,1,1", "--viz"]).viz
    assert track.parse_args(["--prewarp", "--weights", "1,2,3,4,5"]).merge_weights == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert track.main(["--root", "/nonexistent", "--search", "3", "--check-only"]) == 2          # accepted; the inputs are what is missing
    capsys.readouterr()
    with pytest.raises(SystemExit):
        track.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--search W", "--live-weights a,b,c,d,e", "output/live_search.json", "output/final_weights/", "oldmerge.py:225-227,253-255",
                 "merge_functions.py:613-634", "not the bytes of --live-weights"):
        assert word in text, word


def test_rounds_and_weight_sets():
    from premvos_amd import prewarp, track
    assert track.MAX_SEATS == 8
    assert track.plan_search_rounds(1) == [(0, 1)] and track.plan_search_rounds(8) == [(0, 8)]
    assert track.plan_search_rounds(9) == [(0, 8), (8, 9)] and track.plan_search_rounds(17) == [(0, 8), (8, 16), (16, 17)]
    assert track.plan_search_rounds(0) == []
    for W in (1, 8, 9, 17):                                                                     # every set once, in order, <= 8 per round
        r = track.plan_search_rounds(W)
        assert [i for a, b in r for i in range(a, b)] == list(range(W)) and all(0 < b - a <= 8 for a, b in r)
    ws = track.live_search_weights(9, seed=4)
    assert ws.shape == (9, 5) and np.array_equal(ws[0], track.NORMALISED_WEIGHTS) and np.array_equal(ws[0], R.NORMALISED_WEIGHTS)
    assert np.array_equal(ws[1:], prewarp.search_weights(9, 4)[1:]) and np.allclose(ws.sum(axis=1), 1)
    assert np.array_equal(track.live_search_weights(3, 4), ws[:3]) and not np.array_equal(track.live_search_weights(3, 5)[1:], ws[1:3])
    assert track.search_skip_reason([], [(4, 4)], 40).startswith("no templates")
    assert "max_boxes" in track.search_skip_reason([{}] * 41, [(4, 4)], 40)
    assert "differ in size" in track.search_skip_reason([{}], [(4, 4), (4, 6)], 40)
    assert track.search_skip_reason([{}] * 40, [(4, 4)] * 3, 40) is None


def test_the_json_content():
    import json
    from premvos_amd import track
    ws = track.live_search_weights(3, 1)
    per = {"a": {"scores": np.array([[0.5, 0.7], [0.9, 0.5], [0.6, 0.8]]), "frames": 4, "counts": None},
           "b": {"skipped": "no templates (frame 00000 has no annotated object)"},
           "c": {"scores": np.array([[0.3], [0.4], [0.7]]), "frames": 5, "counts": None}}
    r = track.live_search_result(per, ws, 1)
    assert set(r) == {"videos", "weights", "seed", "mean", "frames", "best", "skipped"}
    assert set(r) >= {"videos", "weights", "seed", "mean", "frames"}                            # prewarp_search.json's keys
    assert r["videos"] == {"a": {"scores": [[0.5, 0.7], [0.9, 0.5], [0.6, 0.8]]}, "c": {"scores": [[0.3], [0.4], [0.7]]}}
    assert r["frames"] == 9 and r["seed"] == 1 and r["weights"] == ws.tolist() and r["skipped"] == {"b": per["b"]["skipped"]}
    assert r["mean"] == [float(np.mean([0.5, 0.7, 0.3])), float(np.mean([0.9, 0.5, 0.4])), float(np.mean([0.6, 0.8, 0.7]))] and r["best"] == 2
    json.dumps(r)
    tie = {"a": {"scores": np.array([[0.5], [0.75], [0.75]]), "frames": 3}}
    assert track.live_search_result(tie, ws, 0)["best"] == 1                                    # the lowest index on a tie
    nothing = track.live_search_result({"b": per["b"]}, ws, 0)
    assert nothing["best"] is None and nothing["mean"] == [None] * 3 and nothing["videos"] == {} and nothing["frames"] == 0


def test_live_weights_never_write_the_live_loops_places():
    from premvos_amd import track
    lay = track.mode_layout("/r", live_weights=True)
    assert track.mode_suffix(live_weights=True) == "weights"
    assert lay["out"] == "/r/output/final_weights/" and lay["overlay"] == "/r/output/overlay_weights/" and lay["viz"] == "/r/output/viz_weights/"
    assert lay["eval"] == "/r/output/eval_weights" and lay["summary"] == "/r/output/premvos_amd_davis_eval_weights.json"
    plain = track.mode_layout("/r")
    for k in ("out", "overlay", "viz", "eval", "summary"):
        assert lay[k] != plain[k] and "output/final/" not in lay[k], k
    assert plain == track.mode_layout("/r", "argmax", False, False) and plain["out"] == "/r/output/final/"
    for k in ("images", "anns", "props", "flows"):
        assert lay[k] == plain[k]


def test_the_restatement_with_set_0_is_the_restated_loop(tmp_path, name="alpha"):
    a, g = R.load_fixture()
    assert g["videos"][name]["with_annotation"]
    d = R.make_video_tree(tmp_path, name, a, g)
    logs = []
    for f in (lambda e: R.do_video(os.path.join(d["images"], name) + "/", d["images"], d["anns"], d["props"], d["flows"], e.do_refinement, e.add_ReID),
              lambda e: L.do_video(os.path.join(d["images"], name) + "/", d["images"], d["anns"], d["props"], d["flows"], e.do_refinement, e.add_ReID,
                                   L.weight_sets(1)[0])[0]):
        logs.append(f(R.ReplayEngines(a[f"v_{name}_refine_mask"], a[f"v_{name}_reid"], a[f"v_{name}_refine_bbox"])))
    assert len(logs[0]) == len(logs[1]) == g["videos"][name]["frames"]
    for x, y in zip(*logs):
        assert set(x) == set(y)
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    assert np.array_equal(np.array([r["png"] for r in logs[1]]), a[f"v_{name}_png"])


def test_the_restated_objective_on_a_tiny_video():
    """eval_video by hand: frames 1 .. N-2 count, an id absent from the annotation scores 1 where nothing was painted, 0 where something was."""
    import prewarp_restated as PR
    idx = np.zeros((4, 2, 3), np.uint8)
    gt = np.zeros((4, 2, 3), np.uint8)
    idx[1, 0, :2], gt[1, 0, 1:] = 1, 1          # frame 1, object 0: |R and G| = 1, |R or G| = 3
    idx[2, 1, 0] = 2                            # frame 2: object 1 painted, absent from gt -> 0; object 0 neither -> 1
    assert PR.eval_video(idx, gt, 2).tolist() == [(1 / 3 + 1) / 2, (1 + 0) / 2]


@pytest.mark.parametrize("name,seed", [("V3", 5), ("V2F300", 7), ("V8", 6)])
def test_the_kernel_tests_inputs_tell_the_weight_sets_apart(name, seed):
    """On the score inputs tests/test_gpu_live_search.py feeds the kernel, the restatement's selections under (1,0,0,0,0), (0,0,0,1,0) and
    the default weights are not all equal: a kernel that ignored its weights could not match all three."""
    per, _, _ = L.sets_inputs(name, seed)
    a = next(x for x in per if x is not None and len(x[3]) >= 5)
    sels = [L.selections(a, w).tolist() for w in L.THREE_SETS]
    assert sels[0] != sels[1] and sels[0] != sels[2] and sels[1] != sels[2], sels
    # and in the case itself two seats of EQUAL inputs select differently under their own sets
    V = L.SETS_CASES[name][0]
    ws = L.weight_sets(V, seed)
    by_T = {}
    for v, x in enumerate(per):
        if x is not None:
            by_T.setdefault(len(x[3]), []).append(L.selections(x, ws[v]).tolist())
    assert name in L.DIFFER and any(len(s) > 1 and any(t != s[0] for t in s[1:]) for s in by_T.values()), by_T
