"""Negative first-frame templates of the pre-warp merge (``--negatives``, oldmerge.py's use_ff_negative_props), the part that needs no
GPU: the numpy restatement (tests/prewarp_neg_restated.py) against what the reference itself computed with the switch on
(tests/golden/prewarp_neg_ref.npz, tools/make_golden_prewarp_neg.py), the restatement's own rules, header / binding / document
agreement of the four new entries and their argument checks (before any HIP call, so they run here), the tables and the command
lines."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
ENTRIES = (("premvos_prewarp_negatives_i32", 14), ("premvos_prewarp_gather_neg_u8", 11), ("premvos_prewarp_chain_neg_f64", 22),
           ("premvos_prewarp_paint_neg_bits_u8", 21))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLD, "prewarp_neg_host_refs.json")) as f:
        g = json.load(f)
    return np.load(os.path.join(GOLD, "prewarp_neg_ref.npz")), g


@pytest.mark.parametrize("name", ["alpha", "beta"])
def test_restatement_equals_the_reference_with_the_switch_on(fixture, name):
    import prewarp_neg_restated as RN
    import prewarp_restated as R
    ref, g = fixture
    frames = RN.fixture_video(ref, g, name)
    out = RN.merge_video(frames, g["h"], g["w"], g["weights"], negatives="all")
    assert out["negatives"] == ref[f"v_{name}_negatives"].tolist() == g["videos"][name]["negatives"] and len(out["negatives"]) == 4
    T0 = len(frames[0]["ann"])
    assert out["T_ann"] == len(g["videos"][name]["objects"]) and out["chosen"].shape[1] == out["T_ann"] + 4
    for t in range(len(frames)):
        assert out["planes"][t].shape == ref[f"v_{name}_planes_{t}"].shape
        assert np.abs(out["planes"][t] - ref[f"v_{name}_planes_{t}"]).max() <= 1e-12, t
        assert np.abs(out["weighted"][t] - ref[f"v_{name}_weighted_{t}"]).max() <= 1e-12, t
    assert np.array_equal(out["chosen"], ref[f"v_{name}_chosen"])
    assert np.abs(out["best"] - ref[f"v_{name}_best"]).max() <= 1e-12
    assert np.array_equal(out["idmap"], ref[f"v_{name}_png"])
    assert np.array_equal(R.eval_video(out["index"], ref[f"v_{name}_gt"], T0), ref[f"v_{name}_eval"])
    # the switch shows: without it the restatement gives the reference's other PNGs, which differ
    off = R.merge_video(frames, g["h"], g["w"], g["weights"])
    assert np.array_equal(off["idmap"], ref[f"v_{name}_png_off"]) and not np.array_equal(off["idmap"], out["idmap"])
    assert not (out["idmap"] > out["T_ann"]).any()                                              # a negative never shows as an object
    for t in g["videos"][name]["stolen_frames"]:                                                # the distractor's track keeps its column
        k = out["T_ann"] + out["negatives"].index(4)
        assert out["chosen"][t, k] == 4 and 4 in off["chosen"][t] and 4 not in out["chosen"][t, :out["T_ann"]]


def test_the_rules_of_the_restatement():
    import prewarp_neg_restated as RN
    h, w = 6, 8
    m = np.zeros((6, h, w), np.uint8)
    m[0, 0:2, 0:2] = 1                 # touches the annotation by exactly one pixel
    m[1, 3:5, 0:3] = 1                 # free
    m[2, 4:6, 2:5] = 1                 # overlaps proposal 1 by one pixel
    m[3, 0:2, 5:8] = 1                 # free, equal score with proposal 4
    m[4, 3:5, 6:8] = 1                 # free
    ann = np.zeros((h, w), np.uint8)   # proposal 5: the empty mask
    ann[1:3, 1:4] = 1
    s = np.array([0.9, 0.5, 0.8, 0.7, 0.7, 0.1])
    assert RN.select_negatives(m, [ann], s) == [2, 3, 4, 5]                                     # 0 touches; 2 beats 1, which then overlaps it
    assert RN.select_negatives(m, [ann], [0.9, 0.8, 0.5, 0.7, 0.7, 0.95]) == [5, 1, 3, 4]       # the empty mask is taken; equal scores in file order
    assert RN.select_negatives(m, [ann], s, K=2) == [2, 3] and RN.select_negatives(m, [ann], s, K=0) == []
    assert RN.select_negatives(m, [ann], [0.9, np.nan, 0.8, np.nan, 0.7, 0.1]) == [2, 4, 5]     # a NaN score is never taken
    assert RN.select_negatives(m, [], s) == [0, 2, 3, 4, 5]                                     # no annotation in frame 0: only each other
    assert RN.select_negatives(m[:0], [ann], []) == []
    rng = np.random.default_rng(0)
    fr = [{"score": s, "mask": m, "fwd": m, "reid": rng.standard_normal((6, 128)), "ann": [{"id": 1, "mask": ann, "fwd": ann, "reid": rng.standard_normal(128)}]},
          {"score": s, "mask": m, "fwd": m, "reid": rng.standard_normal((6, 128)), "ann": []}]
    import prewarp_restated as R
    base = R.merge_video(fr, h, w)
    for off in (None, 0):                                                                       # K = 0 equals no negatives
        out = RN.merge_video(fr, h, w, negatives=off)
        assert out["negatives"] == [] and all(np.array_equal(out[k], base[k]) for k in ("chosen", "best", "idmap", "index"))
    out = RN.merge_video(fr, h, w, negatives=2)
    assert out["negatives"] == [2, 3] and out["chosen"].shape == (2, 3) and RN.merge_video(fr, h, w, negatives="all")["negatives"] == [2, 3, 4, 5]
    none = [dict(f, ann=[]) for f in fr]                                                        # no annotated object: no negatives
    assert RN.negatives_of(none, h, w, "all") == [] and RN.negatives_of(fr, h, w, "all") == [2, 3, 4, 5]


def test_header_signatures_and_documents_name_the_new_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "prewarp_ops.hip")).read()
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
        text = open(os.path.join(ROOT, doc)).read()
        assert f"{len(declared)} entry points, ABI v21" in text and "--negatives" in text, doc
    for cite in ("oldmerge.py:63-85", "oldmerge.py:43", "oldmerge.py:137-138,147", "oldmerge.py:138,147", "oldmerge.py:148,173", "oldmerge.py:168-174"):
        assert cite in hdr, cite
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("8.5.2", "use_ff_negative_props", "quality on DAVIS unmeasured", "pass --negatives K", "readback"):
        assert word in design, word
    assert not re.search(r"atomicAdd\([^)]*(float|double)", src)                                # integers and float64 compares only


def test_the_new_entries_refuse_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.int64)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused
    # a 2-frame video: P = 2, 2; one object, in frame 0; one negative: slots [cur 0..3 | fwd 4..7 | ann 8 | annfwd 9 | neg 10]
    blocks = np.array([[0, 2, 8, 1, 10, 1, 0, 0], [2, 2, 4, 2, 9, 1, 4, 4]], np.int32)
    poff, first = np.array([0, 2, 4], np.int32), np.array([0, 1, 1], np.int32)

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    def neg(bits=one, S=11, stride=8, hw=60, cur0=0, P0=2, ann0=8, A0=1, score=one, K=-1, conflict=one, taken=one, count=one):
        return lib.premvos_prewarp_negatives_i32(bits, S, stride, hw, cur0, P0, ann0, A0, score, K, conflict, taken, count, None)

    def gather(bits=one, S=11, stride=8, cur0=0, P0=2, neg0=10, n=1, taken=one, ep=one, et=one):
        return lib.premvos_prewarp_gather_neg_u8(bits, S, stride, cur0, P0, neg0, n, taken, ep, et, None)

    def chain(inter=one, ni=10, na=10, bh=blocks, ph=poff, fh=first, N=2, T=2, n_neg=1, wts=one, W=1, chosen=one, weighted=None):
        return lib.premvos_prewarp_chain_neg_f64(inter, ni, one, na, bh.ctypes.data, one, ph.ctypes.data, one, fh.ctypes.data, one, N, T, n_neg, one, one,
                                                 one, wts, W, chosen, one, weighted, None)

    def paint(bits=one, S=11, stride=8, hw=60, bh=blocks, fh=first, ids=one, ann0=8, N=2, T=2, n_neg=1, W=1, idmap=one, gt=None, T0=0, counts=None):
        return lib.premvos_prewarp_paint_neg_bits_u8(bits, S, stride, hw, bh.ctypes.data, one, fh.ctypes.data, one, ids, ann0, one, one, N, T, n_neg, W,
                                                     idmap, gt, T0, counts, None)

    for f in (neg, paint, gather):
        refused(f(bits=None), b"null")
        refused(f(S=0), b"bad dims")
        refused(f(stride=12), b"multiple of 8")
        refused(f(bits=one + 4), b"8-byte aligned")
    refused(neg(hw=0), b"bad dims")
    refused(neg(hw=65), b"multiple of 8")
    refused(neg(P0=-1), b"bad dims")
    refused(neg(P0=257, S=1000), b"at most 256")
    refused(neg(A0=65, S=1000), b"at most 256")
    refused(neg(count=None), b"null")
    refused(neg(score=None), b"null")
    refused(neg(conflict=None), b"null")
    refused(neg(taken=None), b"null")
    refused(neg(cur0=10), b"outside the pool")
    refused(neg(ann0=11), b"outside the pool")
    refused(gather(n=3), b"bad dims")                                                           # more negatives than proposals
    refused(gather(n=-1), b"bad dims")
    refused(gather(taken=None), b"null")
    refused(gather(ep=None), b"null")
    refused(gather(neg0=11), b"outside the pool")
    refused(gather(neg0=1), b"overlap")
    assert gather(n=0, taken=None) == 0                                                         # nothing to do, nothing launched
    refused(chain(wts=None), b"null")
    refused(chain(T=65), b"at most 64")
    refused(chain(n_neg=3), b"negatives among")
    refused(chain(n_neg=-1), b"negatives among")
    refused(chain(n_neg=0), b"first")                                                           # first runs to 1, T is 2
    refused(chain(T=3, n_neg=1), b"first")
    refused(chain(T=3, n_neg=2), b"the video's tables ask")                                     # block 0 has 1 + 1 columns, not 1 + 2
    refused(chain(W=2, weighted=one), b"one weight set")
    refused(chain(ni=7), b"do not fit")
    refused(paint(ids=None), b"null")
    refused(paint(idmap=None), b"neither")
    refused(paint(n_neg=3), b"negatives among")
    refused(paint(n_neg=0), b"first")
    refused(paint(counts=one, gt=one, T0=2), b"bit planes")                                     # T0 beyond the annotated templates
    refused(paint(ann0=11), b"annotation masks")
    refused(paint(S=3), b"outside the pool")
    # the old entries are the n_neg = 0 call: their refusals keep their names
    assert lib.premvos_prewarp_chain_f64(one, 10, one, 10, blocks.ctypes.data, one, poff.ctypes.data, one, first.ctypes.data, one, 2, 2, one, one, one,
                                         one, 1, one, one, None, None) == -1 and lib.premvos_last_error().startswith(b"prewarp_chain: first")


def test_tables_with_and_without_negatives():
    from premvos_amd import _lib, prewarp as pw
    old = pw.Tables([3, 0, 2], [2, 0, 1])                                                       # (the numbers tests/test_cpu_prewarp.py pins)
    same = pw.Tables([3, 0, 2], [2, 0, 1], 0)
    for k in ("N", "sumP", "T", "S", "cur0", "fwd0", "ann0", "annfwd0", "n_inter", "n_areas"):
        assert getattr(old, k) == getattr(same, k), k
    assert (old.T, old.T_ann, old.n_neg, old.S) == (3, 3, 0, 16)
    assert old.blocks.tolist() == same.blocks.tolist() == [[0, 3, 10, 2, 0, 0, 0, 0], [3, 0, 5, 3, 13, 2, 6, 5], [3, 2, 8, 0, 15, 0, 6, 10]]
    tab = pw.Tables([3, 0, 2], [2, 0, 1], 2)
    assert (tab.T, tab.T_ann, tab.n_neg, tab.S, tab.neg0) == (5, 3, 2, 18, 16) and tab.first.tolist() == [0, 2, 2, 3] == old.first.tolist()
    assert tab.poff.tolist() == old.poff.tolist() and (tab.ann0, tab.annfwd0) == (old.ann0, old.annfwd0)
    assert tab.blocks.tolist() == [[0, 3, 10, 2, 16, 2, 0, 0], [3, 0, 5, 3, 13, 2, 12, 7], [3, 2, 8, 0, 15, 0, 12, 12]]
    assert (tab.n_inter, tab.n_areas) == (12, 14)
    with pytest.raises(AssertionError):
        pw.Tables([3, 0, 2], [2, 0, 1], 4)                                                      # more negatives than frame 0 has proposals
    with pytest.raises(_lib.PremvosError, match="pass --negatives K"):
        pw.Tables([100], [10], 60).check_caps()                                                 # 70 templates
    with pytest.raises(_lib.PremvosError, match="LDS") as e:
        pw.Tables([4], [65]).check_caps()
    assert "--negatives" not in str(e.value)                                                    # today's message without negatives
    assert pw.negatives_cap(None) is None and pw.negatives_cap("all") == -1 and pw.negatives_cap(0) == 0 and pw.negatives_cap(3) == 3
    for bad in ("some", -1, 1.5, True):
        with pytest.raises(ValueError):
            pw.negatives_cap(bad)
    assert [pw.negatives_room(n, 7, 2) for n in (None, "all", 0, 3, 9)] == [0, 7, 0, 3, 7] and pw.negatives_room("all", 7, 0) == 0


def test_command_lines_and_output_names(capsys):
    from premvos_amd import stream, track
    for argv, word in ((["--negatives"], "only with --prewarp or --prewarp-search"), (["--negatives", "3"], "only with --prewarp or --prewarp-search"),
                       (["--prewarp", "--negatives", "-1"], "--negatives"), (["--prewarp", "--negatives", "few"], "--negatives"),
                       (["--search", "3", "--negatives"], "only with --prewarp")):
        with pytest.raises(SystemExit) as e:
            track.main(["--root", "/nonexistent"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    for argv, want in ((["--prewarp", "--negatives"], "all"), (["--prewarp", "--negatives", "2"], 2), (["--prewarp-search", "4", "--negatives", "0"], 0),
                       (["--prewarp"], None), (["--prewarp", "--negatives", "--ensemble", "1,1,1,1,1;1,2,3,4,5", "--late-annotations", "--eval", "--overlay"], "all")):
        assert getattr(track.parse_args(["--root", "/nonexistent"] + argv), "negatives", None) == want, argv
    assert track.main(["--root", "/nonexistent", "--prewarp", "--negatives", "--check-only"]) == 2      # accepted; the inputs are what is missing
    capsys.readouterr()
    assert track.prewarp_stem(None) == "prewarp" and track.prewarp_stem("all") == track.prewarp_stem(0) == "prewarp_neg"
    with pytest.raises(SystemExit):
        track.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--negatives", "oldmerge.py:43,63-85", "output/final_prewarp_neg/", "eval_prewarp_neg/", "overlay_prewarp_neg/",
                 "premvos_amd_davis_eval_prewarp_neg.json", "prewarp_neg_search.json", "final_prewarp_neg_ensemble/", "prewarp_neg_ensemble.json",
                 "output/prewarp_negatives.json"):
        assert word in text, word
    for argv in (["--negatives"], ["--track", "--negatives", "2"], ["--reid", "--negatives"]):
        with pytest.raises(SystemExit) as e:
            stream.parse_args(argv)
        assert e.value.code == stream.REFUSE_NEGATIVES_WITHOUT_PREWARP and "only with --track --prewarp" in str(e.value.code), argv
    with pytest.raises(SystemExit) as e:
        stream.parse_args(["--prewarp", "--negatives"])
    assert e.value.code == stream.REFUSE_PREWARP_WITHOUT_TRACK
    with pytest.raises(SystemExit) as e:
        stream.parse_args(["--track", "--prewarp", "--negatives", "x"])
    assert "--negatives" in str(e.value.code)
    assert stream.parse_args(["--track", "--prewarp", "--negatives"]).negatives == "all"
    assert stream.parse_args(["--track", "--prewarp", "--negatives", "3"]).negatives == 3 and not hasattr(stream.parse_args(["--track", "--prewarp"]), "negatives")
    assert stream._prewarp_options(None, 3)["negatives"] == 3 and "negatives" not in stream._prewarp_options(None)
