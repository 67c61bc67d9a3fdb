"""The host side of the GPU DAVIS evaluator (premvos_amd/evaluate.py, premvos_davis_counts_u8) without a GPU: the numpy restatement
the GPU tests compare against equals tools/davis_eval.py, the measures made of its counts are the same floats, the per-video count
files sum up to the same dict, the library refuses bad arguments before any HIP call, and the ABI documents name the entry."""
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import davis_restated as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tools_davis_eval():
    pytest.importorskip("scipy")
    spec = importlib.util.spec_from_file_location("davis_eval", os.path.join(ROOT, "tools", "davis_eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------- helper equals tools
@pytest.mark.parametrize("h,w,r", [(5, 7, 3), (37, 53, 2), (64, 100, 8), (97, 131, 18), (3, 200, 18)])
def test_the_restated_dilation_equals_scipys(h, w, r):
    from scipy import ndimage
    E = _tools_davis_eval()
    res, gt = D.case_frames(h, w, 11 * h + w)
    for m in (res[0] == 1, gt[0] == 1, res[0] == 3, gt[0] == 7):
        b = D.seg2bmap(m)
        assert np.array_equal(b, E.seg2bmap(m))
        assert np.array_equal(D.dilate_disk(b, r), ndimage.binary_dilation(b, structure=E._disk(r)))


def test_the_restated_measures_equal_tools_davis_eval():
    E = _tools_davis_eval()
    for h, w, seed in ((37, 53, 1), (64, 100, 2), (120, 90, 3), (1, 1, 4), (3, 200, 5)):
        res, gt = D.case_frames(h, w, seed)
        for k in range(3):
            for i in (1, 3, 7, 9):
                R, G = res[k] == i, gt[k] == i
                assert D.db_eval_iou(G, R) == E.db_eval_iou(G, R)
                assert D.db_eval_boundary(R, G) == E.db_eval_boundary(R, G)


def test_the_restated_protocol_equals_tools_davis_eval(tmp_path):
    E = _tools_davis_eval()
    results, anns = D.make_tree(tmp_path)
    assert not os.path.exists(os.path.join(results, "alpha", "00002.png"))                    # the missing result file
    want = E.evaluate(results, anns)
    assert D.evaluate(results, anns) == want
    assert want["objects"] == 3 and want["sequences"] == 2 and 0 < want["mean_J"] < 1 and 0 < want["mean_F"] < 1
    assert D.evaluate(results, anns, ["beta"]) == E.evaluate(results, anns, ["beta"])
    last = D.read_ids(os.path.join(anns, "alpha", "00004.png"))
    assert last[-1, -1] == 1 and (last[-1, :] == 1).any() and (last[:, -1] == 1).any()          # touches the bottom and right borders
    assert not (D.read_ids(os.path.join(results, "alpha", "00003.png")) == 3).any()           # the lost object


# ------------------------------------------------------------------------------------------------------------------------ measures
def test_measures_of_the_restated_counts_are_the_restated_floats():
    from premvos_amd import evaluate as ev
    assert ev.bound_pix(480, 854) == 8 == D.bound_pix(480, 854) and ev.bound_pix(1080, 1920) == 18 and ev.bound_pix(2160, 3840) == 36
    ids = [1, 3, 7, 9, 11]
    seen = set()
    for h, w, seed in ((37, 53, 1), (64, 100, 2), (5, 7, 3), (1, 1, 4)):
        res, gt = D.case_frames(h, w, seed)
        counts = np.stack([D.counts(res[k], gt[k], ids)[0] for k in range(3)])
        J, F = ev.measures(counts)
        assert J.shape == F.shape == (3, len(ids)) and J.dtype == F.dtype == np.float64
        for k in range(3):
            for t, i in enumerate(ids):
                assert float(J[k, t]) == D.db_eval_iou(gt[k] == i, res[k] == i)
                assert float(F[k, t]) == D.db_eval_boundary(res[k] == i, gt[k] == i)
                seen.add((counts[k, t, 2] > 0, counts[k, t, 3] > 0))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}               # the three empty-boundary cases and 2pr/(p+r)
    assert ev.measures(np.zeros((1, 1, 6), np.int64))[0][0, 0] == 1.0                         # the empty union


def test_sequence_eval_without_frames_and_summarise_equal_the_restated_dict(tmp_path):
    from premvos_amd import evaluate as ev
    results, anns = D.make_tree(tmp_path)
    eval_dir = tmp_path / "output" / "eval"
    for video in ("alpha", "beta"):
        names, ids, counts = D.sequence_counts(os.path.join(results, video), os.path.join(anns, video))
        assert ev.sequence_means(ids, counts) == D.evaluate_sequence(os.path.join(results, video), os.path.join(anns, video))
        ev.write_video_file(str(eval_dir / (video + ".json")), video, names, ids, counts)
        d = json.load(open(eval_dir / (video + ".json")))
        assert d["frames"] == names and d["ids"] == ids and np.array_equal(np.array(d["counts"]), counts) and set(d["J"]) == {str(i) for i in ids}
    want = D.evaluate(results, anns)
    assert ev.summarise(str(eval_dir)) == want
    assert ev.summarise(str(eval_dir), ["beta"]) == D.evaluate(results, anns, ["beta"])
    assert ev.main(["--root", str(tmp_path), "--collect"]) == 0                               # host only
    assert json.load(open(tmp_path / "output" / "premvos_amd_davis_eval.json")) == want


# ---------------------------------------------------------------------------------------------------------------------- the C-ABI
def test_library_built_for_gfx950_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21
    one = np.zeros(1024, np.int64).ctypes.data
    f = lib.premvos_davis_counts_u8
    assert f(None, one, 1, 4, 4, one, 1, 2, one, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert f(one, None, 1, 4, 4, one, 1, 2, one, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert f(one, one, 1, 4, 4, None, 1, 2, one, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert f(one, one, 1, 4, 4, one, 1, 2, None, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert f(one, one, -1, 4, 4, one, 1, 2, one, None, None) == -1 and b"negative" in lib.premvos_last_error()
    assert f(one, one, 1, 4, 4, one, -1, 2, one, None, None) == -1 and b"negative" in lib.premvos_last_error()
    assert f(one, one, 1, 0, 4, one, 1, 2, one, None, None) == -1 and f(one, one, 1, 4, 0, one, 1, 2, one, None, None) == -1
    assert f(one, one, 1, 4, 4, one, 1, 0, one, None, None) == -1 and b"48" in lib.premvos_last_error()
    assert f(one, one, 1, 4, 4, one, 1, 49, one, None, None) == -1 and b"48" in lib.premvos_last_error()
    assert f(one, one, 1, 4, 4, one, 256, 2, one, None, None) == -1 and b"255" in lib.premvos_last_error()
    assert f(one, one, 0, 4, 4, one, 1, 2, one, None, None) == 0                              # nothing to do: no launch
    assert f(one, one, 1, 4, 4, one, 0, 2, one, None, None) == 0


def test_header_signatures_and_documents_name_the_entry():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    name = "premvos_davis_counts_u8"
    assert name in declared and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 11
    assert _lib.ABI_VERSION == 21                                             # additive: nothing an older caller binds has changed
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert name in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v{_lib.ABI_VERSION}" in open(os.path.join(ROOT, doc)).read(), doc
    for cite in ("tools/davis_eval.py:33-47", "tools/davis_eval.py:25-71"):
        assert cite in hdr
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "davis_ops.hip")).read()
    assert re.search(r"__launch_bounds__\(THREADS\) void davis_counts_kernel", src) and "THREADS = 256" in src
    assert not re.search(r"sqrt|\bfloat\b|\bdouble\b", src)                   # integers only: the disk test is dx*dx + dy*dy <= r*r


# --------------------------------------------------------------------------------------------------------------------- command line
def test_check_only_names_the_missing_folder_and_eval_needs_track(tmp_path, capsys):
    from premvos_amd import evaluate as ev, stream
    assert ev.main(["--root", str(tmp_path), "--check-only"]) == 2
    out = capsys.readouterr().out
    assert str(tmp_path / "output/final") in out and str(tmp_path / "data/DAVIS/Annotations/480p") in out
    (tmp_path / "output" / "final").mkdir(parents=True)
    assert ev.main(["--root", str(tmp_path), "--check-only"]) == 2
    out = capsys.readouterr().out
    assert str(tmp_path / "output/final") not in out and str(tmp_path / "data/DAVIS/Annotations/480p") in out
    (tmp_path / "data" / "DAVIS" / "Annotations" / "480p").mkdir(parents=True)
    assert ev.main(["--root", str(tmp_path), "--check-only"]) == 0
    assert ev.main(["--root", str(tmp_path), "--collect"]) == 2 and "output/eval" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="--eval .* needs --track"):
        stream.parse_args(["--eval"])
    with pytest.raises(SystemExit, match="--eval .* needs --track"):
        stream.parse_args(["--reid", "--eval"])
    a = stream.parse_args(["--track", "--eval"])
    assert a.track and a.eval and a.reid and not stream.parse_args(["--track"]).eval


def test_a_png_that_is_not_a_palette_image_is_refused_with_the_host_tool_named(tmp_path):
    from PIL import Image
    from premvos_amd import evaluate as ev
    Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match=r"tools/davis_eval\.py"):
        ev._read_ids(str(tmp_path / "rgb.png"))
    D.write_index_png(str(tmp_path / "p.png"), np.arange(20, dtype=np.uint8).reshape(4, 5))
    assert np.array_equal(ev._read_ids(str(tmp_path / "p.png")), np.arange(20, dtype=np.uint8).reshape(4, 5))


def test_the_module_keeps_the_packages_rules():
    src = open(os.path.join(ROOT, "premvos_amd", "evaluate.py")).read()
    assert "import oracle" not in src and "from oracle" not in src and "import tools" not in src and "from tools" not in src
    assert "scipy" not in src and "resolve_device" in src


def test_the_timing_tool_reads_its_arguments_and_judges_the_loop_on_the_host():
    sys.path.insert(0, ROOT)
    from tools import time_davis_eval as TD
    a = TD.parse_args([])
    assert (a.frames, a.loop_frames, a.alternations, a.child) == (64, 64, 2, None) and a.out.endswith("profiles/davis_eval.json")
    assert [leg[1:] for leg in TD.LEGS] == [(480, 854, 3), (480, 854, 10), (1080, 1920, 3)]
    with pytest.raises(SystemExit):
        TD.parse_args(["--child", "nonsense"])
    c = TD.loop_condition([50.0, 51.0], [49.0, 50.5])
    assert c["spread_without_eval"] == 1.0 and c["largest_distance_with_eval"] == 1.5 and c["within_twice_the_spread"]
    assert not TD.loop_condition([50.0, 50.2], [49.0, 50.0])["within_twice_the_spread"]
    res, gt = TD.blob_clip(48, 64, 3, 4)
    assert res.shape == gt.shape == (4, 48, 64) and set(np.unique(gt)) == {0, 1, 2, 3}
    c, _ = D.counts(res[1], gt[1], [1, 2, 3])
    assert (c[:, 0] > 0).all() and (c[:, 0] < c[:, 1]).all()                 # overlapping, not identical: J strictly between 0 and 1
