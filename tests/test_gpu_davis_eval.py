"""premvos_davis_counts_u8 and premvos_amd.evaluate on the GPU against the numpy restatement of tools/davis_eval.py
(tests/davis_restated.py, pinned to the tool itself by tests/test_cpu_davis_gpu_host.py): counts and maps bit for bit, the batch, the
default radius, repeatability, the whole file protocol, and the evaluator inside the merge loop (`--eval`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import davis_restated as D  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [1, 3, 7]


def _dev(a):
    from premvos_amd import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.resolve_device())


# (h, w, forced radius): single pixel; image smaller than the disk; no dimension a multiple of a tile; tile-aligned height; one pixel
# past a 32 x 64 tile both ways; the 1080p radius across several tiles; wider than tall by far; and the two radii at which a row of
# boundary bits (64 + 2r columns) takes three 64-bit words instead of two: a 4K frame's 36 and the limit 48
@pytest.mark.parametrize("h,w,r", [(1, 1, 1), (5, 7, 3), (37, 53, 2), (64, 100, 8), (33, 65, 8), (97, 131, 18), (3, 200, 18),
                                   (70, 150, 36), (40, 135, 48)])
def test_counts_and_maps_equal_the_restatement(h, w, r):
    from premvos_amd import evaluate as ev
    res, gt = D.case_frames(h, w, 1000 * h + w)
    if h * w >= 12:                                          # what case_frames promises, on the shapes with room for it
        assert (res[0] == 9).any() and (res[0] == 3).any() and not (gt[0] == 3).any() and (gt[0] == 7).any() and not (res[0] == 7).any()
        assert not (res[1] == 7).any() and not (gt[1] == 7).any() and (res[2] == 1).all()
        assert all((edge == 1).any() for m in (res[0], gt[0]) for edge in (m[0], m[-1], m[:, 0], m[:, -1]))
    counts, maps = ev.davis_counts(_dev(res), _dev(gt), IDS, radius=r, maps=True)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (3, 3, 6) and tuple(maps.shape) == (3, 3, 4, h, w)
    counts, maps = counts.cpu().numpy(), maps.cpu().numpy()
    for k in range(3):
        want_c, want_m = D.counts(res[k], gt[k], IDS, r)
        assert np.array_equal(maps[k], want_m), (k, [int((maps[k, t, j] != want_m[t, j]).sum()) for t in range(3) for j in range(4)])
        assert np.array_equal(counts[k], want_c), (k, counts[k], want_c)
    assert not counts[1, 2].any()                            # the id in neither map: six zeros
    J, F = ev.measures(counts)
    for k in range(3):
        for t, i in enumerate(IDS):
            assert float(J[k, t]) == D.db_eval_iou(gt[k] == i, res[k] == i)
            if r == D.bound_pix(h, w):
                assert float(F[k, t]) == D.db_eval_boundary(res[k] == i, gt[k] == i)


def test_batch_default_radius_and_repeatability():
    from premvos_amd import evaluate as ev
    h, w = 480, 854
    res = np.stack([D.blob_maps(h, w, 50 + k)[0] for k in range(4)])
    gt = np.stack([D.blob_maps(h, w, 50 + k)[1] for k in range(4)])
    assert ev.bound_pix(h, w) == 8
    want = D.counts(res[0], gt[0], IDS)[0]                   # the default radius of both
    assert want[:, 2:].all(), want                           # every object has boundary pixels and matches in both directions
    rd, gd = _dev(res), _dev(gt)
    one = ev.davis_counts(rd[0], gd[0], IDS).cpu().numpy()
    assert one.shape == (1, 3, 6) and np.array_equal(one[0], want)
    batch = ev.davis_counts(rd, gd, IDS)
    singles = [ev.davis_counts(rd[k], gd[k], torch.tensor(IDS, dtype=torch.int32, device=rd.device)).cpu().numpy()[0] for k in range(4)]
    assert np.array_equal(batch.cpu().numpy(), np.stack(singles))
    again = ev.davis_counts(rd, gd, IDS)
    assert torch.equal(batch, again)
    seq = ev.SequenceEval(IDS, ["a", "b", "c", "d"])
    for k in (2, 0, 3, 1):
        seq.add(k, rd[k], gd[k])
    assert torch.equal(seq.counts, batch)
    J, F = ev.measures(batch)
    assert seq.finish() == {i: (float(np.mean(J[:, t])), float(np.mean(F[:, t]))) for t, i in enumerate(IDS)}


def test_limits_and_shape_mismatch():
    from premvos_amd import _lib, evaluate as ev
    a = _dev(np.zeros((4, 6), np.uint8))
    with pytest.raises(_lib.PremvosError, match="48"):
        ev.davis_counts(a, a, IDS, radius=49)
    with pytest.raises(_lib.PremvosError, match="255"):
        ev.davis_counts(a, a, list(range(256)))
    with pytest.raises(ValueError, match="differ in shape"):
        ev.davis_counts(a, _dev(np.zeros((4, 7), np.uint8)), IDS)
    assert tuple(ev.davis_counts(a, a, []).shape) == (1, 0, 6)
    big = ev.davis_counts(a, a, [0, 300, -1], radius=48).cpu().numpy()[0]          # ids no uint8 map can hold: zeros; 0 = the background
    assert big[0].tolist() == [24, 24, 0, 0, 0, 0] and not big[1:].any()


def test_evaluate_equals_the_restated_protocol(tmp_path):
    from premvos_amd import evaluate as ev
    results, anns = D.make_tree(tmp_path)
    want = D.evaluate(results, anns)
    assert ev.evaluate(results, anns) == want
    assert ev.evaluate(results, anns, ["beta"]) == D.evaluate(results, anns, ["beta"])
    assert ev.main(["--root", str(tmp_path), "--results", "results", "--annotations", "annotations"]) == 0
    assert json.load(open(tmp_path / "output" / "premvos_amd_davis_eval.json")) == want
    D.write_index_png(os.path.join(results, "beta", "00001.png"), np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError, match="differs from the annotation's"):
        ev.evaluate(results, anns, ["beta"])


# ------------------------------------------------------------------------------------------------------------- inside the merge loop
def _child(module, root, *extra, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "PREMVOS_SIDECAR")}
    env.update({"PYTHONPATH": REPO, "PREMVOS_DRIVER_BATCH": "2", "PREMVOS_STREAM_REFINE_LANES": "2"})
    cmd = [sys.executable, "-m", module, "--root", str(root)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def _tree(root, videos):
    """The synthetic tree of the --track tests (tests/stream_reid_tree.py + the two `live` configurations) with an annotation for
    EVERY frame of 'bear' (two objects, ids 1 and 3, drifting with the frames) and none for the other videos."""
    import stream_reid_tree as T
    root.mkdir()
    T.make_tree(root, videos=videos)
    (root / "code" / "refinement_net" / "configs").mkdir(parents=True)
    (root / "code" / "refinement_net" / "configs" / "live").write_text(json.dumps({"model": "live", "load": "../weights/refinement_specific_weights"}))
    (root / "code" / "ReID_net" / "configs" / "live").write_text(json.dumps(
        {"model": "Re-ID", "load": "../weights/ReID_general_weights", "input_size": [128, 128], "network": T.REID_NETWORK}))
    for k in range(videos["bear"]):
        ann = np.zeros((120, 200), np.uint8)
        ann[20 + k:70 + k, 30 + 2 * k:90 + 2 * k] = 1
        ann[60:110, 120 - k:180 - k] = 3
        D.write_index_png(str(root / "data" / "DAVIS" / "Annotations" / "480p" / "bear" / f"{k:05d}.png"), ann)
    return T.STREAM_ARGS


def _files(base):
    return sorted(str(p.relative_to(base)) for p in base.rglob("*") if p.is_file())


def test_eval_inside_the_merge_loop_equals_evaluate_and_leaves_the_trees_alone(tmp_path):
    """Copy A: `stream --track`.  Copy B: `stream --track --eval`, then `track --eval` on B's own intermediate tree (the tracker's
    non-resident-feed step).  The per-video file and the summary of each equal evaluate() on the PNGs that were written."""
    from premvos_amd import evaluate as ev
    videos = {"bear": 5, "camel": 3}
    args = _tree(tmp_path / "a", videos)
    _tree(tmp_path / "b", videos)
    _child("premvos_amd.stream", tmp_path / "a", "--batch", "2", "--track", *args)
    out = _child("premvos_amd.stream", tmp_path / "b", "--batch", "2", "--track", "--eval", *args)
    assert "camel: no templates, not evaluated" in out and "J&F" in out
    a, b = tmp_path / "a" / "output", tmp_path / "b" / "output"
    for sub in ("intermediate", "final"):
        assert _files(a / sub) == _files(b / sub) and len(_files(a / sub)) >= 8, sub
        for f in _files(a / sub):
            assert (a / sub / f).read_bytes() == (b / sub / f).read_bytes(), (sub, f)
    assert not (a / "eval").exists() and _files(b / "eval") == ["bear.json"]
    anns = str(tmp_path / "b" / "data" / "DAVIS" / "Annotations" / "480p")
    want = ev.evaluate(str(b / "final"), anns, ["bear"])
    assert want == D.evaluate(str(b / "final"), anns, ["bear"]) and want["objects"] == 2
    assert 0 < want["mean_J"] < 1, want                               # non-vacuous: the objects are tracked, and not perfectly
    names, ids, counts = D.sequence_counts(str(b / "final" / "bear"), os.path.join(anns, "bear"))

    def check():
        d = json.load(open(b / "eval" / "bear.json"))
        assert d["video"] == "bear" and d["frames"] == names == ["00001", "00002", "00003"] and d["ids"] == ids == [1, 3]
        assert np.array_equal(np.array(d["counts"]), counts)
        r = ev.sequence_means(ids, counts)
        assert d["J"] == {str(i): r[i][0] for i in ids} and d["F"] == {str(i): r[i][1] for i in ids}
        assert json.load(open(b / "premvos_amd_davis_eval.json")) == want
    check()
    before = {f: (b / "final" / f).read_bytes() for f in _files(b / "final")}
    os.remove(b / "eval" / "bear.json")
    os.remove(b / "premvos_amd_davis_eval.json")
    out = _child("premvos_amd.track", tmp_path / "b", "--eval")
    assert "camel: no templates, not evaluated" in out and "J&F" in out
    assert {f: (b / "final" / f).read_bytes() for f in _files(b / "final")} == before
    check()
    assert ev.main(["--root", str(tmp_path / "b"), "--collect"]) == 0 and json.load(open(b / "premvos_amd_davis_eval.json")) == want
