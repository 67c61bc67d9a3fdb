"""`python -m premvos_amd.stream --track --prewarp`: frames in, the pre-warp merge's PNGs out, one process.  The yardstick is the
two-program path -- `stream --reid`, then `premvos_amd.track --prewarp` on the tree it wrote -- and the bar is equality of every file
under output/intermediate/ and output/final_prewarp/.  Every program runs in a fresh child process under its own time limit, one at a
time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_reid_tree as T  # noqa: E402
import track_restated as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files(base):
    return sorted(str(p.relative_to(base)) for p in base.rglob("*") if p.is_file())


def _annotations():
    """bear: two objects whose ids are not adjacent; camel: one object -- the pool is rebuilt across a video boundary"""
    bear = np.zeros((120, 200), np.uint8)
    bear[20:70, 30:90] = 1
    bear[60:110, 120:180] = 3
    camel = np.zeros((120, 200), np.uint8)
    camel[30:100, 50:150] = 2
    return {"bear": bear, "camel": camel}


def _tree(root, videos):
    """The synthetic tree of the --reid tests + the ReID `live` configuration (the only engine this merge loads) + a first-frame
    annotation for every video of ``videos``."""
    root.mkdir()
    T.make_tree(root, videos=videos)
    (root / "code" / "ReID_net" / "configs" / "live").write_text(json.dumps(
        {"model": "Re-ID", "load": "../weights/ReID_general_weights", "input_size": [128, 128], "network": T.REID_NETWORK}))
    anns = _annotations()
    for name in videos:
        d = root / "data" / "DAVIS" / "Annotations" / "480p" / name
        d.mkdir(parents=True)
        R.write_index_png(str(d / "00000.png"), anns[name])
    return anns


def _child(module, root, *extra, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "PREMVOS_SIDECAR")}
    env.update({"PYTHONPATH": REPO, "PREMVOS_DRIVER_BATCH": "2", "PREMVOS_STREAM_REFINE_LANES": "2"})
    cmd = [sys.executable, "-m", module, "--root", str(root)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r


def _png(fn):
    from PIL import Image
    return np.array(Image.open(fn))


def test_one_command_writes_the_tree_and_the_pngs_of_stream_reid_then_track_prewarp(tmp_path):
    """Copy A: `stream --reid`, then `track --prewarp`.  Copy B: `stream --track --prewarp`.  'bear' (5 frames, objects 1 and 3) and
    'camel' (3 frames, object 2) cross chunk (--batch 2), launch (PREMVOS_DRIVER_BATCH=2) and lane (2 lanes) boundaries.  Non-vacuity is
    judged on copy A, where no new code runs."""
    videos = {"bear": 5, "camel": 3}
    anns = _tree(tmp_path / "a", videos)
    _tree(tmp_path / "b", videos)
    _child("premvos_amd.stream", tmp_path / "a", "--batch", "2", "--reid", *T.STREAM_ARGS)
    _child("premvos_amd.track", tmp_path / "a", "--prewarp")
    out = _child("premvos_amd.stream", tmp_path / "b", "--batch", "2", "--track", "--prewarp", *T.STREAM_ARGS).stdout
    assert "frames: 8" in out
    a, b = tmp_path / "a" / "output", tmp_path / "b" / "output"
    for sub in ("intermediate", "final_prewarp"):
        fa, fb = _files(a / sub), _files(b / sub)
        assert fa == fb, sub
        for f in fa:
            assert (a / sub / f).read_bytes() == (b / sub / f).read_bytes(), (sub, f)
    assert _files(a / "final_prewarp") == [f"bear/{t:05d}.png" for t in range(5)] + [f"camel/{t:05d}.png" for t in range(3)]
    assert sum(f.startswith("ReID_proposals") for f in _files(b / "intermediate")) == 8
    assert not (a / "final").exists() and not (b / "final").exists()
    # non-vacuity, on copy A: frame 0 is the annotation, an annotated id still has pixels in bear's last frame
    for name in videos:
        assert np.array_equal(_png(a / "final_prewarp" / name / "00000.png"), anns[name]), name
    per_frame = [{int(i): int((_png(a / "final_prewarp" / "bear" / f"{t:05d}.png") == i).sum()) for i in (1, 3)} for t in range(5)]
    print("copy A, pixels per annotated object and frame:", per_frame)
    last = _png(a / "final_prewarp" / "bear" / "00004.png")
    assert set(np.unique(last)) <= {0, 1, 3} and ((last == 1).any() or (last == 3).any()), per_frame
    man_a = json.load(open(a / "premvos_amd_manifest.json"))
    man_b = json.load(open(b / "premvos_amd_manifest.json"))
    from premvos_amd import prewarp as pw
    assert "track" not in man_a and man_b["track"] == {"merge": "prewarp", "reid_config": "code/ReID_net/configs/live",
                                                       "weights": pw.normalised().tolist(), "output": "output/final_prewarp"}
    assert man_b["reid"] == man_a["reid"]


def test_eval_and_overlay_ride_along_and_change_no_png(tmp_path):
    from PIL import Image
    videos = {"bear": 5}
    _tree(tmp_path / "plain", videos)
    _tree(tmp_path / "full", videos)
    # an annotation for every frame, so that there is something to score (the merge reads frame 0's only)
    for t in range(1, 5):
        for tag in ("plain", "full"):
            R.write_index_png(str(tmp_path / tag / "data" / "DAVIS" / "Annotations" / "480p" / "bear" / f"{t:05d}.png"), _annotations()["bear"])
    _child("premvos_amd.stream", tmp_path / "plain", "--batch", "2", "--track", "--prewarp", *T.STREAM_ARGS)
    _child("premvos_amd.stream", tmp_path / "full", "--batch", "2", "--track", "--prewarp", "--eval", "--overlay", *T.STREAM_ARGS)
    p, f = tmp_path / "plain" / "output", tmp_path / "full" / "output"
    pngs = _files(p / "final_prewarp")
    assert pngs == _files(f / "final_prewarp") == [f"bear/{t:05d}.png" for t in range(5)]
    for fn in pngs:
        assert (p / "final_prewarp" / fn).read_bytes() == (f / "final_prewarp" / fn).read_bytes(), fn
    assert _png(p / "final_prewarp" / "bear" / "00000.png").any()
    counts = json.load(open(f / "eval_prewarp" / "bear.json"))
    assert counts
    summary = json.load(open(f / "premvos_amd_davis_eval_prewarp.json"))
    assert "mean_J" in summary and "mean_F" in summary
    assert _files(f / "overlay_prewarp") == [f"bear/{t:05d}.jpg" for t in range(5)]
    for t in range(5):
        with Image.open(f / "overlay_prewarp" / "bear" / f"{t:05d}.jpg") as im:
            im.load()
            assert im.size == (200, 120)
    for d in ("eval", "overlay", "final", "eval_prewarp", "overlay_prewarp"):
        assert not (p / d).exists(), d
    for d in ("eval", "overlay", "final"):
        assert not (f / d).exists(), d
    assert not (p / "premvos_amd_davis_eval_prewarp.json").exists() and not (f / "premvos_amd_davis_eval.json").exists()
