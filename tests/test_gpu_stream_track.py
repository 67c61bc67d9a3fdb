"""`python -m premvos_amd.stream --track`: frames in, final DAVIS PNGs out, one process per GPU.  The yardstick is the two-program
path -- `stream --reid`, then `premvos_amd.track` on the tree it wrote -- and the bar is equality of every file under
output/intermediate/ and output/final/.  Every program runs in a fresh child process under its own time limit."""
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


def _tree(root, videos, annotate="bear"):
    """The synthetic tree of the --reid tests + the two `live` engine configurations MergeTrack loads + a first-frame annotation for
    ``annotate`` with two objects whose ids are not adjacent (as tests/test_gpu_track.py's command test), none for the others."""
    root.mkdir()
    T.make_tree(root, videos=videos)
    (root / "code" / "refinement_net" / "configs").mkdir(parents=True)
    (root / "code" / "refinement_net" / "configs" / "live").write_text(json.dumps({"model": "live", "load": "../weights/refinement_specific_weights"}))
    (root / "code" / "ReID_net" / "configs" / "live").write_text(json.dumps(
        {"model": "Re-ID", "load": "../weights/ReID_general_weights", "input_size": [128, 128], "network": T.REID_NETWORK}))
    ann = np.zeros((120, 200), np.uint8)
    ann[20:70, 30:90] = 1
    ann[60:110, 120:180] = 3
    if annotate:
        d = root / "data" / "DAVIS" / "Annotations" / "480p" / annotate
        d.mkdir(parents=True)
        R.write_index_png(str(d / "00000.png"), ann)
    return ann


def _child(module, root, *extra, gpus=None, timeout=900, check=True):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "PREMVOS_SIDECAR")}
    env.update({"PREMVOS_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "PYTHONPATH": REPO, "PREMVOS_DRIVER_BATCH": "2",
                "PREMVOS_STREAM_REFINE_LANES": "2"})
    cmd = [sys.executable, "-m", module, "--root", str(root)] + (["--gpus", str(gpus)] if gpus else []) + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=REPO)
    if check:
        assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-3000:])
    return r


def _png(fn):
    from PIL import Image
    return np.array(Image.open(fn))


def test_one_command_writes_the_tree_and_the_pngs_of_the_two_program_path(tmp_path):
    """Copy A: `stream --reid`, then `track`.  Copy B: `stream --track`.  'bear' (5 frames, 2 annotated objects) crosses chunk
    (--batch 2), launch (PREMVOS_DRIVER_BATCH=2) and lane (2 lanes) boundaries; 'camel' (3 frames) has no annotation.
    Non-vacuity is judged on copy A: an annotated object still has pixels in bear's last frame."""
    videos = {"bear": 5, "camel": 3}
    ann = _tree(tmp_path / "a", videos)
    _tree(tmp_path / "b", videos)
    _child("premvos_amd.stream", tmp_path / "a", "--batch", "2", "--reid", *T.STREAM_ARGS)
    _child("premvos_amd.track", tmp_path / "a")
    out = _child("premvos_amd.stream", tmp_path / "b", "--batch", "2", "--track", *T.STREAM_ARGS).stdout
    assert "frames: 8" in out
    a, b = tmp_path / "a" / "output", tmp_path / "b" / "output"
    for sub in ("intermediate", "final"):
        fa, fb = _files(a / sub), _files(b / sub)
        assert fa == fb, sub
        for f in fa:
            assert (a / sub / f).read_bytes() == (b / sub / f).read_bytes(), (sub, f)
    assert _files(a / "final") == [f"bear/{t:05d}.png" for t in range(5)] + [f"camel/{t:05d}.png" for t in range(3)]
    assert sum(f.startswith("ReID_proposals") for f in _files(b / "intermediate")) == 8
    for t in range(3):
        assert not _png(a / "final" / "camel" / f"{t:05d}.png").any()
    assert np.array_equal(_png(a / "final" / "bear" / "00000.png"), ann)
    last = _png(a / "final" / "bear" / "00004.png")
    per_frame = [{int(i): int((_png(a / "final" / "bear" / f"{t:05d}.png") == i).sum()) for i in (1, 3)} for t in range(5)]
    print("copy A, pixels per annotated object and frame:", per_frame)
    assert set(np.unique(last)) <= {0, 1, 3} and ((last == 1).any() or (last == 3).any()), per_frame
    man_a = json.load(open(a / "premvos_amd_manifest.json"))
    man_b = json.load(open(b / "premvos_amd_manifest.json"))
    assert "track" not in man_a and man_b["track"] == {"refinement_config": "code/refinement_net/configs/live",
                                                       "reid_config": "code/ReID_net/configs/live", "output": "output/final"}
    assert man_b["reid"] == man_a["reid"]


def test_two_ranks_write_the_one_rank_bytes_and_one_video_on_two_ranks_is_refused(tmp_path):
    videos = {"bear": 4, "camel": 3}
    roots = []
    for tag, gpus in (("one", 1), ("two", 2)):
        _tree(tmp_path / tag, videos)
        out = _child("premvos_amd.stream", tmp_path / tag, "--batch", "2", "--track", *T.STREAM_ARGS, gpus=gpus, timeout=1500).stdout
        assert "frames: 7" in out
        roots.append(tmp_path / tag / "output")
    for sub in ("intermediate", "final"):
        fa, fb = _files(roots[0] / sub), _files(roots[1] / sub)
        assert fa == fb and len(fa) == ((3 + 2) + 5 * 7 if sub == "intermediate" else 7), (sub, fa)
        for f in fa:
            assert (roots[0] / sub / f).read_bytes() == (roots[1] / sub / f).read_bytes(), (sub, f)
    assert any(_png(roots[0] / "final" / "bear" / f"{t:05d}.png").any() for t in range(4))
    _tree(tmp_path / "single", {"bear": 4})
    r = _child("premvos_amd.stream", tmp_path / "single", "--batch", "2", "--track", *T.STREAM_ARGS, gpus=2, check=False)
    assert r.returncode != 0 and "whole videos" in r.stderr, (r.stdout[-500:], r.stderr[-1500:])
    assert not (tmp_path / "single" / "output").exists()
