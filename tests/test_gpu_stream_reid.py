"""`python -m premvos_amd.stream --reid`: stage E inside the streaming driver.  The tree it writes under ReID_proposals/ is the one
premvos_amd.reid.driver.forward_directory writes from refined_proposals/ (same files, same keys, embeddings within the 1e-3 bar of
tests/test_gpu_reid.py), every other directory keeps its bytes, and premvos_amd.track accepts the result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import reid_oracle as QO  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_reid_tree as T  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER = ("flow", "general_proposals", "specific_proposals", "combined_proposals", "refined_proposals")


def _files(base):
    return sorted(str(p.relative_to(base)) for p in base.rglob("*") if p.is_file())


def _run(root, *extra):
    from premvos_amd import stream
    cwd = os.getcwd()
    try:
        assert stream.main(["--root", str(root), "--batch", "2"] + T.STREAM_ARGS + list(extra)) == 0
    finally:
        os.chdir(cwd)
    return root / "output" / "intermediate"


def test_reid_tree_of_the_streaming_driver(tmp_path, monkeypatch):
    from premvos_amd import rle
    from premvos_amd.reid import forward_directory
    monkeypatch.setenv("PREMVOS_DRIVER_BATCH", "2")
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    roots = {}
    for tag in ("plain", "reid", "again"):
        (tmp_path / tag).mkdir()
        frames = T.make_tree(tmp_path / tag)
        roots[tag] = _run(tmp_path / tag, *(() if tag == "plain" else ("--reid",)))
    plain, reid, again = roots["plain"], roots["reid"], roots["again"]
    # without the flag: no new directory; with it: every other directory keeps its bytes
    assert sorted(os.listdir(plain)) == sorted(OTHER) and sorted(os.listdir(reid)) == sorted(OTHER + ("ReID_proposals",))
    assert _files(plain) == [f for f in _files(reid) if not f.startswith("ReID_proposals")] and len(_files(plain)) == 4 + 4 * 5
    for f in _files(plain):
        assert (plain / f).read_bytes() == (reid / f).read_bytes(), f
    assert "reid" not in json.load(open(tmp_path / "plain" / "output" / "premvos_amd_manifest.json"))
    assert json.load(open(tmp_path / "reid" / "output" / "premvos_amd_manifest.json"))["reid"]["config"] == "code/ReID_net/configs/run"
    # a second run: the same bytes
    assert _files(again) == _files(reid)
    for f in _files(reid):
        assert (again / f).read_bytes() == (reid / f).read_bytes(), f
    # the files themselves
    per_frame = []
    for t in range(5):
        raw = (reid / "ReID_proposals" / "bear" / f"{t:05d}.json").read_text()
        q = json.loads(raw)
        assert json.dumps(q) == raw                                                # a later load / dump reproduces the file
        stripped = [{k: v for k, v in p.items() if k != "ReID"} for p in q]
        assert json.dumps(stripped) == (reid / "refined_proposals" / "bear" / f"{t:05d}.json").read_text()
        n = 0
        for p in q:
            bb = rle.to_bbox(p["segmentation"])
            assert ("ReID" in p) == (bb[2] > 0 and bb[3] > 0)
            if "ReID" in p:
                assert list(p)[-1] == "ReID" and len(p["ReID"]) == 128 and np.isfinite(p["ReID"]).all()
                n += 1
        per_frame.append(n)
    print("proposals with an embedding per frame:", per_frame)
    assert min(per_frame) >= 1 and sum(per_frame) >= 10, per_frame
    # the stage driver on the same refined proposals: the same keys, embeddings within the bar
    eng = T.reid_engine(tmp_path / "reid")
    two = tmp_path / "two_programs"
    assert forward_directory(eng, str(tmp_path / "reid" / "data" / "DAVIS" / "JPEGImages" / "480p") + "/",
                             str(reid / "refined_proposals") + "/", str(two) + "/") == 5
    assert _files(two) == [f[len("ReID_proposals/"):] for f in _files(reid) if f.startswith("ReID_proposals")]
    worst = 0.0
    for t in range(5):
        a = json.load(open(reid / "ReID_proposals" / "bear" / f"{t:05d}.json"))
        b = json.load(open(two / "bear" / f"{t:05d}.json"))
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert list(x) == list(y) and {k: v for k, v in x.items() if k != "ReID"} == {k: v for k, v in y.items() if k != "ReID"}
            if "ReID" in x:
                d = np.abs(np.array(x["ReID"]) - np.array(y["ReID"])).max()
                worst = max(worst, d / max(1.0, np.abs(y["ReID"]).max()))
                assert d < 1e-3 * max(1.0, np.abs(y["ReID"]).max())
    print("streaming vs stage driver, worst relative embedding difference:", worst)
    # the CPU oracle on the first two embeddings of frame 0
    q0 = json.load(open(reid / "ReID_proposals" / "bear" / "00000.json"))
    have = [p for p in q0 if "ReID" in p][:2]
    assert have
    cb = QO.context_boxes([rle.to_bbox(p["segmentation"]) for p in have], 120, 200, feed=False)
    ref = QO.forward(QO.synth_weights(0, T.REID_UNITS), np.stack([QO.make_crop(frames[0], b, feed=False) for b in cb]), T.REID_UNITS)
    for p, e in zip(have, ref):
        assert np.abs(np.array(p["ReID"]) - e).max() < 1e-3 * max(1.0, np.abs(ref).max())
    # the merge stage accepts the tree once its engine configurations exist
    for net in ("refinement_net", "ReID_net"):
        d = tmp_path / "reid" / "code" / net / "configs"
        d.mkdir(parents=True, exist_ok=True)
        (d / "live").write_text(json.dumps({"load": "../weights/none"}))
    r = subprocess.run([sys.executable, "-m", "premvos_amd.track", "--root", str(tmp_path / "reid"), "--check-only"],
                       capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO), timeout=300)
    assert r.returncode == 0 and "inputs are in place" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_refusals_write_nothing(tmp_path, monkeypatch):
    from premvos_amd import stream
    T.make_tree(tmp_path, t=2)
    cwd = os.getcwd()
    try:
        with pytest.raises(SystemExit) as e:
            stream.main(["--root", str(tmp_path), "--reid", "--gather"] + T.STREAM_ARGS)
        assert "--reid" in str(e.value) and "--gather" in str(e.value)
        monkeypatch.setenv("PREMVOS_SIDECAR", "1")
        with pytest.raises(SystemExit) as e:
            stream.main(["--root", str(tmp_path), "--reid"] + T.STREAM_ARGS)
        assert "--reid" in str(e.value) and "PREMVOS_SIDECAR=1" in str(e.value)
    finally:
        os.chdir(cwd)
    assert not (tmp_path / "output").exists()


def _stream_subprocess(root, *extra, gpus=1):
    """A FRESH process (or two ranks of them, sharing the test box's one GPU over gloo -- RCCL needs a device per rank)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "PREMVOS_SIDECAR")}
    env.update({"PREMVOS_DIST_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "PYTHONPATH": REPO})
    r = subprocess.run([sys.executable, "-m", "premvos_amd.stream", "--root", str(root), "--gpus", str(gpus)] + T.STREAM_ARGS + list(extra),
                       capture_output=True, text=True, env=env, timeout=1500, cwd=REPO)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_two_ranks_write_the_one_rank_tree_with_reid(tmp_path):
    roots = []
    for tag, gpus in (("one", 1), ("two", 2)):
        root = tmp_path / tag
        root.mkdir()
        T.make_tree(root, videos={"bear": 4, "camel": 3})
        out = _stream_subprocess(root, "--batch", "2", "--reid", gpus=gpus)
        assert "frames: 7" in out
        roots.append(root / "output" / "intermediate")
    fa, fb = _files(roots[0]), _files(roots[1])
    assert fa == fb and len(fa) == (3 + 2) + 5 * 7
    assert sum(f.startswith("ReID_proposals") for f in fa) == 7
    for f in fa:
        assert (roots[0] / f).read_bytes() == (roots[1] / f).read_bytes(), f
    assert any('"ReID"' in (roots[0] / f).read_text() for f in fa if f.startswith("ReID_proposals"))
