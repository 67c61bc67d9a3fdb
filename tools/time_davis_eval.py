#!/usr/bin/env python
"""What the DAVIS measures cost on the GPU (premvos_amd.evaluate, premvos_davis_counts_u8) against the host (tools/davis_eval.py).

    1  the kernel: a 64-frame 480x854 clip of blob masks in HBM, T = 3 and T = 10 objects, and a 1080x1920 leg (radius 18):
       ms per frame when every frame is its own launch (what the merge loop does) and ms per video launch (what evaluate() does)
    2  premvos_amd.evaluate.evaluate() end to end on the PNG tree of that clip, PNG decode included, in frames/s
    3  tools/davis_eval.evaluate on the same box and the same tree (its first --host-frames frames: the host is linear in frames and
       takes minutes on the whole clip); without scipy the numpy restatement of tests/davis_restated.py runs and the report says so
    4  inside the merge loop: tools/time_stream_track.py's job with an annotation for EVERY frame, `stream --track` without and with
       --eval, alternated twice, every program in a fresh child process (one warm-up pass, one timed pass between synchronises)

Conditions: (2) beats (3) on every leg (the ratio is reported); the frames/s of `--track --eval` lie within twice the spread between
the two runs without --eval of the same call.  Every GPU program is a child process under its own time limit; a child that fails
ends the call.

    python tools/time_davis_eval.py [--frames 64] [--loop-frames 64] [--out profiles/davis_eval.json]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEGS = (("480p_T3", 480, 854, 3), ("480p_T10", 480, 854, 10), ("1080p_T3", 1080, 1920, 3))


def blob_clip(h: int, w: int, objects: int, frames: int, seed: int = 0):
    """(results, annotations) uint8 [frames,h,w]: ``objects`` ellipses drifting over the clip; the result is the annotation moved by a
    few pixels with a changed radius -- J around 0.8, contours partly within the tolerance."""
    import numpy as np
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    cy, cx = rng.uniform(0.15 * h, 0.85 * h, objects), rng.uniform(0.1 * w, 0.9 * w, objects)
    ry, rx = rng.uniform(0.06 * h, 0.16 * h, objects), rng.uniform(0.04 * w, 0.1 * w, objects)
    vy, vx = rng.uniform(-1.5, 1.5, objects), rng.uniform(-2.5, 2.5, objects)
    res, gt = np.zeros((frames, h, w), np.uint8), np.zeros((frames, h, w), np.uint8)
    for k in range(frames):
        for i in range(objects):
            y, x = cy[i] + vy[i] * k, cx[i] + vx[i] * k
            gt[k][((yy - y) / ry[i]) ** 2 + ((xx - x) / rx[i]) ** 2 <= 1] = i + 1
            dy, dx = rng.uniform(-4, 4, 2)
            res[k][((yy - y - dy) / (ry[i] * rng.uniform(0.9, 1.1))) ** 2 + ((xx - x - dx) / (rx[i] * rng.uniform(0.9, 1.1))) ** 2 <= 1] = i + 1
    return res, gt


def write_tree(root: str, name: str, res, gt) -> None:
    from premvos_amd.track import write_png
    for k in range(len(gt)):
        write_png(os.path.join(root, "annotations", name, f"{k:05d}.png"), gt[k])
        write_png(os.path.join(root, "results", name, f"{k:05d}.png"), res[k])


def host_evaluator():
    """-> (name, evaluate(results_root, annotations_root, sequences)) of the host yardstick that can run here."""
    try:
        import scipy  # noqa: F401
        from tools import davis_eval
        return "tools/davis_eval.py (scipy.ndimage.binary_dilation)", davis_eval.evaluate
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import davis_restated
        return "tests/davis_restated.py (numpy restatement: scipy is not installed)", davis_restated.evaluate


def child_kernel(root: str, frames: int, host_frames: int) -> dict:
    """Items 1-3 in one process."""
    import numpy as np
    import torch
    from premvos_amd import _lib
    from premvos_amd import evaluate as ev
    dev = _lib.resolve_device()
    host_name, host_eval = host_evaluator()
    rep = {"host_evaluator": host_name, "legs": {}}
    for name, h, w, T in LEGS:
        n = frames if h == 480 else max(4, frames // 8)
        res, gt = blob_clip(h, w, T, n)
        write_tree(root, name, res, gt)
        ids = list(range(1, T + 1))
        rd, gd = torch.from_numpy(res[1:-1]).to(dev), torch.from_numpy(gt[1:-1]).to(dev)
        N = rd.shape[0]
        seq = ev.SequenceEval(ids, [str(k) for k in range(N)])

        def per_frame():
            for k in range(N):
                seq.add(k, rd[k], gd[k])

        def timed(fn, reps=5):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps
        ms_video = timed(lambda: ev.davis_counts(rd, gd, ids))
        ms_frames = timed(per_frame)
        assert torch.equal(seq.counts, ev.davis_counts(rd, gd, ids))
        results, anns = os.path.join(root, "results"), os.path.join(root, "annotations")
        ev.evaluate(results, anns, [name])                              # (the pool's threads, the library: once untimed)
        t = time.perf_counter()
        got = ev.evaluate(results, anns, [name])
        gpu_s = time.perf_counter() - t
        # the host on the first `host_frames` evaluated frames of the same tree
        m = min(host_frames if h == 480 else 2, N)                      # (a 1080p object-frame takes the host seconds)
        for sub in ("results", "annotations"):
            os.makedirs(os.path.join(root, "host", sub, name))
            for k in range(m + 2):
                shutil.copy(os.path.join(root, sub, name, f"{k:05d}.png"), os.path.join(root, "host", sub, name, f"{k:05d}.png"))
        t = time.perf_counter()
        want = host_eval(os.path.join(root, "host", "results"), os.path.join(root, "host", "annotations"), [name])
        host_s = time.perf_counter() - t
        same = ev.evaluate(os.path.join(root, "host", "results"), os.path.join(root, "host", "annotations"), [name]) == want
        rep["legs"][name] = {
            "h": h, "w": w, "objects": T, "radius": ev.bound_pix(h, w), "evaluated_frames": N,
            "kernel_ms_per_frame_one_launch_per_frame": round(ms_frames / N, 4), "kernel_ms_per_video_launch": round(ms_video, 4),
            "kernel_ms_per_frame_in_the_video_launch": round(ms_video / N, 4),
            "evaluate_gpu_seconds": round(gpu_s, 4), "evaluate_gpu_frames_per_s": round(N / gpu_s, 2),
            "host_frames": m, "host_seconds": round(host_s, 3), "host_frames_per_s": round(m / host_s, 3),
            "host_ms_per_object_frame": round(1e3 * host_s / (m * T), 2),
            "gpu_over_host": round((N / gpu_s) / (m / host_s), 1), "gpu_faster": bool(N / gpu_s > m / host_s),
            "same_dict_as_the_host_on_its_frames": bool(same), "mean_J": got["mean_J"], "mean_F": got["mean_F"]}
        print(f"time_davis_eval: {name}: {rep['legs'][name]}", file=sys.stderr, flush=True)
    return rep


def build_loop_job(root: str, n_frames: int, objects: int) -> None:
    """tools/time_stream_track.build_job + an annotation for every frame (the first frame's ellipses, drifting)."""
    import numpy as np
    from PIL import Image
    from premvos_amd.track import write_png
    from tools import time_stream_track as TT
    TT.build_job(root, n_frames, objects)
    d = os.path.join(root, "data", "DAVIS", "Annotations", "480p", "clip0")
    first = np.array(Image.open(os.path.join(d, "00000.png")))
    for k in range(1, n_frames):
        write_png(os.path.join(d, f"{k:05d}.png"), np.roll(first, (k // 8, k // 4), (0, 1)))


def child_loop(root: str, out: str, evaluate: bool) -> dict:
    """`stream --track` [--eval] on the loop job: one untimed pass, one timed pass."""
    from premvos_amd import stream
    from tools.time_stream_reid import CONFIG, IMAGES, WEIGHTS, _timed
    from tools.time_stream_track import LIVE
    os.chdir(root)
    base = os.path.dirname(out.rstrip("/"))
    track = dict(LIVE, final=os.path.join(base, "final_warm"), anns="data/DAVIS/Annotations/480p",
                 eval=os.path.join(base, "eval_warm") if evaluate else None)
    pipe = stream.StreamPipeline(*WEIGHTS, batch=8, out=out.rstrip("/") + "_warm", reid_config=CONFIG, track=track)
    clip = [IMAGES + "clip0/"]
    n = pipe.run_sequences(clip)
    pipe.out, track["final"] = out, os.path.join(base, "final")
    if evaluate:
        track["eval"] = os.path.join(base, "eval")
    dt, n2, box = _timed(lambda: pipe.run_sequences(clip), pipe.dev.index)
    assert n == n2
    rep = {"program": "stream --track --eval" if evaluate else "stream --track", "frames": n, "seconds": round(dt, 4),
           "frames_per_s": round(n / dt, 2), "box": box}
    if evaluate:
        from premvos_amd import evaluate as ev
        r = ev.summarise(track["eval"])
        rep.update({"mean_J": r["mean_J"], "mean_F": r["mean_F"], "objects": r["objects"],
                    "equals_evaluate_on_the_pngs": bool(r == ev.evaluate(track["final"], track["anns"], ["clip0"]))})
    return rep


def run_child(args: list, limit: int) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    sys.stderr.write(r.stderr[-2000:])
    if r.returncode != 0:
        raise SystemExit(f"time_davis_eval: child {args} ended with {r.returncode}; nothing more is started\n{r.stdout[-1500:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frames of the evaluator's clip (the first and last are not evaluated)")
    ap.add_argument("--host-frames", type=int, default=6, help="evaluated frames the host yardstick is timed on")
    ap.add_argument("--loop-frames", type=int, default=64, help="frames of the merge loop's clip; 0 = skip item 4")
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "davis_eval.json"))
    ap.add_argument("--child", default=None, choices=["kernel", "loop", "loop_eval"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--inter", default=None)
    return ap.parse_args(argv)


def loop_condition(plain: list, with_eval: list) -> dict:
    """The frames/s of the runs with --eval against the spread of the runs without it (host only)."""
    mean = sum(plain) / len(plain)
    spread = max(plain) - min(plain)
    worst = max(abs(v - mean) for v in with_eval)
    return {"frames_per_s_without_eval": plain, "frames_per_s_with_eval": with_eval, "spread_without_eval": round(spread, 3),
            "spread_without_eval_percent": round(100 * spread / mean, 2), "largest_distance_with_eval": round(worst, 3),
            "cost_percent_of_mean": round(100 * (mean - sum(with_eval) / len(with_eval)) / mean, 2),
            "within_twice_the_spread": bool(worst <= 2 * spread)}


def main() -> int:
    a = parse_args()
    if a.child:
        rep = child_kernel(a.root, a.frames, a.host_frames) if a.child == "kernel" else child_loop(a.root, a.inter, a.child == "loop_eval")
        print(json.dumps(rep))
        return 0
    rep = {"what": "tools/time_davis_eval.py: the DAVIS measures on the GPU (premvos_amd.evaluate) against the host yardstick, and the cost "
                   "of --eval inside stream --track; every GPU program in a fresh child process", "frames": a.frames}
    root = tempfile.mkdtemp(prefix="premvos_davis_eval_")
    try:
        rep.update(run_child(["--child", "kernel", "--root", root, "--frames", str(a.frames), "--host-frames", str(a.host_frames)], a.limit))
        rep["condition_gpu_faster_than_host_on_every_leg"] = all(v["gpu_faster"] for v in rep["legs"].values())
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.loop_frames:
        root = tempfile.mkdtemp(prefix="premvos_davis_loop_")
        try:
            build_loop_job(root, a.loop_frames, a.objects)
            runs = []
            for k in range(a.alternations):
                for mode in ("loop", "loop_eval"):
                    inter = os.path.join(root, f"{mode}{k}", "intermediate")
                    runs.append(run_child(["--child", mode, "--root", root, "--inter", inter], a.limit))
                    print(f"time_davis_eval: {runs[-1]['program']}: {runs[-1]['frames_per_s']} frames/s", file=sys.stderr, flush=True)
                    shutil.rmtree(os.path.dirname(inter))
            rep["in_loop"] = dict(loop_condition([r["frames_per_s"] for r in runs if "eval" not in r["program"]],
                                                 [r["frames_per_s"] for r in runs if "eval" in r["program"]]),
                                  frames=a.loop_frames, objects=a.objects, runs=runs)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())
