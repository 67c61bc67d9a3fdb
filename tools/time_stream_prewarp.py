#!/usr/bin/env python
"""What `stream --track --prewarp` costs beside `stream --reid` (no merge) and `stream --track` (the live-warp loop in the process).

The job is that of tools/time_stream_track.build_job (synthetic 480x854 clip, object-like refinement weights, full-depth nets, a
first-frame annotation of 10 objects, the two `live` engine configurations).  Every program runs in a FRESH child process under its own
time limit: it builds its nets, runs the clip once untimed (plans, allocator), then once timed with a synchronise before each clock
read while a host thread samples the shader clock.  The sequence (reid, track, prewarp) is alternated twice in one call because boxes
differ by ~5 % in clock; a child that fails ends the call.

The condition, in the form of DESIGN.md 8.4: both `--prewarp` runs are above both `stream --track` runs by more than the two
`stream --track` runs differ from each other.  Recorded, not judged: how close the `--prewarp` runs come to `stream --reid`, how long
the tracker thread stood in front of an empty feed, how long the producer stood in front of a full one, the peak HBM.

    python tools/time_stream_prewarp.py [--frames 128] [--out profiles/stream_prewarp.json]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.time_stream_reid import CONFIG, IMAGES, WEIGHTS, _timed  # noqa: E402
from tools.time_stream_track import LIVE, build_job  # noqa: E402

PROGRAMS = {"reid": "stream --reid", "track": "stream --track", "prewarp": "stream --track --prewarp"}


def child(root: str, out: str, mode: str) -> dict:
    import torch
    from premvos_amd import stream
    os.chdir(root)
    warm = out.rstrip("/") + "_warm"
    final = "final_prewarp" if mode == "prewarp" else "final"
    track = None
    if mode != "reid":
        track = dict(LIVE, final=os.path.join(os.path.dirname(warm), final + "_warm"), anns="data/DAVIS/Annotations/480p",
                     **(stream._prewarp_options(None) if mode == "prewarp" else {}))
    pipe = stream.StreamPipeline(*WEIGHTS, batch=8, out=warm, reid_config=CONFIG, track=track)
    clip = [IMAGES + "clip0/"]
    n = pipe.run_sequences(clip)
    shutil.rmtree(warm)
    pipe.out = out
    if track:
        shutil.rmtree(track["final"])
        track["final"] = os.path.join(os.path.dirname(out), final)
    dt, n2, box = _timed(lambda: pipe.run_sequences(clip), pipe.dev.index)
    assert n == n2
    rep = {"program": PROGRAMS[mode], "frames": n, "seconds": round(dt, 4), "frames_per_s": round(n / dt, 2), "box": box,
           "peak_hbm_gb_torch_allocator": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}
    if track:
        rep["producer_waited_on_full_feed_s"] = round(pipe.track_feed_waited_s, 4)
        rep["final_pngs"] = sum(len(fs) for _, _, fs in os.walk(track["final"]))
    if mode == "prewarp":
        rep["tracker_waited_on_empty_feed_s"] = round(pipe.track_prewarp_stats["waited_s"], 4)
    return rep


def run_child(args: list, limit: int) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"time_stream_prewarp: child {args} ended with {r.returncode}; nothing more is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"time_stream_prewarp: {rep['program']}: {rep['frames']} frames in {rep['seconds']} s", file=sys.stderr, flush=True)
    return rep


def condition(track_fps: list, prewarp_fps: list) -> dict:
    """8.4's rule: the slower --prewarp run exceeds the faster --track run by more than the --track runs differ from each other"""
    spread = max(track_fps) - min(track_fps)
    margin = min(prewarp_fps) - max(track_fps)
    return {"track_runs_differ_by": round(spread, 2), "slowest_prewarp_minus_fastest_track": round(margin, 2), "holds": bool(margin > spread)}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_prewarp.json"))
    ap.add_argument("--child", default=None, choices=sorted(PROGRAMS))
    ap.add_argument("--root", default=None)
    ap.add_argument("--inter", default=None)
    return ap.parse_args(argv)


def main() -> int:
    a = parse_args()
    if a.child:
        print(json.dumps(child(a.root, a.inter, a.child)))
        return 0
    root = tempfile.mkdtemp(prefix="premvos_stream_prewarp_")
    try:
        build_job(root, a.frames, a.objects)
        rep = {"what": "tools/time_stream_prewarp.py: a synthetic 480x854 clip through stream --reid, stream --track and stream --track "
                       "--prewarp; every program in a fresh process, one warm-up pass, one timed pass, the sequence alternated",
               "frames": a.frames, "objects": a.objects, "alternations": []}
        for k in range(a.alternations):
            runs = {}
            for mode in ("reid", "track", "prewarp"):
                inter = os.path.join(root, f"{mode}{k}", "intermediate")
                runs[mode] = run_child(["--child", mode, "--root", root, "--inter", inter], a.limit)
                shutil.rmtree(os.path.dirname(inter))
            rep["alternations"].append(runs)
        fps = {m: [x[m]["frames_per_s"] for x in rep["alternations"]] for m in PROGRAMS}
        rep["frames_per_s"] = fps
        rep["condition_prewarp_above_track"] = condition(fps["track"], fps["prewarp"])
        rep["prewarp_over_reid"] = [round(p / r, 3) for p, r in zip(fps["prewarp"], fps["reid"])]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())
