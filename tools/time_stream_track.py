#!/usr/bin/env python
"""What it costs to get output/final/<video>/<frame>.png from JPEGs: two programs, or one.

    leg 1  `premvos_amd.stream --reid`, then `premvos_amd.track` on its tree -- the two-program way: the second program parses the JSON
           the first one dumped, turns every COCO string back into run boundaries, decodes them, reads the .flo files and decodes
           every JPEG again
    leg 2  `premvos_amd.stream --track`: the merge loop runs inside the streaming driver on the arrays it has in HBM

The job is that of tools/time_stream_reid.build_job (synthetic 480x854 clip, object-like refinement weights, full-depth nets) plus a
first-frame annotation of 10 objects and the two `live` engine configurations.  Every program runs in a FRESH child process under its
own time limit: it builds its nets, runs the clip once untimed (plans, allocator), then once timed with a synchronise before each
clock read while a host thread samples the shader clock.  The legs are alternated (1, 2, 1, 2) in one call because boxes differ by
~5 % in clock; a child that fails ends the call.  The condition: leg 2 takes less wall time than the sum of leg 1's two programs in
BOTH alternations.  Recorded, not judged: plain `stream` frames/s twice, `stream --track` frames/s, the tracker thread's per-phase
split inside the stream (a third, instrumented pass: a synchronise of the tracker's stream per phase), how long the producer waited on
a full feed, and the process's peak HBM with and without the flag.

    python tools/time_stream_track.py [--frames 128] [--out profiles/stream_track.json]
"""
from __future__ import annotations

import argparse
import glob
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

from tools.time_stream_reid import CONFIG, IMAGES, WEIGHTS, _timed  # noqa: E402

LIVE = {"refinement_config": "code/refinement_net/configs/live", "reid_config": "code/ReID_net/configs/live"}
PHASES = ("inputs", "overlap", "scores", "paint", "warp", "boxes+reid", "refine")


def build_job(root: str, n_frames: int, objects: int = 10) -> None:
    """time_stream_reid.build_job + the two `live` configs + a first-frame annotation of ``objects`` ellipses.  Host only."""
    import numpy as np
    from tools import time_stream_reid
    from premvos_amd.track import write_png
    time_stream_reid.build_job(root, n_frames)
    os.makedirs(os.path.join(root, "code", "refinement_net", "configs"))
    with open(os.path.join(root, LIVE["refinement_config"]), "w") as f:
        json.dump({"model": "live", "load": "../weights/refine.pt"}, f)
    with open(os.path.join(root, LIVE["reid_config"]), "w") as f:
        json.dump({"model": "Re-ID", "load": "../weights/reid.pt", "input_size": [128, 128]}, f)
    H, W = 480, 854
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ann = np.zeros((H, W), np.uint8)
    for i in range(objects):
        cy, cx = 110 + 250 * (i // 5), 100 + 160 * (i % 5)
        ann[((yy - cy) / (60 + 4 * i)) ** 2 + ((xx - cx) / (55 + 2 * i)) ** 2 <= 1] = i + 1
    write_png(os.path.join(root, "data", "DAVIS", "Annotations", "480p", "clip0", "00000.png"), ann)


def _peak_gb() -> float:
    import torch
    return round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)


def child_stream(root: str, out: str, mode: str) -> dict:
    """``mode``: plain | reid | track."""
    import torch
    from premvos_amd import stream
    os.chdir(root)
    warm = out.rstrip("/") + "_warm"
    track = dict(LIVE, final=os.path.join(os.path.dirname(warm), "final_warm"), anns="data/DAVIS/Annotations/480p") if mode == "track" else None
    pipe = stream.StreamPipeline(*WEIGHTS, batch=8, out=warm, reid_config=CONFIG if mode != "plain" else None, track=track)
    clip = [IMAGES + "clip0/"]
    n = pipe.run_sequences(clip)
    shutil.rmtree(warm)
    pipe.out = out
    if track:
        shutil.rmtree(track["final"])
        track["final"] = os.path.join(os.path.dirname(out), "final")
    dt, n2, box = _timed(lambda: pipe.run_sequences(clip), pipe.dev.index)
    assert n == n2
    rep = {"program": {"plain": "stream", "reid": "stream --reid", "track": "stream --track"}[mode], "frames": n, "seconds": round(dt, 4),
           "frames_per_s": round(n / dt, 2), "box": box, "peak_hbm_gb_torch_allocator": _peak_gb()}
    if track:
        rep["producer_waited_on_full_feed_s"] = round(pipe.track_feed_waited_s, 4)
        # the tracker thread's phases: a third pass with a synchronise of ITS stream at the end of every phase (slower by design)
        phases, clock, st = {k: 0.0 for k in PHASES}, [0.0], pipe.streams["track"]

        def tick(name):
            st.synchronize()
            now = time.perf_counter()
            phases[name] += now - clock[0]
            clock[0] = now
        pipe.track_timer = tick
        pipe.out, track["final"] = warm, os.path.join(os.path.dirname(warm), "final_warm")
        # (the clock restarts when a step begins: `inputs` would otherwise include the wait for the chunk)
        from premvos_amd import track as tk
        step = tk.Tracker.step_resident

        def timed_step(self, *a, **kw):
            st.synchronize()
            clock[0] = time.perf_counter()
            return step(self, *a, **kw)
        tk.Tracker.step_resident = timed_step
        try:
            pipe.run_sequences(clip)
        finally:
            tk.Tracker.step_resident, pipe.track_timer = step, None
        shutil.rmtree(warm)
        shutil.rmtree(track["final"])
        rep["tracker_phase_ms_per_frame_with_syncs"] = {k: round(1e3 * v / max(n - 1, 1), 3) for k, v in phases.items()}
    return rep


def child_track(root: str, inter: str) -> dict:
    """The second program of leg 1: premvos_amd.track's own main loop on the tree under ``inter`` (engines as track.main builds them)."""
    from premvos_amd import _lib, track
    from premvos_amd import io_pipeline as iop
    from premvos_amd.refinement.driver import refinement_net_init
    from premvos_amd.reid.driver import ReID_net_init
    os.chdir(os.path.join(root, "code"))
    refinement_net, ReID_net = refinement_net_init(), ReID_net_init()
    os.chdir(root)
    lay = track._layout(root)
    lay["props"], lay["flows"] = os.path.join(inter, "ReID_proposals") + "/", os.path.join(inter, "flow") + "/"
    video = os.path.join(lay["images"], "clip0") + "/"

    def run(out):
        with iop.Writer() as writer:
            return len(track.do_video(video, lay["images"], lay["anns"], lay["props"], lay["flows"], out, refinement_net, ReID_net, writer=writer))
    warm = os.path.join(os.path.dirname(inter.rstrip("/")), "final_warm") + "/"
    n = run(warm)
    shutil.rmtree(warm)
    dt, n2, box = _timed(lambda: run(os.path.join(os.path.dirname(inter.rstrip("/")), "final") + "/"), _lib.resolve_device().index)
    assert n == n2
    return {"program": "track", "frames": n, "seconds": round(dt, 4), "frames_per_s": round(n / dt, 2), "box": box,
            "peak_hbm_gb_torch_allocator": _peak_gb()}


def compare_finals(a: str, b: str) -> dict:
    fa = sorted(glob.glob(os.path.join(a, "*", "*.png")))
    same = [open(f, "rb").read() == open(os.path.join(b, os.path.relpath(f, a)), "rb").read() for f in fa]
    return {"pngs": len(fa), "identical": int(sum(same))}


def objects_alive(final: str) -> int:
    import numpy as np
    from PIL import Image
    last = sorted(glob.glob(os.path.join(final, "clip0", "*.png")))[-1]
    return int(len(set(np.unique(np.array(Image.open(last))).tolist()) - {0}))


def run_child(args: list, limit: int) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"time_stream_track: child {args} ended with {r.returncode}; nothing more is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"time_stream_track: {rep['program']}: {rep['frames']} frames in {rep['seconds']} s", file=sys.stderr, flush=True)
    return rep


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_track.json"))
    ap.add_argument("--child", default=None, choices=["plain", "reid", "track", "track_program"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--inter", default=None)
    return ap.parse_args(argv)


def main() -> int:
    a = parse_args()
    if a.child:
        rep = child_track(a.root, a.inter) if a.child == "track_program" else child_stream(a.root, a.inter, a.child)
        print(json.dumps(rep))
        return 0
    root = tempfile.mkdtemp(prefix="premvos_stream_track_")
    try:
        build_job(root, a.frames, a.objects)
        rep = {"what": "tools/time_stream_track.py: output/final/ of a synthetic 480x854 clip by two programs (stream --reid, then track) and "
                       "by one (stream --track); every program in a fresh process, one warm-up pass, one timed pass, legs alternated",
               "frames": a.frames, "objects": a.objects, "alternations": [], "stream_without_flags": []}
        for k in range(a.alternations):
            two, one, plain = (os.path.join(root, f"{tag}{k}", "intermediate") for tag in ("two", "one", "plain"))
            p = run_child(["--child", "plain", "--root", root, "--inter", plain], a.limit)
            s = run_child(["--child", "reid", "--root", root, "--inter", two], a.limit)
            q = run_child(["--child", "track_program", "--root", root, "--inter", two], a.limit)
            r = run_child(["--child", "track", "--root", root, "--inter", one], a.limit)
            total = round(s["seconds"] + q["seconds"], 4)
            fin2, fin1 = os.path.join(os.path.dirname(two), "final"), os.path.join(os.path.dirname(one), "final")
            rep["stream_without_flags"].append(p)
            rep["alternations"].append({
                "leg1_two_programs": {"stream_reid": s, "track": q, "seconds": total, "frames_per_s": round(a.frames / total, 2)},
                "leg2_one_program": r, "leg2_over_leg1_seconds": round(r["seconds"] / total, 3), "leg2_faster": bool(r["seconds"] < total),
                "final_pngs": compare_finals(fin2, fin1), "objects_with_pixels_in_the_last_frame": objects_alive(fin2)})
            for d in (two, one, plain):
                shutil.rmtree(os.path.dirname(d))
        rep["condition_leg2_faster_in_every_alternation"] = all(x["leg2_faster"] for x in rep["alternations"])
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())
