#!/usr/bin/env python
"""What stepping several videos together buys the merge loop: aggregate frames/s of `premvos_amd.track`'s sequential ``do_video`` over 4
videos against ``do_videos_lockstep`` with 2 and 4 seats (premvos_amd.track.TrackerGroup), on the clip of tools/time_track_loop.py
(480x854, 64 frames, 10 objects, 20 fresh proposals per frame, full-depth nets, synthetic weights) as a file tree with 4 videos (one set
of files, four names).  Every program is a fresh child: engines, a warm-up pass over the whole tree (plans, graphs, allocator, page
cache), then the timed pass with the shader clock sampled.  The sequence sequential / 2 seats / 4 seats runs twice, alternating, in one
call; a last child runs 4 seats instrumented (a synchronise per phase) for the ms per phase.  The phase clock runs on from step to
step: `decode` also holds the host's work between two steps (prefetch waits, parsing, uploads, writer hand-over).

The yardstick is the sequential loop of the same call, nothing fixed in advance: "faster" may be claimed only if both 4-seat runs exceed
both sequential runs by more than the two sequential runs differ from each other (``lockstep4_faster`` in the result).

    python tools/time_track_lockstep.py [--frames 64] [--objects 10] [--candidates 20] [--videos 4] [--out profiles/track_lockstep.json]
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
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

H, W = 480, 854
MODES = {"sequential": 1, "lockstep2": 2, "lockstep4": 4}


def layout(tree: str, out: str = "out") -> dict:
    return {k: os.path.join(tree, k) + "/" for k in ("images", "anns", "props", "flows")} | {"out": os.path.join(tree, out) + "/"}


def build_tree(tree: str, frames: int, objects: int, candidates: int, videos: int) -> None:
    """time_track_loop.py's clip as files: JPEGs, the first frame's annotation (``objects`` boxes), per-frame proposal files with ReID,
    .flo files; videos clip1.. are links to clip0's folders.  Host only."""
    from PIL import Image
    from premvos_amd import rle, synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_restated as R
    lay = layout(tree)
    for k in ("images", "anns", "props", "flows"):
        os.makedirs(os.path.join(lay[k], "clip0"))
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    clip = synth.clip_frames(0, frames, H, W).numpy()
    cand_boxes = synth.clip_boxes(0, frames, candidates, H, W).numpy()

    def box_mask(b):
        m = np.zeros((H, W), np.uint8)
        y0, x0, y1, x1 = (int(v) for v in b)
        m[y0:max(y1, y0 + 1), x0:max(x1, x0 + 1)] = 1
        return m
    ann, n = np.zeros((H, W), np.uint8), 0
    for b in synth.boxes(1, 8 * objects, H, W, rank=99)[0].numpy():            # (an annotation is one plane: each object keeps what is still free)
        free = (box_mask(b) != 0) & (ann == 0)
        if n < objects and free.sum() >= 0.5 * box_mask(b).sum():
            n += 1
            ann[free] = n
    assert n == objects, "too few boxes with half of their area free"
    R.write_index_png(os.path.join(lay["anns"], "clip0", "00000.png"), ann)
    for t in range(frames):
        Image.fromarray(clip[t]).save(os.path.join(lay["images"], "clip0", f"{t:05d}.jpg"), quality=95)
        if t < frames - 1:
            R.write_flo(os.path.join(lay["flows"], "clip0", f"{t:05d}.flo"),
                        np.stack([2.5 * np.sin(yy / 97.0 + 0.1 * t) + 1.25, 1.5 * np.cos(xx / 131.0 - 0.07 * t) - 0.5], -1).astype(np.float32))
        props = []
        for b in cand_boxes[t]:
            seg = rle.encode(box_mask(b))
            props.append({"bbox": rle.to_bbox(seg), "segmentation": seg, "score": round(float(rng.uniform(0.5, 1.0)), 2), "conf_score": "0.5",
                          "ReID": rng.normal(0, 0.3, 128).round(4).tolist()})
        with open(os.path.join(lay["props"], "clip0", f"{t:05d}.json"), "w") as f:
            json.dump(props, f)
    for v in range(1, videos):
        for k in ("images", "anns", "props", "flows"):
            os.symlink("clip0", os.path.join(lay[k], f"clip{v}"))


def child(tree: str, mode: str, videos: int, phases: bool) -> dict:
    import torch
    import bench
    from oracle import reid_oracle as QO
    from premvos_amd import _lib, io_pipeline as iop, synth, track
    from premvos_amd.refinement import RefinementNet
    from premvos_amd.refinement.driver import RefinementEngine
    from premvos_amd.reid import ReIDEngine, ReIDNet
    dev = _lib.resolve_device()
    ref_eng = RefinementEngine(RefinementNet(synth.refinement_weights(0), 16, dev))
    reid_eng = ReIDEngine(ReIDNet(QO.synth_weights(0), dev))
    names = [f"clip{v}" for v in range(videos)]
    spent: dict = {}
    clock = [0.0]

    def tick(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        spent[name] = spent.get(name, 0.0) + now - clock[0]
        clock[0] = now

    def run(out: str, timer=None) -> int:
        lay = layout(tree, out)
        with iop.Writer() as writer:
            if MODES[mode] == 1:
                n = sum(len(track.do_video(os.path.join(lay["images"], v) + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"],
                                           ref_eng, reid_eng, writer=writer)) for v in names)
            else:
                n = sum(len(x) for x in track.do_videos_lockstep(names, lay, MODES[mode], ref_eng, reid_eng, writer, timer=timer).values())
            torch.cuda.synchronize()
        return n
    run(f"out_{mode}_warm")
    shutil.rmtree(os.path.join(tree, f"out_{mode}_warm"))
    torch.cuda.synchronize()
    with bench.BoxSampler(dev.index) as box:
        t0 = time.perf_counter()
        n = run(f"out_{mode}")                                                # (the clock stops when the last PNG is on disk)
        dt = time.perf_counter() - t0
    s = box.summary()
    res = {"mode": mode, "seats": MODES[mode], "videos": videos, "frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 2),
           "sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean")}
    if phases:
        clock[0] = time.perf_counter()
        t0 = clock[0]
        n = run(f"out_{mode}_phases", tick)
        total = time.perf_counter() - t0
        steps = n / MODES[mode]
        res["phase_ms_per_step_with_syncs"] = {k: round(1e3 * v / steps, 3) for k, v in spent.items()}
        res["phase_ms_per_step_with_syncs"]["outside the steps (seating the videos, closing the writer)"] = round(1e3 * (total - sum(spent.values())) / steps, 3)
        res["steps"] = steps
        shutil.rmtree(os.path.join(tree, f"out_{mode}_phases"))
    shutil.rmtree(os.path.join(tree, f"out_{mode}"))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--child", default=None, choices=sorted(MODES), help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--phases", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.tree, a.child, a.videos, a.phases)), flush=True)
        return 0
    tree = tempfile.mkdtemp(prefix="track_lockstep_")
    try:
        build_tree(tree, a.frames, a.objects, a.candidates, a.videos)
        runs = []

        def one(mode: str, phases: bool = False) -> dict:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--videos", str(a.videos)] + (["--phases"] if phases else [])
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(json.dumps(res), flush=True)
            return res
        for k in range(2):
            for mode in ("sequential", "lockstep2", "lockstep4"):
                runs.append(dict(one(mode), alternation=k))
        ph = one("lockstep4", phases=True)
    finally:
        shutil.rmtree(tree, ignore_errors=True)
    fps = {m: [r["frames_per_s"] for r in runs if r["mode"] == m] for m in MODES}
    spread = abs(fps["sequential"][0] - fps["sequential"][1])
    out = {"what": f"premvos_amd.track over {a.videos} videos of one synthetic 480x854 clip ({a.frames} frames, {a.objects} objects, {a.candidates} fresh "
                   "proposals per frame, full-depth nets): aggregate frames/s, files in, PNGs on disk; fresh child per run, warm-up pass then timed pass",
           "runs": runs, "frames_per_s": fps, "sequential_spread_frames_per_s": round(spread, 2),
           "lockstep4_faster": bool(min(fps["lockstep4"]) - max(fps["sequential"]) > spread),
           "lockstep2_faster": bool(min(fps["lockstep2"]) - max(fps["sequential"]) > spread),
           "rule": "faster = both lockstep runs exceed both sequential runs by more than the two sequential runs differ",
           "lockstep4_phases": ph}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
