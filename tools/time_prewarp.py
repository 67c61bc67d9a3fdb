#!/usr/bin/env python
"""What the pre-warp merge (`premvos_amd.track --prewarp`, premvos_amd/prewarp.py) costs next to the live-warp loop: aggregate frames/s,
files in, PNGs on disk, of `track` (sequential ``do_video``), `track --lockstep 4` and `track --prewarp` on the 4-video x 64-frame tree of
tools/time_track_lockstep.py (480x854, 10 objects, 20 proposals per frame, full-depth nets, synthetic weights).  Every program is a
fresh child process: engines, a warm-up pass over the whole tree, then the timed pass with the shader clock sampled.  The sequence
track / lockstep4 / prewarp runs twice, alternating, in one call.  A last pair of children times ``--prewarp-search 256`` (every frame
annotated: the tree's first annotation copied to each frame) against 256 x the single pre-warp pass of the same call.

8.4's rule: "faster" holds only if both prewarp runs exceed both ``--lockstep 4`` runs by more than those two differ from each other
(``prewarp_faster_than_lockstep4``).  The two merges do NOT compute the same thing: the pre-warp merge runs no network in the loop, and
its quality on DAVIS is unmeasured -- these are costs, not a like-for-like comparison.

    python tools/time_prewarp.py [--frames 64] [--objects 10] [--candidates 20] [--videos 4] [--sets 256] [--out profiles/prewarp.json]

``--negatives``: the other leg -- only `track --prewarp` and `track --prewarp --negatives` (all negatives) on the same tree, a fresh child
per program, alternating, two runs each: what the negative first-frame templates cost next to the merge without them,
with the spread of the two runs and how many negatives each video took.  No threshold; a cost, not a measure of quality.

    python tools/time_prewarp.py --negatives [--out profiles/prewarp_neg.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import time_track_lockstep as L  # noqa: E402

MODES = ("track", "lockstep4", "prewarp")
NEG_MODES = ("prewarp", "prewarp_neg")


def annotate_every_frame(tree: str, frames: int, videos: int) -> None:
    """anns_all/: the first frame's annotation under every frame's name (the search needs an annotation per frame)"""
    src = os.path.join(tree, "anns", "clip0", "00000.png")
    os.makedirs(os.path.join(tree, "anns_all", "clip0"))
    for t in range(frames):
        shutil.copyfile(src, os.path.join(tree, "anns_all", "clip0", f"{t:05d}.png"))
    for v in range(1, videos):
        os.symlink("clip0", os.path.join(tree, "anns_all", f"clip{v}"))


def keep_objects(tree: str, keep: int) -> None:
    """the --negatives leg: only the ids 1 .. ``keep`` stay annotated, so that proposals clear of them exist and negatives are taken"""
    import numpy as np
    from PIL import Image
    fn = os.path.join(tree, "anns", "clip0", "00000.png")
    ann = np.array(Image.open(fn))
    ann[ann > keep] = 0
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import track_restated as R                                                    # (the tree's own writer of index PNGs)
    R.write_index_png(fn, ann)


def child(tree: str, mode: str, videos: int, sets: int) -> dict:
    if mode in ("track", "lockstep4"):
        r = L.child(tree, "sequential" if mode == "track" else "lockstep4", videos, False)
        r["mode"] = mode
        return r
    import torch
    import bench
    from oracle import reid_oracle as QO
    from premvos_amd import _lib, io_pipeline as iop, prewarp as pw
    from premvos_amd.reid import ReIDEngine, ReIDNet
    dev = _lib.resolve_device()
    reid_eng = ReIDEngine(ReIDNet(QO.synth_weights(0), dev))
    names = [f"clip{v}" for v in range(videos)]

    negatives = "all" if mode == "prewarp_neg" else None

    def run(out: str, search: int = 0) -> int:
        lay = L.layout(tree, out)
        if search:
            lay["anns"] = os.path.join(tree, "anns_all") + "/"
        with iop.Writer() as writer:
            n = pw.run_tree(tree, names, search_sets=search, ReID_net=reid_eng, writer=writer, lay=lay, negatives=negatives)["frames"]
            torch.cuda.synchronize()
        return n

    def timed(out: str, search: int = 0) -> dict:
        run(out + "_warm", search)
        shutil.rmtree(os.path.join(tree, out + "_warm"), ignore_errors=True)
        torch.cuda.synchronize()
        with bench.BoxSampler(dev.index) as box:
            t0 = time.perf_counter()
            n = run(out, search)                                              # (the clock stops when the last PNG is on disk)
            dt = time.perf_counter() - t0
        s = box.summary()
        shutil.rmtree(os.path.join(tree, out), ignore_errors=True)
        return {"frames": n, "seconds": round(dt, 3), "frames_per_s": round(n / dt, 2),
                "sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean")}
    if mode == "prewarp":
        return dict(timed("out_prewarp"), mode=mode, videos=videos)
    if mode == "prewarp_neg":
        r = dict(timed("out_prewarp_neg"), mode=mode, videos=videos)
        with open(os.path.join(tree, "output", "prewarp_negatives.json")) as f:       # (run_tree writes it under the tree's root)
            took = {k: {"candidates": v["candidates"], "taken": len(v["taken"]), "templates": v["templates"]} for k, v in json.load(f)["videos"].items()}
        return dict(r, negatives=took)
    single, many = timed("out_prewarp_single"), timed("out_prewarp_search", sets)
    return {"mode": "search", "sets": sets, "videos": videos, "single_pass": single, "search": many,
            "search_seconds_over_sets_x_single_pass": round(many["seconds"] / (sets * single["seconds"]), 5)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--negatives", action="store_true", help="the --negatives leg: track --prewarp against track --prewarp --negatives only")
    ap.add_argument("--keep-objects", type=int, default=2, help="--negatives: how many of the --objects stay annotated (the others' proposals "
                                                                "are then free to become negatives)")
    ap.add_argument("--child", default=None, choices=MODES + ("search", "prewarp_neg"), help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.tree, a.child, a.videos, a.sets)), flush=True)
        return 0
    tree = tempfile.mkdtemp(prefix="time_prewarp_")
    try:
        L.build_tree(tree, a.frames, a.objects, a.candidates, a.videos)
        if a.negatives:
            keep_objects(tree, a.keep_objects)
        annotate_every_frame(tree, a.frames, a.videos)
        runs = []

        def one(mode: str) -> dict:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--videos", str(a.videos), "--sets", str(a.sets)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(json.dumps(res), flush=True)
            return res
        for k in range(2):
            for mode in (NEG_MODES if a.negatives else MODES):
                runs.append(dict(one(mode), alternation=k))
        search = None if a.negatives else one("search")
    finally:
        shutil.rmtree(tree, ignore_errors=True)
    if a.negatives:
        fps = {m: [r["frames_per_s"] for r in runs if r["mode"] == m] for m in NEG_MODES}
        out = {"what": f"premvos_amd.track --prewarp with and without --negatives over {a.videos} videos of one synthetic 480x854 clip ({a.frames} "
                       f"frames, {a.keep_objects} of {a.objects} objects annotated, {a.candidates} proposals per frame): aggregate frames/s, files in, PNGs on disk; fresh child "
                       "per run, warm-up pass then timed pass, alternating, two runs each",
               "runs": runs, "frames_per_s": fps, "spread_frames_per_s": {m: round(abs(v[0] - v[1]), 2) for m, v in fps.items()},
               "negatives_over_prewarp": round((sum(fps["prewarp_neg"]) / 2) / (sum(fps["prewarp"]) / 2), 4),
               "negatives": next(r["negatives"] for r in runs if r["mode"] == "prewarp_neg"),
               "quality": "J&F with the negative templates on DAVIS is unmeasured (no weights, no dataset here)"}
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
        print(json.dumps(out))
        return 0
    fps = {m: [r["frames_per_s"] for r in runs if r["mode"] == m] for m in MODES}
    spread = abs(fps["lockstep4"][0] - fps["lockstep4"][1])
    out = {"what": f"premvos_amd.track over {a.videos} videos of one synthetic 480x854 clip ({a.frames} frames, {a.objects} objects, {a.candidates} "
                   "proposals per frame, full-depth nets): aggregate frames/s, files in, PNGs on disk; fresh child per run, warm-up pass then timed pass",
           "runs": runs, "frames_per_s": fps, "lockstep4_spread_frames_per_s": round(spread, 2),
           "prewarp_faster_than_lockstep4": bool(min(fps["prewarp"]) - max(fps["lockstep4"]) > spread),
           "rule": "faster = both prewarp runs exceed both --lockstep 4 runs by more than those two differ from each other",
           "search": search,
           "quality": "J&F of the pre-warp merge on DAVIS is unmeasured (no weights, no dataset here); it runs no network in the loop and is "
                      "not presented as equal in quality to the live-warp loop"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
