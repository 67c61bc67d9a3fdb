#!/usr/bin/env python
"""What running a video's weight sets in lockstep buys the live loop's weight search: frames x sets per second of W sequential
``do_video`` runs, one per weight set through ``Tracker(weights=...)``, against ``track.search_video`` with the same W sets
(premvos_amd.track.SearchGroup), for W = 4 and W = 8, on the clip of tools/time_track_loop.py (480x854, 64 frames, 10 objects, 20 fresh
proposals per frame, full-depth nets, synthetic weights) as a file tree with an annotation for every frame.  Every program is a fresh
child: engines, a warm-up pass (plans, graphs, allocator, page cache), then the timed pass with the shader clock sampled.  The sequence
sequential4 / search4 / sequential8 / search8 runs twice, alternating, in one call, every child under its own time limit; a last child runs
search8 instrumented (a synchronise per phase) for the ms per phase.  The phase clock runs on from step to step: `decode` also holds
the host's work between two steps (prefetch waits, parsing, uploads).

The two sides do not do the same host work: a sequential run writes its PNGs (it is the loop as it exists), the search reads each
annotation and writes nothing.  The yardstick is the sequential loop of the same call, nothing fixed in advance: "faster" may be claimed
only if both search runs exceed both sequential runs by more than the two sequential runs differ from each other.

    python tools/time_live_search.py [--frames 64] [--objects 10] [--candidates 20] [--out profiles/live_search.json]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"sequential4": 4, "search4": 4, "sequential8": 8, "search8": 8}


def _lockstep_tool():
    spec = importlib.util.spec_from_file_location("time_track_lockstep", os.path.join(ROOT, "tools", "time_track_lockstep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_tree(tree: str, frames: int, objects: int, candidates: int) -> None:
    """time_track_lockstep.py's tree with one video, and the first frame's annotation copied to every frame (the search reads one per
    frame; what it scores does not matter here).  Host only."""
    LT = _lockstep_tool()
    LT.build_tree(tree, frames, objects, candidates, 1)
    anns = os.path.join(LT.layout(tree)["anns"], "clip0")
    for t in range(1, frames):
        shutil.copyfile(os.path.join(anns, "00000.png"), os.path.join(anns, f"{t:05d}.png"))


def child(tree: str, mode: str, phases: bool) -> dict:
    import torch
    import bench
    from oracle import reid_oracle as QO
    from premvos_amd import _lib, io_pipeline as iop, synth, track
    from premvos_amd.refinement import RefinementNet
    from premvos_amd.refinement.driver import RefinementEngine
    from premvos_amd.reid import ReIDEngine, ReIDNet
    LT = _lockstep_tool()
    dev = _lib.resolve_device()
    ref_eng = RefinementEngine(RefinementNet(synth.refinement_weights(0), 16, dev))
    reid_eng = ReIDEngine(ReIDNet(QO.synth_weights(0), dev))
    W = MODES[mode]
    ws = track.live_search_weights(W, seed=0)
    spent: dict = {}
    clock = [0.0]

    def tick(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        spent[name] = spent.get(name, 0.0) + now - clock[0]
        clock[0] = now

    def run(out: str, timer=None) -> int:
        lay = LT.layout(tree, out)
        if mode.startswith("sequential"):
            n = 0
            with iop.Writer() as writer:
                for w in ws:
                    n += len(track.do_video(os.path.join(lay["images"], "clip0") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"],
                                            lay["out"], ref_eng, reid_eng, writer=writer, tracker=track.Tracker(ref_eng, reid_eng, weights=w)))
                torch.cuda.synchronize()
            shutil.rmtree(os.path.join(tree, out))
            return n
        with iop.thread_pool(max(1, iop.io_threads()), "premvos-search") as pool:
            r = track.search_video("clip0", lay, ws, ref_eng, reid_eng, pool=pool, timer=timer)      # (ends with the counts on the host)
        return r["frames"] * W
    run(f"out_{mode}_warm")
    torch.cuda.synchronize()
    with bench.BoxSampler(dev.index) as box:
        t0 = time.perf_counter()
        n = run(f"out_{mode}")
        dt = time.perf_counter() - t0
    s = box.summary()
    res = {"mode": mode, "sets": W, "frames_x_sets": n, "seconds": round(dt, 3), "frames_x_sets_per_s": round(n / dt, 2),
           "sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean")}
    if phases:
        clock[0] = time.perf_counter()
        t0 = clock[0]
        n = run(f"out_{mode}_phases", tick)
        total = time.perf_counter() - t0
        steps = n / W
        res["phase_ms_per_step_with_syncs"] = {k: round(1e3 * v / steps, 3) for k, v in spent.items()}
        res["phase_ms_per_step_with_syncs"]["outside the steps (seating the video, the counts' copy)"] = round(1e3 * (total - sum(spent.values())) / steps, 3)
        res["steps"] = steps
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--child", default=None, choices=sorted(MODES), help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--phases", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.tree, a.child, a.phases)), flush=True)
        return 0
    tree = tempfile.mkdtemp(prefix="live_search_")
    try:
        build_tree(tree, a.frames, a.objects, a.candidates)
        runs = []

        def one(mode: str, phases: bool = False) -> dict:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree] + (["--phases"] if phases else [])
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)      # (a child's own time limit; a failure ends the call)
            if r.returncode != 0:
                raise RuntimeError(f"{cmd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(json.dumps(res), flush=True)
            return res
        for k in range(2):
            for mode in MODES:
                runs.append(dict(one(mode), alternation=k))
        ph = one("search8", phases=True)
    finally:
        shutil.rmtree(tree, ignore_errors=True)
    rate = {m: [r["frames_x_sets_per_s"] for r in runs if r["mode"] == m] for m in MODES}
    out = {"what": f"the live loop under W weight sets on one synthetic 480x854 clip ({a.frames} frames, {a.objects} objects, {a.candidates} fresh "
                   "proposals per frame, full-depth nets): frames x sets per second; sequential = W do_video runs through Tracker(weights=) with "
                   "PNGs on disk, search = track.search_video (SearchGroup); fresh child per run, warm-up pass then timed pass",
           "runs": runs, "frames_x_sets_per_s": rate,
           "rule": "faster = both search runs exceed both sequential runs by more than the two sequential runs differ", "search8_phases": ph}
    for W in (4, 8):
        seq, sea = rate[f"sequential{W}"], rate[f"search{W}"]
        spread = abs(seq[0] - seq[1])
        out[f"sequential{W}_spread"] = round(spread, 2)
        out[f"search{W}_faster"] = bool(min(sea) - max(seq) > spread)
        out[f"search{W}_ratio_min_max"] = [round(min(sea) / max(seq), 3), round(max(sea) / min(seq), 3)]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
