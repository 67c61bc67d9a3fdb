#!/usr/bin/env python
"""What it costs to get output/intermediate/ReID_proposals/: two programs, or one.

    leg 1  `premvos_amd.stream` (stages A-D), then `premvos_amd.reid.driver.forward_directory` on its tree -- the two-program way:
           the second program decodes every JPEG again, parses the refined JSON, walks every RLE string for the boxes, launches the
           net per frame and waits for a device-to-host copy per frame
    leg 2  `premvos_amd.stream --reid`: the ReID net runs on the refined masks while they are in HBM

The job is that of tools/time_merge_ingest.build_job: a synthetic 480x854 clip, `object_like_refinement_weights()` (the plain synthetic
refinement weights give empty masks: nothing to embed) and the full-depth ReID net.  Every program runs in a FRESH child process under
its own time limit: it builds its nets, runs the clip once untimed (plans, allocator), then once timed with a synchronise before
each clock read while a host thread samples the shader clock.  The legs are alternated (1, 2, 1, 2) in one call because boxes
differ by ~5 % in clock; a child that fails ends the call.  The condition: leg 2 takes less wall time than the sum of leg 1's two
programs in BOTH alternations; `stream` without --reid is reported twice, which is the run-to-run spread of the unchanged form.

    python tools/time_stream_reid.py [--frames 64] [--out profiles/stream_reid.json]
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

WEIGHTS = ("weights/pwc.pth.tar", "weights/general.pt", "weights/specific.pt", "weights/refine.pt")
CONFIG = "code/ReID_net/configs/run"
IMAGES = "data/DAVIS/JPEGImages/480p/"


def build_job(root: str, n_frames: int) -> None:
    """time_merge_ingest.build_job + the ReID stage's config and full-depth weights + seq_to_run.txt.  Host only."""
    import torch
    from oracle import reid_oracle as QO
    from tools.time_merge_ingest import build_job as base_job
    base_job(root, n_frames, 1)
    torch.save(QO.synth_weights(0), os.path.join(root, "weights", "reid.pt"))
    os.makedirs(os.path.join(root, os.path.dirname(CONFIG)))
    with open(os.path.join(root, CONFIG), "w") as f:
        json.dump({"model": "Re-ID", "load": "../weights/reid.pt", "input_size": [128, 128]}, f)
    with open(os.path.join(root, "seq_to_run.txt"), "w") as f:
        f.write(IMAGES + "clip0/\n")


def _timed(fn, device_index: int):
    """fn() between two synchronises, with the clock the box granted meanwhile -> (seconds, fn's result, box summary)."""
    import torch
    import bench
    torch.cuda.synchronize()
    with bench.BoxSampler(device_index) as box:
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    s = box.summary()
    return dt, res, {"sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"),
                     "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean"), "error": s.get("error")}


def child_stream(root: str, out: str, reid: bool) -> dict:
    import torch
    from premvos_amd import stream
    os.chdir(root)
    warm = out.rstrip("/") + "_warm"
    pipe = stream.StreamPipeline(*WEIGHTS, batch=8, out=warm, reid_config=CONFIG if reid else None)
    clip = [IMAGES + "clip0/"]
    n = pipe.run_sequences(clip)
    shutil.rmtree(warm)
    pipe.out = out
    dt, n2, box = _timed(lambda: pipe.run_sequences(clip), pipe.dev.index)
    assert n == n2
    rep = {"program": "stream --reid" if reid else "stream", "frames": n, "seconds": round(dt, 4), "frames_per_s": round(n / dt, 2),
           "box": box}
    if reid:
        # the ReID step alone: a third pass with a synchronise on both sides of every call (one call = one launch group of the
        # refinement net: PREMVOS_DRIVER_BATCH frames) -- slower than the overlapped form above by design
        calls, step = [], pipe._reid_step

        def instrumented(*a, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = step(*a, **kw)
            torch.cuda.synchronize()
            calls.append((time.perf_counter() - t, len(a[3])))
            return r
        pipe._reid_step = instrumented
        pipe.out = warm
        pipe.run_sequences(clip)
        shutil.rmtree(warm)
        rep["reid_step"] = {"groups": len(calls), "ms_per_group_with_syncs": round(1e3 * sum(c[0] for c in calls) / max(len(calls), 1), 3),
                            "slots_per_group_mean": round(sum(c[1] for c in calls) / max(len(calls), 1), 1),
                            "ms_per_slot": round(1e3 * sum(c[0] for c in calls) / max(sum(c[1] for c in calls), 1), 4)}
    return rep


def child_reid_driver(root: str, inter: str) -> dict:
    """The second program of leg 1, as tools/run_stages.py starts it (config 'load' resolved from code/)."""
    from premvos_amd import _lib
    from premvos_amd.reid import driver as qd
    os.chdir(root)
    cfg = qd.Config(CONFIG)
    cfg._entries["load"] = os.path.normpath(os.path.join(root, "code", cfg.str("load")))
    eng = qd.engine_from_config(cfg)
    refined, warm, out = os.path.join(inter, "refined_proposals") + "/", inter.rstrip("/") + "_warm/", os.path.join(inter, "ReID_proposals") + "/"
    n = qd.forward_directory(eng, IMAGES, refined, warm)
    shutil.rmtree(warm)
    dt, n2, box = _timed(lambda: qd.forward_directory(eng, IMAGES, refined, out), _lib.resolve_device().index)
    assert n == n2
    return {"program": "reid.driver.forward_directory", "frames": n, "seconds": round(dt, 4), "frames_per_s": round(n / dt, 2), "box": box}


def embedded_per_frame(inter: str) -> float:
    files = sorted(glob.glob(os.path.join(inter, "ReID_proposals", "*", "*.json")))
    return round(sum(sum("ReID" in p for p in json.load(open(f))) for f in files) / max(len(files), 1), 2)


def compare_trees(a: str, b: str) -> dict:
    """ReID_proposals/ of the two ways: the same proposals carry the key; the largest embedding difference relative to max(1, |ref|.max())."""
    worst, n = 0.0, 0
    for fa in sorted(glob.glob(os.path.join(a, "ReID_proposals", "*", "*.json"))):
        pa, pb = json.load(open(fa)), json.load(open(os.path.join(b, os.path.relpath(fa, a))))
        assert [list(p) for p in pa] == [list(p) for p in pb], fa
        for x, y in zip(pa, pb):
            if "ReID" in x:
                ref = max(1.0, max(abs(v) for v in x["ReID"]))
                worst = max(worst, max(abs(u - v) for u, v in zip(x["ReID"], y["ReID"])) / ref)
                n += 1
    return {"embeddings_compared": n, "worst_relative_difference": worst, "same_keys": True}


def run_child(args: list, limit: int) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit(f"time_stream_reid: child {args} ended with {r.returncode}; nothing more is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_reid.json"))
    ap.add_argument("--child", default=None, choices=["stream", "stream_reid", "reid_driver"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--inter", default=None)
    a = ap.parse_args()
    if a.child:
        rep = child_reid_driver(a.root, a.inter) if a.child == "reid_driver" else child_stream(a.root, a.inter, a.child == "stream_reid")
        print(json.dumps(rep))
        return 0
    root = tempfile.mkdtemp(prefix="premvos_stream_reid_")
    try:
        build_job(root, a.frames)
        rep = {"what": "tools/time_stream_reid.py: output/intermediate/ReID_proposals/ of a synthetic 480x854 clip by two programs (stream, "
                       "then reid.driver.forward_directory) and by one (stream --reid); every program in a fresh process, one warm-up pass, "
                       "one timed pass, legs alternated",
               "frames": a.frames, "alternations": []}
        for k in range(a.alternations):
            two, one = os.path.join(root, f"two{k}", "intermediate"), os.path.join(root, f"one{k}", "intermediate")
            s = run_child(["--child", "stream", "--root", root, "--inter", two], a.limit)
            q = run_child(["--child", "reid_driver", "--root", root, "--inter", two], a.limit)
            r = run_child(["--child", "stream_reid", "--root", root, "--inter", one], a.limit)
            total = round(s["seconds"] + q["seconds"], 4)
            rep["alternations"].append({
                "leg1_two_programs": {"stream": s, "reid_driver": q, "seconds": total, "frames_per_s": round(a.frames / total, 2),
                                      "embedded_proposals_per_frame": embedded_per_frame(two)},
                "leg2_one_program": dict(r, embedded_proposals_per_frame=embedded_per_frame(one)),
                "leg2_over_leg1_seconds": round(r["seconds"] / total, 3), "leg2_faster": bool(r["seconds"] < total),
                "trees": compare_trees(two, one)})
            shutil.rmtree(os.path.dirname(two))
            shutil.rmtree(os.path.dirname(one))
        plain = [x["leg1_two_programs"]["stream"]["frames_per_s"] for x in rep["alternations"]]
        rep["stream_without_reid_frames_per_s"] = plain
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
