#!/usr/bin/env python
"""What an overlay JPEG costs: the forward kernel, the host Huffman pass, and `stream --track` with and without `--overlay`.

    kernel   premvos_jpeg_forward_u8 at 480x854, 4:2:0, quality 95, plain and with the blend fused in: device events around
             back-to-back launches into one preallocated buffer (warm-up first; REPEATS windows of LAUNCHES launches; the per-launch
             time of a window bounds the kernel's time from above), and the GB/s of compulsory bytes -- 3 B read per pixel (+ 1 B of
             id map with the blend), 2 B written per coefficient
    host     premvos_jpeg_entropy_encode_host on the same coefficients, one thread, ms per frame and the file's size
    stream   `premvos_amd.stream --track` frames/s on the synthetic clip of tools/time_stream_track.py (480x854, 10 objects, full-depth
             nets) without the flag, with `--overlay`, and -- with --baseline-tree, a built checkout of the commit this one is compared
             with -- that commit's own `stream --track`: every program in a FRESH child process under its own time limit, one warm-up pass,
             one timed pass with the shader clock sampled, the three alternated in one call.  A child that fails ends the call.

No threshold: nothing here was timed before.  The report says which of the two -- one writer thread's Huffman pass, or the frame period
of the merge loop -- is the longer, i.e. what bounds the flag.

    python tools/time_jpeg_encode.py [--frames 64] [--baseline-tree DIR] [--out profiles/jpeg_encode.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 480, 854
WARMUP, REPEATS, LAUNCHES = 50, 7, 500


def child_kernel() -> dict:
    import numpy as np
    import torch
    from premvos_amd import _lib, jpeg, overlay, synth
    from tools.time_stream_reid import _timed
    lib, dev = _lib.load(), _lib.resolve_device()
    frame = synth.clip_frames(0, 1, H, W)[0].to(dev).contiguous()
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ids = np.zeros((H, W), np.uint8)
    for i in range(10):                                      # the annotation of tools/time_stream_track.build_job
        cy, cx = 110 + 250 * (i // 5), 100 + 160 * (i % 5)
        ids[((yy - cy) / (60 + 4 * i)) ** 2 + ((xx - cx) / (55 + 2 * i)) ** 2 <= 1] = i + 1
    idmap, pal = torch.from_numpy(ids).to(dev), overlay.palette(dev)
    ql, qc = jpeg.quant_tables(overlay.QUALITY)
    info = jpeg.JpegInfo()
    rep = {"program": "kernel + host pass", "shape": [H, W], "sampling": "4:2:0", "quality": overlay.QUALITY}
    for tag, im, pl in (("plain", None, None), ("blend_fused", idmap, pal)):
        args = (frame.data_ptr(), im.data_ptr() if im is not None else None, pl.data_ptr() if pl is not None else None, H, W,
                ql.ctypes.data, qc.ctypes.data, 2, 2, C.byref(info))
        _lib.check(lib.premvos_jpeg_forward_u8(*args, None, 0, None), "forward")
        n = int(info.coef_count)
        coef = torch.empty(n, dtype=torch.int16, device=dev)
        stream = _lib.current_stream()

        def launches(k):
            for _ in range(k):
                lib.premvos_jpeg_forward_u8(*args, coef.data_ptr(), n, stream)
        launches(WARMUP)
        per_launch = []

        def windows():
            for _ in range(REPEATS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launches(LAUNCHES)
                b.record()
                b.synchronize()
                per_launch.append(a.elapsed_time(b) * 1e3 / LAUNCHES)
        _, _, box = _timed(windows, dev.index)
        nbytes = H * W * (3 + (1 if im is not None else 0)) + 2 * n
        us = statistics.median(per_launch)
        host_coef = coef.cpu().numpy()
        out = np.empty(2 * n + 4096, np.uint8)
        written, ms = C.c_int64(0), []
        for _ in range(30):
            t = time.perf_counter()
            rc = lib.premvos_jpeg_entropy_encode_host(host_coef.ctypes.data, C.byref(info), out.ctypes.data, out.size, C.byref(written))
            ms.append(1e3 * (time.perf_counter() - t))
            assert rc == 0
        rep[tag] = {"forward_us_per_launch": {"median": round(us, 2), "min": round(min(per_launch), 2), "max": round(max(per_launch), 2),
                                              "windows": REPEATS, "launches_per_window": LAUNCHES},
                    "compulsory_bytes": nbytes, "gb_per_s_of_compulsory_bytes": round(nbytes / us / 1e3, 1), "box": box,
                    "host_huffman_ms_per_frame_one_thread": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3)},
                    "file_bytes": int(written.value)}
    return rep


def child_stream(root: str, out: str, overlay_flag: bool) -> dict:
    """tools/time_stream_track.child_stream's track leg, with ``--overlay`` on request."""
    from premvos_amd import stream
    from tools.time_stream_reid import CONFIG, IMAGES, WEIGHTS, _timed
    from tools.time_stream_track import LIVE
    os.chdir(root)
    warm, base = out.rstrip("/") + "_warm", os.path.dirname(out.rstrip("/"))
    track = dict(LIVE, final=os.path.join(base, "final_warm"), anns="data/DAVIS/Annotations/480p",
                 overlay=os.path.join(base, "overlay_warm") if overlay_flag else None)
    pipe = stream.StreamPipeline(*WEIGHTS, batch=8, out=warm, reid_config=CONFIG, track=track)
    clip = [IMAGES + "clip0/"]
    n = pipe.run_sequences(clip)
    for d in (warm, track["final"], track["overlay"]):
        if d:
            shutil.rmtree(d)
    pipe.out, track["final"] = out, os.path.join(base, "final")
    if overlay_flag:
        track["overlay"] = os.path.join(base, "overlay")
    dt, n2, box = _timed(lambda: pipe.run_sequences(clip), pipe.dev.index)
    assert n == n2
    rep = {"program": "stream --track --overlay" if overlay_flag else "stream --track", "frames": n, "seconds": round(dt, 4),
           "frames_per_s": round(n / dt, 2), "box": box}
    if overlay_flag:
        jpgs = [os.path.join(track["overlay"], "clip0", f) for f in sorted(os.listdir(os.path.join(track["overlay"], "clip0")))]
        rep["overlay_files"], rep["overlay_bytes_mean"] = len(jpgs), round(sum(map(os.path.getsize, jpgs)) / max(len(jpgs), 1))
    return rep


def run_child(cmd: list, limit: int, cwd: str) -> dict:
    r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=limit, cwd=cwd)
    if r.returncode != 0:
        raise SystemExit(f"time_jpeg_encode: child {cmd} ended with {r.returncode}; nothing more is started\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"time_jpeg_encode: {rep['program']}: done", file=sys.stderr, flush=True)
    return rep


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout of the commit to compare with: its own stream --track is timed too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.txt"))
    ap.add_argument("--child", default=None, choices=["kernel", "track", "track_overlay"])
    ap.add_argument("--root", default=None)
    ap.add_argument("--inter", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_kernel() if a.child == "kernel" else child_stream(a.root, a.inter, a.child == "track_overlay")))
        return 0
    me = os.path.abspath(__file__)
    rep = {"what": "tools/time_jpeg_encode.py", "frames": a.frames, "kernel": run_child([me, "--child", "kernel"], a.limit, ROOT), "stream": []}
    root = tempfile.mkdtemp(prefix="premvos_jpeg_encode_")
    try:
        from tools.time_stream_track import build_job
        build_job(root, a.frames)
        for k in range(a.alternations):
            row = {}
            if a.baseline_tree:
                base = os.path.abspath(a.baseline_tree)
                row["baseline_stream_track"] = run_child([os.path.join(base, "tools", "time_stream_track.py"), "--child", "track", "--root", root,
                                                          "--inter", os.path.join(root, f"base{k}", "intermediate")], a.limit, base)
            row["stream_track"] = run_child([me, "--child", "track", "--root", root, "--inter", os.path.join(root, f"off{k}", "intermediate")],
                                            a.limit, ROOT)
            row["stream_track_overlay"] = run_child([me, "--child", "track_overlay", "--root", root, "--inter",
                                                     os.path.join(root, f"on{k}", "intermediate")], a.limit, ROOT)
            ref = row.get("baseline_stream_track", row["stream_track"])
            row["overlay_over_reference_frames_per_s"] = round(row["stream_track_overlay"]["frames_per_s"] / ref["frames_per_s"], 4)
            row["reference"] = "baseline tree" if a.baseline_tree else "this tree without the flag"
            rep["stream"].append(row)
            for tag in ("base", "off", "on"):
                shutil.rmtree(os.path.join(root, f"{tag}{k}"), ignore_errors=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    huff = rep["kernel"]["blend_fused"]["host_huffman_ms_per_frame_one_thread"]["median"]
    period = statistics.mean(1e3 / r["stream_track_overlay"]["frames_per_s"] for r in rep["stream"]) if rep["stream"] else None
    lines = ["tools/time_jpeg_encode.py -- 480x854, 4:2:0, quality 95", ""]
    for tag in ("plain", "blend_fused"):
        kr = rep["kernel"][tag]
        lines.append(f"forward kernel, {tag}: {kr['forward_us_per_launch']['median']} us per launch (min {kr['forward_us_per_launch']['min']}, max "
                     f"{kr['forward_us_per_launch']['max']}; {REPEATS} windows of {LAUNCHES} back-to-back launches, device events), "
                     f"{kr['compulsory_bytes']} compulsory bytes = {kr['gb_per_s_of_compulsory_bytes']} GB/s; sclk {kr['box'].get('sclk_mhz_mean')} MHz")
        lines.append(f"host Huffman pass, {tag}: {kr['host_huffman_ms_per_frame_one_thread']['median']} ms per frame on one thread, "
                     f"{kr['file_bytes']} bytes per file")
    for k, row in enumerate(rep["stream"]):
        lines.append(f"alternation {k}: " + ", ".join(f"{name} {row[name]['frames_per_s']} frames/s (sclk {row[name]['box'].get('sclk_mhz_mean')} MHz)"
                                                     for name in ("baseline_stream_track", "stream_track", "stream_track_overlay") if name in row)
                     + f"; --overlay / {row['reference']} = {row['overlay_over_reference_frames_per_s']}")
    if period is not None:
        lines.append(f"one writer thread's Huffman pass: {huff} ms per frame; frame period of stream --track --overlay: {round(period, 2)} ms -> "
                     + ("the Huffman pass on the writer bounds the flag" if huff > period else "the merge loop bounds the flag, not the Huffman pass"))
    text = "\n".join(lines) + "\n\n" + json.dumps(rep, indent=1) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
