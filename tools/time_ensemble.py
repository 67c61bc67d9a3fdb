#!/usr/bin/env python
"""What the ensemble vote (premvos_idmap_vote_u8, `track.vote_idmaps`) costs: ONE vote of 8 id-map sets over a 100-frame 480x854 stack
-- the size `track --prewarp --ensemble` and `python -m premvos_amd.ensemble` vote per video -- timed with hipEvent pairs on the stream
the kernel runs on, after a warm-up: every launch of a series between its own pair (median, minimum, maximum) and the whole series
between one pair (launches back to back, the window long enough not to measure the clock's ramp).  The bytes the algorithm needs, from
the shapes: K bytes read and 2 written per pixel (the voted label and its votes; `hist` is K + 1 numbers).  Bytes / time stands next to
the float4 copy of the same call (`bench.hbm_ceiling`, 1 GiB -> 1 GiB) and to the 6.29 TB/s copy ceiling bench.py records.  The 328 MB
of maps exceed the 256 MB Infinity Cache, the 82 MB of outputs do not: the rate is the kernel's on this stack, not a pure HBM figure.

    python tools/time_ensemble.py [--sets 8] [--frames 100] [--reps 200] [--out profiles/ensemble.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_GB_S = 6290.0                                                    # bench.py's recorded float4-copy ceiling on an MI355X


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    import torch
    import bench
    from premvos_amd import _lib, track
    _lib.require_gpu()
    dev = _lib.resolve_device()
    K, N, h, w = a.sets, a.frames, a.height, a.width
    pixels = N * h * w
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.randint(0, 4, (N, h, w), dtype=torch.uint8, device=dev, generator=g)          # members that mostly agree, as real ones do
    maps = base.unsqueeze(0).repeat(K, 1, 1, 1)
    for k in range(1, K):
        differ = torch.rand((N, h, w), device=dev, generator=g) < 0.05
        maps[k][differ] = torch.randint(0, 4, (int(differ.sum()),), dtype=torch.uint8, device=dev, generator=g)
    out = {"voted": torch.empty((N, h, w), dtype=torch.uint8, device=dev), "votes": torch.empty((N, h, w), dtype=torch.uint8, device=dev),
           "hist": torch.zeros((K + 1,), dtype=torch.int64, device=dev)}

    def vote():
        track.vote_idmaps(maps, out=out["voted"], votes=out["votes"], hist=out["hist"])
    for _ in range(10):
        vote()
    torch.cuda.synchronize()
    out["hist"].zero_()
    vote()
    hist = out["hist"].cpu().tolist()
    assert sum(hist) == pixels and hist[0] == 0, hist
    with bench.BoxSampler(dev.index) as box:
        each = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            vote()
            e1.record()
            e1.synchronize()
            each.append(e0.elapsed_time(e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10 * a.reps):
            vote()
        e1.record()
        e1.synchronize()
        series_ms = e0.elapsed_time(e1) / (10 * a.reps)
    s = box.summary()
    copy_gb_s = bench.hbm_ceiling()
    each.sort()
    moved = (K + 2) * pixels
    rate = lambda ms: round(moved / (ms * 1e-3) / 1e9, 1)  # noqa: E731
    res = {"what": f"one premvos_idmap_vote_u8 launch over {K} sets of {N} x {h} x {w} id maps (voted + votes + hist), hipEvent pairs after 10 warm-up "
                   f"launches; {a.reps} launches timed one by one, then {10 * a.reps} back to back between one pair",
           "sets": K, "frames": N, "h": h, "w": w, "pixels": pixels, "bytes_moved": moved, "bytes_rule": "(K + 2) bytes per pixel: K read, 2 written",
           "ms_median": round(each[len(each) // 2], 4), "ms_min": round(each[0], 4), "ms_max": round(each[-1], 4),
           "ms_per_launch_back_to_back": round(series_ms, 4),
           "GB_per_s_median": rate(each[len(each) // 2]), "GB_per_s_back_to_back": rate(series_ms),
           "copy_GB_per_s_this_call": copy_gb_s, "copy_ceiling_GB_per_s_bench": COPY_CEILING_GB_S,
           "share_of_copy_ceiling_median": round(rate(each[len(each) // 2]) / COPY_CEILING_GB_S, 4),
           "unanimous": round(hist[K] / pixels, 4), "hist": hist,
           "sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean"),
           "not_measured": "rocprofv3 kernel time, other K / sizes, the unaligned path"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
