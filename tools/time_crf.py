#!/usr/bin/env python
"""What the CRF boundary refinement (csrc/crf_ops.hip, `premvos_amd.crf`) costs on a 480x854 frame: the two normalisers, ONE mean-field
round (premvos_crf_step_f32) and the whole refinement of `crf.refine_idmaps` (unary, normalisers, 12 rounds, argmax), for L = 2, 4 and 8
labels at the default window (r = 56) and at r = 32, timed with hipEvent pairs on the stream the kernels run on, after a warm-up: every
repetition between its own pair (median, minimum, maximum).  One frame per call, and a stack of 4 frames for the per-frame cost when the
tiles of several frames fill the chip.  The work, from the shapes: pixels x (2r + 1)^2 pair weights per round for the bilateral kernel
(clipped windows counted whole), each one exponential and L multiply-adds.  Also recorded: on two of the tests' cases the largest
deviation of Q from the fp64 restatement (tests/crf_restated.py) next to d32, the same restatement's in fp32 on the CPU.

    python tools/time_crf.py [--reps 10] [--out profiles/crf.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, reps):
    import torch
    each = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        each.append(e0.elapsed_time(e1))
    each.sort()
    return {"ms_median": round(each[len(each) // 2], 4), "ms_min": round(each[0], 4), "ms_max": round(each[-1], 4)}


def _accuracy(dev):
    import torch
    import crf_restated as X
    from premvos_amd import crf
    out = []
    for H, W, L, kw in ((37, 53, 3, dict(gsxy=0.8, gr=2, sxy=3.0, srgb=10.0, r=6, gt_prob=0.5)), (70, 150, 3, dict())):
        frame, idmap = X.synthetic(H, W, L, 11)
        p = X.params(**kw)
        r64, r32 = X.refine(frame, idmap, L, p), X.refine(frame, idmap, L, p, torch.float32)
        u, _ = crf.unary_from_labels(idmap[None].to(dev), L, p["gt_prob"])
        q1 = crf.meanfield(frame[None].to(dev), u, crf.Params(**dict(p, iters=1)))[0].double().cpu()
        q = crf.meanfield(frame[None].to(dev), u, crf.Params(**p))[0].double().cpu()
        out.append({"h": H, "w": W, "L": L, "r": p["r"], "iters": p["iters"],
                    "d32_round_1": float((r32["Q1"].double() - r64["Q1"]).abs().max()), "d32_last_round": float((r32["Q"].double() - r64["Q"]).abs().max()),
                    "kernel_round_1": float((q1 - r64["Q1"]).abs().max()), "kernel_last_round": float((q - r64["Q"]).abs().max())})
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    import torch
    import bench
    import crf_restated as X
    from premvos_amd import _lib, crf
    _lib.require_gpu()
    dev = _lib.resolve_device()
    H, W = a.height, a.width
    cases = []
    with bench.BoxSampler(dev.index) as box:
        for L in (2, 4, 8):
            frame, idmap = X.synthetic(H, W, L, 11)
            for r, n in ((56, 1), (32, 1), (56, 4)):
                if n > 1 and L != 4:
                    continue
                p = crf.Params(r=r)
                frames, maps = frame[None].repeat(n, 1, 1, 1).to(dev), idmap[None].repeat(n, 1, 1).to(dev)
                u, q0 = crf.unary_from_labels(maps, L, p.gt_prob)
                n_g, n_b = crf.normalisers(frames, p)
                q1 = torch.empty_like(q0)
                for _ in range(2):                                                              # warm-up: every kernel of the timed windows
                    crf._step(frames, u, q0, n_g, n_b, p, q1)
                    res = crf.refine_idmaps(frames, maps, L, p)
                torch.cuda.synchronize()
                taps = n * H * W * (2 * r + 1) ** 2
                step = _timed(lambda: crf._step(frames, u, q0, n_g, n_b, p, q1), a.reps)
                cases.append({"L": L, "r": r, "gr": p.gr, "frames": n, "pair_weights_per_round": taps,
                              "norm_both": _timed(lambda: crf.normalisers(frames, p), a.reps), "step": step,
                              "refine_12_rounds": _timed(lambda: crf.refine_idmaps(frames, maps, L, p), max(3, a.reps // 2)),
                              "step_pair_weights_per_s": round(taps / (step["ms_median"] * 1e-3), -6),
                              "changed_share": round(float(res["changed"].sum()) / (n * H * W), 5)})
                print(json.dumps(cases[-1]), flush=True)
    s = box.summary()
    res = {"what": f"the CRF boundary refinement on {H} x {W} frames: hipEvent pairs around each call after 2 warm-up calls, {a.reps} repetitions "
                   "(refine: half as many); crf_davis.py:43-60's parameters, the window radius as listed",
           "h": H, "w": W, "cases": cases, "accuracy_vs_fp64_restatement": _accuracy(dev),
           "sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean"),
           "not_measured": "rocprofv3 kernel times, L = 16, videos (many frames per call), DAVIS quality"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
