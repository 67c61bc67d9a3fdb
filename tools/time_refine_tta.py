#!/usr/bin/env python
"""What test-time augmentation of the refinement net costs (``RefinementNet(tta=...)``, ``track --refine-tta``): one MI355X, the
full-depth net (num_middle = 16, synthetic weights), 20 boxes on a 480x854 frame, the plan replayed as a HIP graph.  Timed with hipEvent
pairs on the stream the plan runs on, after a warm-up: every replay of a series between its own pair (median, minimum, maximum) and the
whole series between one pair.  The plain ``refine`` and the specs 1+flip, 0.75,1,1.25 and 0.75,1,1.25+flip, each with its ratio to
plain next to the FLOP model (1 + flip) x sum(scale^2) (2.0, 3.125, 6.25), the plan's arena bytes and the conv FLOPs the plan counts.
One eager pass per spec, every launch between its own pair, gives the share of time in the two new kernels (the ``tta_input:*`` and
``tta_output`` steps) and, per member body, the layers whose time exceeds the plain layer's time x the member's FLOP factor by most.
The mean shader clock over all timed regions is recorded (amdsmi, bench.BoxSampler).  Nothing here is a threshold.

    python tools/time_refine_tta.py [--boxes 20] [--reps 20] [--out profiles/refine_tta.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPECS = (None, "1+flip", "0.75,1,1.25", "0.75,1,1.25+flip")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--num-middle", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from oracle import refinement_oracle as RO
    from premvos_amd import _lib
    from premvos_amd.refinement import RefinementNet, tta
    _lib.require_gpu()
    dev = _lib.resolve_device()
    P, H, W, nm = a.boxes, a.height, a.width, a.num_middle
    weights = RO.synth_weights(0, nm)
    rng = np.random.default_rng(0)
    frame = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    wh = rng.uniform(40, 400, (P, 2))
    xy = rng.uniform(0, 1, (P, 2)) * (np.array([W, H]) - np.minimum(wh, [W, H]))
    boxes = torch.tensor(np.stack([xy[:, 1], xy[:, 0], np.minimum(xy[:, 1] + wh[:, 1], H), np.minimum(xy[:, 0] + wh[:, 0], W)], 1),
                         dtype=torch.float32).to(dev)

    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    rows, plain_steps = [], {}
    with bench.BoxSampler(dev.index) as box:
        for text in SPECS:
            spec = tta.resolve(text)
            net = RefinementNet(weights, nm, device=dev, tta=spec)
            p = net.refine(frame, boxes, max_boxes=P)                        # builds, tunes (table, then rule) and captures the plan
            assert p.graph is not None
            for _ in range(3):
                p.launch()
            torch.cuda.synchronize()
            each = []
            for _ in range(a.reps):
                e0, e1 = pair()
                e0.record()
                p.launch()
                e1.record()
                e1.synchronize()
                each.append(e0.elapsed_time(e1))
            e0, e1 = pair()
            e0.record()
            for _ in range(a.reps):
                p.launch()
            e1.record()
            e1.synchronize()
            series = e0.elapsed_time(e1) / a.reps
            ev = [pair() for _ in p.steps]                                   # one eager pass, every launch between its own pair
            for _ in range(2):
                for (s0, s1), (_, fn) in zip(ev, p.steps):
                    s0.record()
                    fn()
                    s1.record()
            torch.cuda.synchronize()
            steps = {n: s0.elapsed_time(s1) for (s0, s1), (n, _) in zip(ev, p.steps)}
            eager = sum(steps.values())
            new = {n: ms for n, ms in steps.items() if n.startswith("tta_input") or n == "tta_output"}
            each.sort()
            row = {"spec": "plain" if spec is None else str(spec), "members": 1 if spec is None else len(spec.members()),
                   "flop_model": 1.0 if spec is None else (2 if spec.flip else 1) * sum(s * s for s in spec.scales),
                   "ms_median": round(each[len(each) // 2], 3), "ms_min": round(each[0], 3), "ms_max": round(each[-1], 3),
                   "ms_back_to_back": round(series, 3), "launches": len(p.steps), "conv_gflop": round(sum(p.flops.values()) / 1e9, 1),
                   "arena_bytes": p.arena.report()["arena_bytes"], "outside_arena_bytes": p.arena.report()["outside_bytes"],
                   "ms_eager_sum": round(eager, 3), "ms_new_kernels": {n: round(ms, 4) for n, ms in new.items()},
                   "share_new_kernels": round(sum(new.values()) / eager, 5) if new else 0.0,
                   "conf_first": [round(float(v), 6) for v in p.conf[:2].cpu()]}
            if spec is None:
                plain_steps = steps
                row["ms_output_layer"] = round(steps["refine_output"], 4)
            else:
                bodies = {}
                nb = 2 if spec.flip else 1
                for scale in spec.scales:
                    tag = f"tta{tta.scale_dimension(385, scale)}/"
                    factor = nb * scale * scale
                    mine = {n.replace(tag, "", 1): ms for n, ms in steps.items() if tag in n}
                    excess = sorted(((ms - factor * plain_steps[n], n, ms, plain_steps[n]) for n, ms in mine.items() if n in plain_steps), reverse=True)
                    bodies[tag.rstrip("/")] = {"flop_factor": factor, "ms": round(sum(mine.values()), 3),
                                               "ms_plain_body_x_factor": round(factor * sum(plain_steps[n] for n in mine if n in plain_steps), 3),
                                               "largest_excess": [{"step": n, "ms": round(ms, 4), "ms_plain": round(pl, 4), "ms_over_model": round(x, 4)}
                                                                  for x, n, ms, pl in excess[:6]]}
                row["bodies"] = bodies
            rows.append(row)
            del p, net
            torch.cuda.empty_cache()
    s = box.summary()
    base = rows[0]
    for r in rows:
        r["ratio_to_plain_median"] = round(r["ms_median"] / base["ms_median"], 3)
        r["ratio_to_plain_back_to_back"] = round(r["ms_back_to_back"] / base["ms_back_to_back"], 3)
        r["ratio_over_flop_model"] = round(r["ratio_to_plain_median"] / r["flop_model"], 3)
    res = {"what": f"RefinementNet.refine of {P} boxes on a {H}x{W} frame, num_middle={nm}, synthetic weights, fp32, the plan replayed as a HIP graph: "
                   f"{a.reps} replays timed one by one after 3 warm-up replays, then {a.reps} back to back between one hipEvent pair; one eager pass "
                   "per spec with every launch between its own pair for the per-step figures (the second of two passes)",
           "boxes": P, "h": H, "w": W, "num_middle": nm, "rows": rows,
           "sclk_mhz_mean": (s.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (s.get("socket_power_w") or {}).get("mean"),
           "not_measured": "quality on DAVIS (no weights, no dataset here); rocprofv3 kernel times; other box counts and frame sizes; the bf16 modes (refused with a spec)"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
