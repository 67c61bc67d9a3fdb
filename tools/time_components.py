#!/usr/bin/env python
"""What the largest-component clean-up (csrc/components_ops.hip, `premvos_amd.components`) costs on 480x854 id maps: the three entries
(premvos_cc_dilate_u8, premvos_cc_label_i32 of the dilated planes, premvos_cc_keep_largest_u8) and the whole of
`components.keep_largest`, on ONE synthetic frame and on a stack of 32, with 2, 4 and 8 objects at D = 100, timed with hipEvent pairs on
the stream the kernels run on, after a warm-up: every repetition between its own pair (median, minimum, maximum).  Also recorded: the
labelling alone on the worst case of propagation schemes, a snake of the frame's size; the time of the scipy restatement
(tests/components_restated.py) on the first frame on the CPU, for scale only; and that the GPU's maps equal the restatement's there.

    python tools/time_components.py [--reps 10] [--out profiles/components.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECKLE = 2e-5          # stray pixels per pixel (about 8 a frame): at the tests' 1 % the boxes of D = 100 would cover the whole frame
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=854)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dilate", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import components_restated as X
    from premvos_amd import _lib, components
    _lib.require_gpu()
    dev = _lib.resolve_device()
    lib = _lib.load()
    H, W, D = a.height, a.width, a.dilate
    cases = []
    with bench.BoxSampler(dev.index) as box:
        for objects in (2, 4, 8):
            L = objects + 1
            host = np.stack([X.synthetic(H, W, L, seed, speckle=SPECKLE) for seed in range(32)])
            t0 = time.perf_counter()
            want = X.keep_largest(host[0], L, D)
            restated_ms = (time.perf_counter() - t0) * 1e3
            for n in (1, 32):
                maps = torch.from_numpy(host[:n]).to(dev)
                dil = components.dilate(maps, L, D)
                labels = components.label(dil.reshape(-1, H, W)).reshape(dil.shape)
                counts = torch.empty_like(labels)
                out = torch.empty_like(maps)
                removed, ncomp = (torch.empty((n, L - 1), dtype=torch.int32, device=dev) for _ in range(2))
                s = _lib.current_stream()

                def entry_dilate():
                    _lib.check(lib.premvos_cc_dilate_u8(maps.data_ptr(), n, H, W, L, D, dil.data_ptr(), s), "cc_dilate")

                def entry_label():
                    _lib.check(lib.premvos_cc_label_i32(dil.data_ptr(), n * (L - 1), H, W, labels.data_ptr(), s), "cc_label")

                def entry_keep():
                    _lib.check(lib.premvos_cc_keep_largest_u8(maps.data_ptr(), labels.data_ptr(), n, H, W, L, counts.data_ptr(), out.data_ptr(),
                                                              removed.data_ptr(), ncomp.data_ptr(), s), "cc_keep_largest")

                for _ in range(2):                                                              # warm-up: every kernel of the timed windows
                    entry_dilate(), entry_label(), entry_keep()
                    res = components.keep_largest(maps, L, D)
                torch.cuda.synchronize()
                same = bool(np.array_equal(res["idmap"][0].cpu().numpy(), want["idmap"]) and res["removed"][0].tolist() == want["removed"].tolist()
                            and res["components"][0].tolist() == want["components"].tolist() and torch.equal(out, res["idmap"]))
                cases.append({"objects": objects, "L": L, "D": D, "frames": n, "planes": n * (L - 1),
                              "dilate": _timed(entry_dilate, a.reps), "label": _timed(entry_label, a.reps), "keep_largest_entry": _timed(entry_keep, a.reps),
                              "keep_largest_whole": _timed(lambda: components.keep_largest(maps, L, D), a.reps),
                              "restated_first_frame_cpu_ms": round(restated_ms, 1), "first_frame_equals_restatement": same,
                              "removed_share_of_foreground": round(float(res["removed"].sum()) / max(1, int((maps > 0).sum())), 5)})
                print(json.dumps(cases[-1]), flush=True)
        m = np.zeros((H, W), np.uint8)                                                          # a snake: one component, the longest path
        m[0::2] = 1
        for j, y in enumerate(range(1, H, 2)):
            m[y, W - 1 if j % 2 == 0 else 0] = 1
        snake = torch.from_numpy(m).to(dev)
        lab = components.label(snake)
        torch.cuda.synchronize()
        snake_case = {"pixels": int(m.sum()), "one_component": bool(((lab == 0) == (snake != 0)).all()),
                      "label": _timed(lambda: components.label(snake), a.reps)}
    smp = box.summary()
    res = {"what": f"the largest-component clean-up on {H} x {W} id maps (tests/components_restated.py's synthetic maps with {SPECKLE} stray pixels per pixel, seeds 0..31): hipEvent "
                   f"pairs around each call after 2 warm-up calls, {a.reps} repetitions; D = {D}",
           "h": H, "w": W, "cases": cases, "snake": snake_case,
           "sclk_mhz_mean": (smp.get("sclk_mhz_mean_of_xcds") or {}).get("mean"), "socket_power_w_mean": (smp.get("socket_power_w") or {}).get("mean"),
           "not_measured": "rocprofv3 kernel times, more than 8 objects, real id maps, the command with its PNG decoding and writing, DAVIS quality"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
