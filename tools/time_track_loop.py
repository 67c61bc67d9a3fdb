#!/usr/bin/env python
"""What the package's own merge loop (premvos_amd.track.Tracker) costs per frame, by the protocol of tools/time_merge_loop.py: one
synthetic 480x854 video, sequential in t, masks resident in HBM, 3 warm-up frames, a synchronise before every clock read, a second,
instrumented pass for the phase split (syncs added).  Per frame the tracker does strictly more than the merge-shaped loop of that
tool: it decodes the frame's fresh proposals from their RLE, scores them (mask / ReID / warp terms) against the templates, selects,
removes overlaps, copies the id map to the host (the PNG writer's input), warps, refines the warped boxes AND embeds them (ReID).

    per frame:  decode(fresh RLE) -> overlap counts -> scores + selection -> paint -> id map D2H -> warp + run boundaries + boxes
                -> refinement of the warped boxes (graph replay) -> ReID of the same boxes -> templates := candidates

The condition this tool checks: decode + overlap + scores + paint per frame cost less than the `refine` phase, i.e. the new logic is
not what binds the loop.  `host_restatement_ms_per_frame` (the numpy restatement of the four, on a few frames) is a BASELINE for
context, never a target.

`--combine probabilistic` / `--oracle` time the loop's two opt-in modes on the same video: the phases become
overlap + scores + combine, resp. label_overlap + gt_scores + paint; the oracle's "annotation" is the first frame's objects as one id
map, resident in HBM (its content does not change the cost).  The condition is the same, against the `refine` phase of the same run.

`--viz` times the loop with the score sheets on (``Tracker(viz=True)``): the phase `sheet` is the extra label overlap + IoU
scores, premvos_viz_scores_u8 and the device half of the sheet's JPEG; the Huffman pass runs on a writer thread, as in ``do_video``, and
one sheet's pass is timed alone (`sheet_huffman_ms`).  The sheets are coded and dropped, not written.

    python tools/time_track_loop.py [--frames 64] [--objects 10] [--candidates 20] [--combine probabilistic] [--oracle] [--viz] [--out track_loop.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--objects", type=int, default=10)
    ap.add_argument("--candidates", type=int, default=20, help="fresh proposals of every frame (RLE + score + 128-d embedding)")
    ap.add_argument("--host-frames", type=int, default=4, help="frames of the host restatement baseline (0: none)")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--combine", default="argmax", choices=("argmax", "probabilistic"), help="Tracker(combine=...)")
    ap.add_argument("--oracle", action="store_true", help="Tracker(oracle=True): scores against an id map of the first frame's objects")
    ap.add_argument("--viz", action="store_true", help="Tracker(viz=True): a score sheet per frame, coded as JPEG on a writer thread")
    a = ap.parse_args()
    from oracle import reid_oracle as QO
    from premvos_amd import _lib, rle, synth, track
    from premvos_amd.refinement import RefinementNet
    from premvos_amd.refinement.driver import RefinementEngine
    from premvos_amd.reid import ReIDEngine, ReIDNet
    H, W, T, N = 480, 854, a.frames, a.objects
    dev = _lib.resolve_device()
    frames = synth.clip_frames(0, T + 1, H, W).to(dev)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flows = torch.from_numpy(np.stack([np.stack([2.5 * np.sin(yy / 97.0 + 0.1 * t) + 1.25, 1.5 * np.cos(xx / 131.0 - 0.07 * t) - 0.5], -1)
                                       for t in range(T)]).astype(np.float32)).to(dev)

    def box_mask(b):
        m = np.zeros((H, W), np.uint8)
        y0, x0, y1, x1 = (int(v) for v in b)
        m[y0:max(y1, y0 + 1), x0:max(x1, x0 + 1)] = 1
        return m
    cand_boxes = synth.clip_boxes(0, T, a.candidates, H, W).numpy()
    fresh = [[{"segmentation": rle.encode(box_mask(b)), "score": round(float(rng.uniform(0.5, 1.0)), 2),
               "ReID": rng.normal(0, 0.3, 128).round(4).tolist()} for b in cand_boxes[t]] for t in range(T)]
    if a.viz:                                                    # (the JSON's 'bbox': x, y, w, h)
        for t in range(T):
            for p, b in zip(fresh[t], cand_boxes[t]):
                p["bbox"] = [float(b[1]), float(b[0]), float(max(b[3] - b[1], 1)), float(max(b[2] - b[0], 1))]
    start = [{"segmentation": rle.encode(box_mask(b)), "score": 1.0, "id": i + 1, "ReID": rng.normal(0, 0.3, 128).round(4).tolist()}
             for i, b in enumerate(synth.boxes(1, N, H, W, rank=99)[0].numpy())]
    ref_eng = RefinementEngine(RefinementNet(synth.refinement_weights(0), 16, dev))
    reid_eng = ReIDEngine(ReIDNet(QO.synth_weights(0), dev))
    gt = None
    if a.oracle or a.viz:
        ann = np.zeros((H, W), np.uint8)
        for p in start[::-1]:
            ann[rle.decode(p["segmentation"]) != 0] = p["id"]
        gt = torch.from_numpy(ann).to(dev)
    logic = ("decode", "overlap", "scores", "label_overlap", "gt_scores", "paint", "combine")      # (a mode's unused phases stay 0)
    if a.viz:
        logic = logic + ("sheet",)
    phases = {k: 0.0 for k in logic + ("idmap_d2h", "warp+rle+bbox", "refine", "reid")}
    clock = [0.0]

    def tick(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        phases[name] += now - clock[0]
        clock[0] = now

    def new_tracker():
        tr = track.Tracker(ref_eng, reid_eng, combine=a.combine, oracle=a.oracle, viz=a.viz)
        tr.add_templates([dict(p) for p in start], None)
        if a.viz:
            from premvos_amd import jpeg, viz
            tr.on_sheet = lambda sheet: (last_sheet.__setitem__(0, sheet), writer.submit(jpeg.entropy_encode, viz.forward(sheet)))
        return tr
    last_sheet = [None]
    writer = None
    if a.viz:
        from premvos_amd import io_pipeline as iop
        writer = iop.Writer()

    def one_frame(tr, t, timed):
        if timed:
            torch.cuda.synchronize()
            clock[0] = time.perf_counter()
        r = tr.step([dict(p) for p in fresh[t]], flows[t], frames[t + 1], gt=gt, **({"frame": frames[t]} if a.viz else {}))
        png = r["idmap"].cpu()                                   # what the PNG writer thread takes
        if timed:
            tick("idmap_d2h")
        return png
    tr = new_tracker()
    for t in range(3):                                           # warm-up: plans / graphs of the bucket, allocator
        one_frame(tr, t, False)
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for t in range(T):
        one_frame(tr, t, False)
    torch.cuda.synchronize()
    if writer is not None:
        writer.close()                                           # (the run ends when the last sheet is coded)
    dt = time.perf_counter() - t_all
    if a.viz:
        writer = iop.Writer()
    n_ph = min(T, 32)
    tr.timer = tick
    for t in range(n_ph):
        one_frame(tr, t, True)
    tr.timer = None
    huffman_ms = None
    if a.viz:
        from premvos_amd import jpeg, viz
        writer.close()
        enc = viz.forward(last_sheet[0])
        enc.ready.synchronize()
        t0 = time.perf_counter()
        n_bytes = len(jpeg.entropy_encode(enc))
        huffman_ms = round(1e3 * (time.perf_counter() - t0), 3)
    ph = {k: round(1e3 * v / n_ph, 3) for k, v in phases.items()}
    new_logic = round(sum(ph[k] for k in logic), 3)
    host_ms = None
    if a.host_frames and a.combine == "argmax" and not a.oracle:                                            # the numpy restatement of decode + overlap + scores + paint: a baseline
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import track_restated as R
        templ = [dict(p) for p in start]
        t0 = time.perf_counter()
        for t in range(a.host_frames):
            props = templ + [dict(p) for p in fresh[t]]
            planes = R.calculate_scores(props, templ)
            weighted = R.weighted_from_planes(planes)
            sel, _ = R.calculate_selected_props(props, weighted, templ, R.SCORE_THRESH, planes[0] + planes[1])
            R.remove_mask_overlap(sel)
        host_ms = round(1e3 * (time.perf_counter() - t0) / a.host_frames, 1)
    out = {"what": "premvos_amd.track.Tracker, sequential in t, one synthetic 480x854 video: decode of the fresh RLE proposals -> overlap -> "
                   f"scores + selection -> paint -> id map to the host -> warp -> refinement + ReID of the {N} warped boxes",
           "combine": a.combine, "oracle": bool(a.oracle), "frames": T, "objects": N, "candidates": a.candidates, "frames_per_s_one_video": round(T / dt, 2),
           "ms_per_frame": round(1e3 * dt / T, 3), "phase_ms_per_frame_with_syncs": ph,
           "new_logic_ms_per_frame": new_logic, "refine_ms_per_frame": ph["refine"],
           "new_logic_cheaper_than_refine": bool(new_logic < ph["refine"]),
           "host_restatement_ms_per_frame": host_ms,
           **({"viz": True, "sheet_ms_per_frame": ph["sheet"], "sheet_cheaper_than_refine": bool(ph["sheet"] < ph["refine"]),
               "sheet_shape": list(last_sheet[0].shape), "sheet_jpeg_bytes": n_bytes, "sheet_huffman_ms": huffman_ms} if a.viz else {}),
           "note": "phase times come from the instrumented pass (a synchronise per phase); `idmap_d2h` there is the copy alone"}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
