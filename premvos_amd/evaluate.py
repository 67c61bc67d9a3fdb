"""The DAVIS-2017 measures (J region similarity, F contour accuracy, J&F) from integer counts made on the GPU -- the protocol of
tools/davis_eval.py (Pont-Tuset et al., arXiv:1704.00675, section 3) with the pixel work in ``premvos_davis_counts_u8``
(premvos_amd/csrc/davis_ops.hip): per object and frame the six integers |R&G|, |R|G|, |bR|, |bG|, |bR & dil(bG)|, |bG & dil(bR)|.
The floats are made of them on the host with the yardstick's own Python expressions, so the same counts give the same bits.

    python -m premvos_amd.evaluate --root <PReMVOS root> [--results output/final] [--annotations data/DAVIS/Annotations/480p]
                                   [--sequences a,b] [--check-only] [--collect]

prints J, F and J&F and writes output/premvos_amd_davis_eval.json.  ``--collect``: no GPU, the summary from the per-video count files
output/eval/<video>.json that ``premvos_amd.track --eval`` / ``premvos_amd.stream --track --eval`` wrote (``LoopEval`` below: the id
maps are scored where the paint kernel left them in HBM, one launch per frame on the tracker's stream, the counts copied back once
per video).

Out of scope, as in tools/davis_eval.py's palette path: void pixels, RGB renderings (a 3-D PNG is refused here)."""
from __future__ import annotations

import glob
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_RADIUS = 48                       # premvos_davis_counts_u8's limit (a 4K frame's radius is 36)
SUMMARY = "output/premvos_amd_davis_eval.json"
EVAL_DIR = "output/eval"


def bound_pix(h: int, w: int) -> int:
    """The disk radius of db_eval_boundary (tools/davis_eval.py:56) for an [h,w] frame."""
    return int(np.ceil(0.008 * np.linalg.norm((h, w))))


def davis_counts(result: torch.Tensor, gt: torch.Tensor, ids, radius: Optional[int] = None, maps: bool = False,
                 out: Optional[torch.Tensor] = None):
    """premvos_davis_counts_u8 -> int64 [N,T,6] CUDA tensor (and, ``maps``, the uint8 [N,T,4,h,w] maps bR, bG, bR & dil(bG),
    bG & dil(bR)).  ``result`` / ``gt``: uint8 [h,w] or [N,h,w] CUDA id maps; ``ids``: T object ids (a sequence or an int32 CUDA
    tensor); ``radius`` None: ``bound_pix(h, w)``; ``out``: an int64 [N,T,6] tensor to write into.  Queued on the current stream."""
    _lib.require_gpu()
    if result.dim() == 2:
        result, gt = result[None], gt[None]
    if result.shape != gt.shape:
        raise ValueError(f"result {tuple(result.shape)} and annotation {tuple(gt.shape)} differ in shape")
    assert result.dim() == 3 and result.dtype == torch.uint8 and gt.dtype == torch.uint8 and result.is_cuda and gt.device == result.device
    dev = result.device
    result, gt = result.contiguous(), gt.contiguous()
    idt = ids if isinstance(ids, torch.Tensor) else torch.tensor([int(i) for i in ids], dtype=torch.int32, device=dev)
    assert idt.dtype == torch.int32 and idt.device == dev and idt.is_contiguous()
    N, h, w = (int(v) for v in result.shape)
    T = int(idt.shape[0])
    r = bound_pix(h, w) if radius is None else int(radius)
    counts = torch.empty((N, T, 6), dtype=torch.int64, device=dev) if out is None else out
    assert counts.is_contiguous() and tuple(counts.shape) == (N, T, 6) and counts.dtype == torch.int64 and counts.device == dev
    m = torch.empty((N, T, 4, h, w), dtype=torch.uint8, device=dev) if maps else None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().premvos_davis_counts_u8(result.data_ptr(), gt.data_ptr(), N, h, w, idt.data_ptr() if T else None, T, r,
                                                       counts.data_ptr() if N * T else None, m.data_ptr() if maps and N * T else None,
                                                       _lib.current_stream()), "davis_counts")
    return (counts, m) if maps else counts


def _j(c) -> float:
    """db_eval_iou (tools/davis_eval.py:25-30) from |R&G|, |R|G|."""
    inter, union = int(c[0]), int(c[1])
    if union == 0:
        return 1.0
    return float(inter) / float(union)


def _f(c) -> float:
    """db_eval_boundary (tools/davis_eval.py:62-71) from |bR|, |bG|, |bR & dil(bG)|, |bG & dil(bR)|."""
    n_fg, n_gt, fg_match, gt_match = int(c[2]), int(c[3]), int(c[4]), int(c[5])
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = float(fg_match) / n_fg, float(gt_match) / n_gt
    return 0.0 if precision + recall == 0 else 2.0 * precision * recall / (precision + recall)


def measures(counts) -> Tuple[np.ndarray, np.ndarray]:
    """int [N,T,6] counts (tensor or array) -> (J, F) float64 [N,T] on the host."""
    c = counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.reshape((-1,) + c.shape[-2:]) if c.ndim != 3 else c
    N, T = c.shape[:2]
    J, F = np.empty((N, T), np.float64), np.empty((N, T), np.float64)
    for n in range(N):
        for t in range(T):
            J[n, t], F[n, t] = _j(c[n, t]), _f(c[n, t])
    return J, F


def sequence_means(ids: Sequence[int], counts) -> Dict[int, Tuple[float, float]]:
    """{id: (mean J, mean F)} over the frames of ``counts`` [N,T,6], as evaluate_sequence (tools/davis_eval.py:105) takes the means."""
    J, F = measures(counts)
    return {int(i): (float(np.mean([float(v) for v in J[:, t]])), float(np.mean([float(v) for v in F[:, t]]))) for t, i in enumerate(ids)}


def _table(per_seq: "Dict[str, Dict[int, Tuple[float, float]]]") -> dict:
    """tools/davis_eval.py:111-119: the dict ``evaluate`` returns, from {sequence: {id: (mean J, mean F)}} in sequence order."""
    js, fs, table = [], [], {}
    for s, r in per_seq.items():
        table[s] = {str(i): {"J": round(j, 5), "F": round(f, 5)} for i, (j, f) in r.items()}
        js += [j for j, _ in r.values()]
        fs += [f for _, f in r.values()]
    mj, mf = (float(np.mean(js)) if js else math.nan), (float(np.mean(fs)) if fs else math.nan)
    return {"mean_J": round(mj, 5), "mean_F": round(mf, 5), "mean_JF_percent": round(50.0 * (mj + mf), 4), "objects": len(js),
            "sequences": len(per_seq), "per_sequence": table}


class SequenceEval:
    """One video's counts: ``add`` queues frame k's launch into row k of an int64 [N,T,6] tensor, ``finish`` -> {id: (mean J, mean F)}.
    ``ids``: the object ids (of the first annotation); ``names``: the N evaluated frames."""

    def __init__(self, ids: Sequence[int], names: Sequence[str], radius: Optional[int] = None):
        self.ids, self.names, self.radius = [int(i) for i in ids], list(names), radius
        self.counts: Optional[torch.Tensor] = None
        self._ids_dev: Optional[torch.Tensor] = None

    def add(self, k: int, result_dev: torch.Tensor, gt_dev: torch.Tensor) -> None:
        assert 0 <= k < len(self.names)
        if self.counts is None:
            dev = result_dev.device
            self.counts = torch.zeros((len(self.names), len(self.ids), 6), dtype=torch.int64, device=dev)
            self._ids_dev = torch.tensor(self.ids, dtype=torch.int32, device=dev)
        if self.ids:
            davis_counts(result_dev, gt_dev, self._ids_dev, self.radius, out=self.counts[k:k + 1])

    def finish(self) -> Dict[int, Tuple[float, float]]:
        counts = np.zeros((len(self.names), len(self.ids), 6), np.int64) if self.counts is None else self.counts
        return sequence_means(self.ids, counts)


# ------------------------------------------------------------------------------------------------------------- the file protocol
def _read_ids(fn: str) -> np.ndarray:
    """A palette PNG's object ids as uint8 [h,w]."""
    from PIL import Image
    a = np.asarray(Image.open(fn))
    if a.ndim == 3:
        raise ValueError(f"{fn}: not a palette PNG (an array of shape {a.shape}); RGB renderings are scored by tools/davis_eval.py only")
    if a.dtype != np.uint8:
        if a.size and (a.max() > 255 or a.min() < 0):
            raise ValueError(f"{fn}: object ids beyond 255 do not fit the id maps scored here; use tools/davis_eval.py")
        a = a.astype(np.uint8)
    return a


def _load_sequence(result_dir: str, annotation_dir: str, pool):
    """evaluate_sequence's reads (tools/davis_eval.py:88-101) -> (ids, names, results [N,h,w], annotations [N,h,w]) uint8 arrays."""
    ann_files = sorted(glob.glob(os.path.join(annotation_dir, "*.png")))
    if len(ann_files) < 3:
        raise ValueError(f"{annotation_dir}: need at least three annotated frames")
    ids = [int(i) for i in np.unique(_read_ids(ann_files[0])) if i != 0]
    mid = ann_files[1:-1]                                             # first and last frame are excluded (semi-supervised protocol)
    res_files = [os.path.join(result_dir, os.path.basename(fn)) for fn in mid]
    read = (lambda fn: _read_ids(fn) if os.path.exists(fn) else None)
    arrays = list(pool.map(read, mid + res_files)) if pool is not None else [read(fn) for fn in mid + res_files]
    gts, ress = arrays[:len(mid)], arrays[len(mid):]
    for k, (g, r) in enumerate(zip(gts, ress)):
        if r is None:
            ress[k] = np.zeros_like(g)                                # a frame without a result file counts as an empty map
        elif r.shape != g.shape:
            raise ValueError(f"{res_files[k]}: shape {r.shape} differs from the annotation's {g.shape}")
    return ids, [os.path.splitext(os.path.basename(fn))[0] for fn in mid], ress, gts


def _sequence_counts(ids: List[int], ress: List[np.ndarray], gts: List[np.ndarray], dev) -> np.ndarray:
    """One upload, one launch, one copy back per frame size of the sequence (DAVIS: one) -> int64 [N,T,6] on the host."""
    counts = np.zeros((len(gts), len(ids), 6), np.int64)
    if not ids:
        return counts
    for shape in sorted({g.shape for g in gts}):
        rows = [k for k, g in enumerate(gts) if g.shape == shape]
        both = torch.from_numpy(np.stack([np.stack([ress[k] for k in rows]), np.stack([gts[k] for k in rows])])).to(dev)
        counts[rows] = davis_counts(both[0], both[1], ids).cpu().numpy()
    return counts


def evaluate(results_root: str, annotations_root: str, sequences: Optional[List[str]] = None, device=None) -> dict:
    """tools/davis_eval.py:108-119 ``evaluate`` with the pixel work on the GPU: the same dict."""
    from . import io_pipeline as iop
    _lib.require_gpu()
    dev = _lib.resolve_device(device)
    seqs = sequences or sorted(d for d in os.listdir(annotations_root) if os.path.isdir(os.path.join(results_root, d)))
    per_seq: Dict[str, Dict[int, Tuple[float, float]]] = {}
    workers = iop.io_threads()
    pool = iop.thread_pool(workers, "premvos-eval") if workers > 0 else None
    try:
        for s in seqs:
            ids, _, ress, gts = _load_sequence(os.path.join(results_root, s), os.path.join(annotations_root, s), pool)
            per_seq[s] = sequence_means(ids, _sequence_counts(ids, ress, gts, dev))
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
    return _table(per_seq)


# ----------------------------------------------------------------------------------------------------------- inside the merge loop
def write_video_file(fn: str, video: str, names: Sequence[str], ids: Sequence[int], counts: np.ndarray) -> None:
    """output/eval/<video>.json: frame names, ids, the integer counts [N][T][6] and the per-object means made of them."""
    r = sequence_means(ids, counts)
    os.makedirs(os.path.dirname(fn) or ".", exist_ok=True)
    with open(fn + ".tmp", "w") as f:
        json.dump({"video": video, "frames": list(names), "ids": [int(i) for i in ids], "counts": np.asarray(counts).tolist(),
                   "J": {str(i): j for i, (j, _) in r.items()}, "F": {str(i): v for i, (_, v) in r.items()}}, f)
    os.replace(fn + ".tmp", fn)


class LoopEval:
    """What ``Tracker.evaluator`` is: one video's annotations in HBM (read on the host once, one upload) and its ``SequenceEval``.
    The driver names the frame (``expect``), the tracker hands over the id map it has just painted (``frame``: one launch on the
    current stream, nothing waits); ``fetch`` queues the counts' copy into a page-locked buffer and records an event, ``dump``
    (the writer thread) waits for it and writes the video's file."""

    def __init__(self, video: str, annotation_dir: str, device=None):
        from . import io_pipeline as iop
        self.video = video
        self.device = _lib.resolve_device(device)
        ann_files = sorted(glob.glob(os.path.join(annotation_dir, "*.png")))
        if len(ann_files) < 3:
            raise ValueError(f"{annotation_dir}: need at least three annotated frames")
        ids = [int(i) for i in np.unique(_read_ids(ann_files[0])) if i != 0]
        mid = ann_files[1:-1]
        workers = iop.io_threads()
        if workers > 0:
            with iop.thread_pool(workers, "premvos-eval") as pool:
                gts = list(pool.map(_read_ids, mid))
        else:
            gts = [_read_ids(fn) for fn in mid]
        if len({g.shape for g in gts}) != 1:
            raise ValueError(f"{annotation_dir}: the annotated frames differ in size")
        names = [os.path.splitext(os.path.basename(fn))[0] for fn in mid]
        self.gt = torch.from_numpy(np.stack(gts)).to(self.device)
        self.seq = SequenceEval(ids, names)
        self._row = {nm: k for k, nm in enumerate(names)}
        self._seen = set()
        self._name: Optional[str] = None
        self._host = self._event = None

    @classmethod
    def open(cls, video: str, annotation_dir: str, device=None) -> "Optional[LoopEval]":
        """The video's evaluator, or None (with a line in the log) when it has fewer than three annotated frames."""
        if len(glob.glob(os.path.join(annotation_dir, "*.png"))) < 3:
            print(f"premvos_amd.evaluate: {video}: fewer than three annotated frames in {annotation_dir}, not evaluated")
            return None
        return cls(video, annotation_dir, device)

    def expect(self, name: str) -> None:
        self._name = name

    def frame(self, idmap: torch.Tensor) -> None:
        k = self._row.get(self._name)
        self._name = None
        if k is None:                                                 # the first / last annotated frame, or a frame without annotation
            return
        if tuple(idmap.shape) != tuple(self.gt.shape[1:]):
            raise ValueError(f"{self.video}/{self.seq.names[k]}: shape {tuple(idmap.shape)} differs from the annotation's "
                             f"{tuple(self.gt.shape[1:])}")
        self.seq.add(k, idmap, self.gt[k])
        self._seen.add(k)

    def fetch(self) -> "LoopEval":
        """After the video's last frame, on the tracker's stream: annotated frames that never came count as empty maps."""
        empty = None
        for k in range(len(self.seq.names)):
            if k not in self._seen:
                empty = torch.zeros_like(self.gt[0]) if empty is None else empty
                self.seq.add(k, empty, self.gt[k])
                self._seen.add(k)
        N, T = len(self.seq.names), len(self.seq.ids)
        self._host = torch.zeros((N, T, 6), dtype=torch.int64).pin_memory()
        if self.seq.counts is not None:
            self._host.copy_(self.seq.counts, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(self.device))
        return self

    def dump(self, eval_dir: str) -> None:
        self._event.synchronize()
        write_video_file(os.path.join(eval_dir, self.video + ".json"), self.video, self.seq.names, self.seq.ids, self._host.numpy())


def summarise(eval_dir: str, sequences: Optional[List[str]] = None) -> dict:
    """Host only: the dict of ``evaluate`` from the per-video count files of ``eval_dir`` (sorted by video, or ``sequences``)."""
    names = sequences or sorted(os.path.splitext(os.path.basename(fn))[0] for fn in glob.glob(os.path.join(eval_dir, "*.json")))
    per_seq = {}
    for s in names:
        with open(os.path.join(eval_dir, s + ".json")) as f:
            d = json.load(f)
        counts = np.asarray(d["counts"], np.int64).reshape(len(d["frames"]), len(d["ids"]), 6)
        per_seq[s] = sequence_means(d["ids"], counts)
    return _table(per_seq)


def write_summary(root: str, r: dict) -> str:
    fn = os.path.join(root, SUMMARY)
    os.makedirs(os.path.dirname(fn), exist_ok=True)
    with open(fn, "w") as f:
        json.dump(r, f, indent=1)
    return fn


# ---------------------------------------------------------------------------------------------------------------- command line
def check_inputs(root: str, results: str, annotations: str, collect: bool = False) -> List[str]:
    """-> what ``main`` would miss under ``root`` (empty = ready)."""
    if collect:
        d = os.path.join(root, EVAL_DIR)
        return [] if glob.glob(os.path.join(d, "*.json")) else [f"{d} holds no per-video count files (written by premvos_amd.track --eval "
                                                               "or premvos_amd.stream --track --eval)"]
    return [f"{os.path.join(root, rel)} is missing ({why})" for rel, why in
            ((results, "the final PNGs: run premvos_amd.stream --track or premvos_amd.track first"), (annotations, "the DAVIS annotations"))
            if not os.path.isdir(os.path.join(root, rel))]


def main(argv: Optional[List[str]] = None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=".")
    ap.add_argument("--results", default="output/final")
    ap.add_argument("--annotations", default="data/DAVIS/Annotations/480p")
    ap.add_argument("--sequences", default=None, help="comma-separated sequence names (default: every folder of --results that is annotated)")
    ap.add_argument("--check-only", action="store_true", help="name what is missing and stop")
    ap.add_argument("--collect", action="store_true", help=f"no GPU: the summary from the count files of {EVAL_DIR}/")
    a = ap.parse_args(argv)
    root = os.path.abspath(a.root)
    problems = check_inputs(root, a.results, a.annotations, a.collect)
    if problems:
        print("premvos_amd.evaluate: inputs are not ready:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print("premvos_amd.evaluate: inputs are in place")
        return 0
    seqs = a.sequences.split(",") if a.sequences else None
    if a.collect:
        r = summarise(os.path.join(root, EVAL_DIR), seqs)
    else:
        r = evaluate(os.path.join(root, a.results), os.path.join(root, a.annotations), seqs)
    print(json.dumps({k: v for k, v in r.items() if k != "per_sequence"}, indent=1))
    print(f"premvos_amd.evaluate: J {r['mean_J']}  F {r['mean_F']}  J&F {r['mean_JF_percent']}  ->  {write_summary(root, r)}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
