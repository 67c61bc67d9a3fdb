"""The merge stage: MergeTrack/merge.py ``do_video`` and the functions of MergeTrack/merge_functions.py it calls, with the pixel and
score work in libpremvos_hip.so (csrc/track_ops.hip + the mask helpers of ``mergetrack``).  The reference's MergeTrack keeps working
unchanged on the trees this package writes; with this module the package can also finish the job alone:

    python -m premvos_amd.track --root <PReMVOS root> [--videos a,b] [--check-only] [--lockstep V]   ->  output/final/<video>/<frame>.png
                                [--overlay]                                                ->  output/overlay/<video>/<frame>.jpg
                                [--combine probabilistic] [--oracle]                       ->  output/final_prob/, final_oracle/, final_oracle_prob/
                                [--viz]                                                    ->  output/viz/<video>/<frame>.jpg
    python -m premvos_amd.track --root <PReMVOS root> [--videos a,b] --max-reid-distance   ->  output/max_reid_distance.json
    python -m premvos_amd.track --root <PReMVOS root> [--videos a,b] --search W [--seed S] ->  output/live_search.json
                                --live-weights a,b,c,d,e [--lockstep V] [--eval] ...       ->  output/final_weights/<video>/<frame>.png
                                --ensemble "a,b,c,d,e;a,b,c,d,e;..." [--prewarp] [--eval] ->  output/final_ensemble/<video>/<frame>.png
                                --ensemble-from output/live_search.json [--top K]          ->  (with --prewarp: output/final_prewarp_ensemble/)
                                --refine-tta 0.75,1,1.25+flip [any flag of the live loop]  ->  output/final_tta/ (final_weights_tta/, final_prob_tta/, ...)

``--refine-tta`` runs the loop's refinement net with DeepLab's multi-scale / flipped inference (premvos_amd.refinement.tta,
refinement_net/network/deeplab/model.py:84-160): every ``net.refine`` / ``refine_group`` of the loop then merges the members' probabilities.
``--ensemble`` runs 2 to 8 weight sets at once and writes their per-pixel vote (``EnsembleGroup``, premvos_idmap_vote_u8: the combination
of the runs MergeTrack/oldmerge.py:129-131,220-224 writes under to_ensemble/<n>/); premvos_amd.ensemble votes PNG trees that exist.
``--search W`` scores W weight sets of this loop with eval_video's objective (``SearchGroup``: the W runs of a video in lockstep, the
random search of MergeTrack/oldmerge.py:225-227,253-255); ``--live-weights`` runs the loop with the weights that were found.

``--combine probabilistic`` and ``--oracle`` are the two swaps merge.py imports next to its loop's functions (merge.py:50-52:
``probabilitic_combination``, ``calculate_gt_scores``; csrc/merge_modes_ops.hip); opt-in, ``Tracker(combine=..., oracle=...)``.
``--viz`` is the third import of that line, ``viz_scores`` (merge_functions.py:547-611): one score sheet per frame, drawn on the GPU
right after the scores (premvos_amd.viz, csrc/viz_ops.hip; ``Tracker(viz=True)``); ``--max-reid-distance`` is the program
MergeTrack/print_max_reid_distance.py, which runs no merge at all.

Three forms of the same loop:

  * the reference's functions under their names and call shapes, on lists of proposal dicts -- ``read_ann``, ``read_props``,
    ``calculate_scores``, ``calculate_selected_props``, ``remove_mask_overlap``, ``update_templates``, ``save_pngs`` (and
    ``mergetrack.warp_proposals``); ``do_video(..., resident=False)`` is merge.py:69-115 written with them;
  * ``Tracker`` (``do_video``'s default): masks, embeddings and scores of the templates and of the warped candidates stay in HBM from
    frame to frame.  Per frame: decode the fresh proposals (premvos_rle_decode_u8), overlap counts (premvos_mask_overlap_u8), scores
    + selection (premvos_track_scores_f64), overlap removal + id map (premvos_track_paint_u8; the selection never visits the host),
    the id map to the PNG writer thread, warp (premvos_mask_warp_u8), run boundaries + boxes, refinement and ReID of the warped boxes.

  * ``TrackerGroup`` (``--lockstep V``, ``do_videos_lockstep``): ``Tracker.step_resident``'s work for up to 8 videos of one frame size
    at once -- one launch per step of premvos_mask_overlap_seats_u8, premvos_track_scores_seats_f64, premvos_track_paint_seats_u8,
    premvos_mask_warp_seats_u8 and of each net for all of them.  Per video the loop's own arithmetic gives the same bits; the nets see
    another batch size, so V > 1 promises the loop of merge.py:69-115 on what the engines returned, not the sequential run's bytes.

The reference's oddities are kept: after refinement a candidate's 'segmentation' is the refined mask while its 'mask' and 'bbox' stay
the warped ones; templates keep the first-frame ReID and id; 'object_score' is the maximum over the template's whole row;
annotations are read only for a ``00000.jpg``; a video without templates gets all-zero PNGs; an unreadable proposal file is an
empty list.  One rule is this package's own: among selections with EQUAL final scores the higher index is painted last (the
reference leaves that to numpy's unstable argsort; in practice such objects both selected the empty proposal).

No CPU fallback for the device work (``_lib.require_gpu()``).  Host-side by design: JSON / PNG files, RLE strings <-> run
boundaries, and ``calculate_selected_props`` of the dict form, whose inputs are host arrays of T x (P + 1) numbers.
"""
from __future__ import annotations

import contextlib
import glob
import json
import os
from copy import deepcopy as copy
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, mergetrack, rle
from .merge_out import VideoOut, remove_stale, summarise, write_pngs

MAX_REID_DISTANCE = 25                                                        # merge_functions.py:12 (compiled into the kernel)
SCORE_THRESH = 1e-10                                                          # merge.py:117
WEIGHTS = np.array([0.25920137, 0.22541801, 0.0775609, 0.12509281, 0.3127269])   # merge.py:119
NORMALISED_WEIGHTS = WEIGHTS / np.sum(WEIGHTS)
EMB = 128


# ---------------------------------------------------------------------------------------------------------------- device wrappers
def counts_from_string(s) -> np.ndarray:
    """``rle.string_to_counts`` without a Python loop per character (the frame's fresh proposals are a few thousand runs): 5-bit groups,
    LSB first, 0x20 = continuation, 0x10 of the last group = sign; from the 4th run on a value is a difference to the run two back,
    i.e. the odd and the even runs (from the third) are two running sums."""
    b = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros((0,), np.int64)
    if b[-1] & 0x20:                                       # a truncated string: the plain decoder's behaviour, whatever it is
        return np.asarray(rle.string_to_counts(s if isinstance(s, str) else bytes(s).decode("ascii")), np.int64)
    ends = np.flatnonzero((b & 0x20) == 0)
    starts = np.concatenate(([0], ends[:-1] + 1))
    n = ends - starts + 1
    k = np.arange(b.size) - np.repeat(starts, n)
    d = np.add.reduceat((b & 0x1F) << (5 * k), starts)
    d = np.where((b[ends] & 0x10) != 0, d | np.left_shift(np.int64(-1), 5 * n), d)
    c = d.copy()
    c[1::2] = np.cumsum(d[1::2])
    c[2::2] = np.cumsum(d[2::2])
    return c


def boundaries_from_segmentations(segs: Sequence[Dict]):
    """COCO RLE dicts -> (pool int32, offsets int32 [n+1]): each mask's ascending column-major run boundaries (the cumulative sum of
    its run lengths without the final h*w), the layout premvos_rle_boundaries_pooled_u8 writes.  Host work on a few hundred integers."""
    parts, offsets = [], [0]
    for s in segs:
        c = s["counts"]
        c = counts_from_string(c) if isinstance(c, (str, bytes)) else c
        b = np.cumsum(np.asarray(c, np.int64))[:-1] if len(c) else np.zeros((0,), np.int64)
        parts.append(b)
        offsets.append(offsets[-1] + len(b))
    pool = np.concatenate(parts).astype(np.int32) if parts else np.zeros((0,), np.int32)
    return pool, np.asarray(offsets, np.int32)


def decode_boundaries(pool, offsets, h: int, w: int, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """premvos_rle_decode_u8: pooled boundaries (numpy or CUDA int32) -> uint8 [n,h,w] in HBM, values 0 / 1."""
    _lib.require_gpu()
    dev = out.device if out is not None else (pool.device if isinstance(pool, torch.Tensor) and pool.is_cuda else _lib.resolve_device(device))
    n = len(offsets) - 1
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    assert out.is_contiguous() and tuple(out.shape) == (n, h, w) and out.dtype == torch.uint8, (out.shape, n, h, w)
    if n == 0:
        return out
    p = (pool if isinstance(pool, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pool, np.int32))).to(device=dev, dtype=torch.int32)
    o = (offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, np.int32))).to(device=dev, dtype=torch.int32)
    p = p.contiguous() if p.numel() else torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().premvos_rle_decode_u8(p.data_ptr(), int(pool.shape[0]), o.contiguous().data_ptr(), n, h, w, out.data_ptr(),
                                                 _lib.current_stream()), "rle_decode")
    return out


def decode_segmentations(segs: Sequence[Dict], out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """``pycocotools.mask.decode`` of every proposal's 'segmentation', on the GPU: uint8 [n,h,w] in HBM."""
    assert len(segs) or out is not None
    h, w = (segs[0]["size"] if len(segs) else out.shape[1:])
    assert all(list(s["size"]) == [h, w] for s in segs), "masks of one frame have one size"
    pool, offsets = boundaries_from_segmentations(segs)
    return decode_boundaries(pool, offsets, int(h), int(w), out, device)


def _f64(x, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    return t.to(device=dev, dtype=torch.float64).contiguous()


def track_scores(inter: torch.Tensor, area_p: torch.Tensor, area_t: torch.Tensor, template_score, proposal_score, emb_p, emb_t,
                 weights=None, score_thresh: float = SCORE_THRESH) -> Dict[str, torch.Tensor]:
    """premvos_track_scores_f64 -> {"planes" [5,T,P], "weighted" [T,P+1], "selected" int32 [T], "final_score" [T], "object_score" [T]}
    (CUDA tensors; nothing is copied to the host).  ``inter`` [T,P] / ``area_p`` / ``area_t`` as ``mergetrack.mask_overlap(proposals,
    templates)`` returns them."""
    _lib.require_gpu()
    dev = inter.device
    T, P = inter.shape
    wts = np.ascontiguousarray(NORMALISED_WEIGHTS if weights is None else weights, dtype=np.float64)
    assert wts.shape == (5,)
    ts, ps, ep, et = _f64(template_score, dev), _f64(proposal_score, dev), _f64(emb_p, dev), _f64(emb_t, dev)
    assert ts.shape == (T,) and ps.shape == (P,) and ep.shape == (P, EMB) and et.shape == (T, EMB), (ts.shape, ps.shape, ep.shape, et.shape)
    assert inter.dtype == torch.int64 and area_p.shape == (P,) and area_t.shape == (T,)
    out = {"planes": torch.empty((5, T, P), dtype=torch.float64, device=dev),
           "weighted": torch.empty((T, P + 1), dtype=torch.float64, device=dev),
           "selected": torch.empty((T,), dtype=torch.int32, device=dev),
           "final_score": torch.empty((T,), dtype=torch.float64, device=dev),
           "object_score": torch.empty((T,), dtype=torch.float64, device=dev)}
    _lib.check(_lib.load().premvos_track_scores_f64(
        inter.contiguous().data_ptr(), area_p.data_ptr(), area_t.data_ptr(), ts.data_ptr(), ps.data_ptr(), ep.data_ptr(), et.data_ptr(),
        T, P, wts.ctypes.data, float(score_thresh), out["planes"].data_ptr(), out["weighted"].data_ptr(), out["selected"].data_ptr(),
        out["final_score"].data_ptr(), out["object_score"].data_ptr(), _lib.current_stream()), "track_scores")
    return out


def track_paint(masks: torch.Tensor, selected: torch.Tensor, final_score: torch.Tensor, ids: torch.Tensor):
    """premvos_track_paint_u8 -> (labels [h,w], idmap [h,w], refined [T,h,w]) uint8 CUDA tensors.  ``masks`` uint8 [P,h,w] in HBM
    (nonzero = foreground); ``selected`` int32 [T], ``final_score`` float64 [T], ``ids`` int32 [T] are read from device memory."""
    _lib.require_gpu()
    dev = masks.device
    P, h, w = masks.shape
    T = selected.shape[0]
    sel = selected.to(device=dev, dtype=torch.int32).contiguous()
    fs = final_score.to(device=dev, dtype=torch.float64).contiguous()
    idt = ids.to(device=dev, dtype=torch.int32).contiguous()
    assert fs.shape == (T,) and idt.shape == (T,)
    labels = torch.empty((h, w), dtype=torch.uint8, device=dev)
    idmap = torch.empty((h, w), dtype=torch.uint8, device=dev)
    refined = torch.empty((T, h, w), dtype=torch.uint8, device=dev)
    m = masks.contiguous()
    _lib.check(_lib.load().premvos_track_paint_u8(m.data_ptr() if P else None, P, h, w, sel.data_ptr(), fs.data_ptr(), idt.data_ptr(), T,
                                                  labels.data_ptr(), idmap.data_ptr(), refined.data_ptr(), _lib.current_stream()),
               "track_paint")
    return labels, idmap, refined


def track_next(final_score: torch.Tensor, bbox: torch.Tensor):
    """premvos_track_next_f32 -> (cand_score float64 [n], yx float32 [n,4]) CUDA tensors: the warped candidates' 'score'
    0.5 * (final_score + 1) (merge_functions.py:234) and the refinement net's (y0, x0, y1, x1) boxes from ``bbox`` int32 [n,4]
    (``embed_masks``' x, y, w, h of the warped masks); ``final_score`` float64 [n], both read from device memory."""
    _lib.require_gpu()
    dev, n = final_score.device, int(final_score.shape[0])
    cand_score = torch.empty((n,), dtype=torch.float64, device=dev)
    yx = torch.empty((n, 4), dtype=torch.float32, device=dev)
    assert bbox.is_contiguous() and bbox.dtype == torch.int32
    _lib.check(_lib.load().premvos_track_next_f32(final_score.data_ptr(), bbox.data_ptr(), n, cand_score.data_ptr(), yx.data_ptr(),
                                                  _lib.current_stream()), "track_next")
    return cand_score, yx


# --------------------------------------------------------------------------- the oracle merge and the probabilistic combination
COMBINE_MODES = ("argmax", "probabilistic")
TEMPERATURE = 0.1                                                             # merge_functions.py:153 (compiled into the kernel)


def track_label_overlap(masks: torch.Tensor, labels: torch.Tensor, T: int):
    """premvos_mask_label_overlap_u8 -> (inter int64 [T,P], area_p int64 [P], area_l int64 [T]) CUDA tensors: candidate p against the
    pixels of ``labels`` (uint8 [h,w], an annotation's id map) that equal t + 1.  ``masks`` uint8 [P,h,w] in HBM, nonzero = foreground."""
    _lib.require_gpu()
    assert masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.shape[0] >= 1, masks.shape
    dev = masks.device
    P, h, w = masks.shape
    lab = labels.to(device=dev).contiguous()
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (h, w), (lab.dtype, lab.shape, (h, w))
    inter = torch.empty((T, P), dtype=torch.int64, device=dev)
    area_p = torch.empty((P,), dtype=torch.int64, device=dev)
    area_l = torch.empty((T,), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().premvos_mask_label_overlap_u8(masks.contiguous().data_ptr(), P, lab.data_ptr(), int(T), h * w, inter.data_ptr(),
                                                         area_p.data_ptr(), area_l.data_ptr(), _lib.current_stream()), "mask_label_overlap")
    return inter, area_p, area_l


def track_gt_scores(inter: torch.Tensor, area_p: torch.Tensor, area_l: torch.Tensor, weights=None,
                    score_thresh: float = SCORE_THRESH) -> Dict[str, torch.Tensor]:
    """premvos_track_gt_scores_f64 -> ``track_scores``' dict from ``track_label_overlap``'s counts: every plane is the IoU with the
    annotation of the template's object (merge_functions.py:78-94)."""
    _lib.require_gpu()
    dev = inter.device
    T, P = inter.shape
    wts = np.ascontiguousarray(NORMALISED_WEIGHTS if weights is None else weights, dtype=np.float64)
    assert wts.shape == (5,)
    assert inter.is_cuda and inter.dtype == torch.int64 and area_p.dtype == torch.int64 and area_l.dtype == torch.int64
    assert area_p.shape == (P,) and area_l.shape == (T,), (area_p.shape, area_l.shape, T, P)
    out = {"planes": torch.empty((5, T, P), dtype=torch.float64, device=dev),
           "weighted": torch.empty((T, P + 1), dtype=torch.float64, device=dev),
           "selected": torch.empty((T,), dtype=torch.int32, device=dev),
           "final_score": torch.empty((T,), dtype=torch.float64, device=dev),
           "object_score": torch.empty((T,), dtype=torch.float64, device=dev)}
    _lib.check(_lib.load().premvos_track_gt_scores_f64(
        inter.contiguous().data_ptr(), area_p.contiguous().data_ptr(), area_l.contiguous().data_ptr(), T, P, wts.ctypes.data,
        float(score_thresh), out["planes"].data_ptr(), out["weighted"].data_ptr(), out["selected"].data_ptr(), out["final_score"].data_ptr(),
        out["object_score"].data_ptr(), _lib.current_stream()), "track_gt_scores")
    return out


def track_combine(masks: torch.Tensor, weighted: torch.Tensor, ids: torch.Tensor) -> Dict[str, torch.Tensor]:
    """premvos_track_combine_f64 -> {"labels" [h,w], "idmap" [h,w], "refined" [T,h,w] uint8, "probs" float64 [T,P], "final_score"
    float64 [T]} CUDA tensors (merge_functions.py:151-195).  ``masks`` uint8 [P,h,w] in HBM; ``weighted`` float64 [T,P] or [T,P+1]
    (``track_scores``': the threshold column is not read), ``ids`` int32 [T], read from device memory."""
    _lib.require_gpu()
    assert masks.is_cuda and masks.dtype == torch.uint8 and masks.dim() == 3 and masks.shape[0] >= 1, masks.shape
    dev = masks.device
    P, h, w = masks.shape
    ws = weighted.to(device=dev, dtype=torch.float64)
    assert ws.dim() == 2 and ws.shape[0] >= 1 and ws.shape[1] in (P, P + 1), (ws.shape, P)
    ws = ws if ws.stride(1) == 1 else ws.contiguous()
    T = ws.shape[0]
    idt = ids.to(device=dev, dtype=torch.int32).contiguous()
    assert idt.shape == (T,)
    out = {"labels": torch.empty((h, w), dtype=torch.uint8, device=dev), "idmap": torch.empty((h, w), dtype=torch.uint8, device=dev),
           "refined": torch.empty((T, h, w), dtype=torch.uint8, device=dev), "probs": torch.empty((T, P), dtype=torch.float64, device=dev),
           "final_score": torch.empty((T,), dtype=torch.float64, device=dev)}
    denom = torch.empty((T,), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().premvos_track_combine_f64(masks.contiguous().data_ptr(), P, h, w, ws.data_ptr(), ws.stride(0), idt.data_ptr(), T,
                                                     out["probs"].data_ptr(), denom.data_ptr(), out["final_score"].data_ptr(),
                                                     out["labels"].data_ptr(), out["idmap"].data_ptr(), out["refined"].data_ptr(),
                                                     _lib.current_stream()), "track_combine")
    return out


# ------------------------------------------------------------------------------------------- the same three, several videos per launch
MAX_SEATS = 8


class SeatTable:
    """The seat table of the ``*_seats_*`` entry points (include/premvos_hip.h): ``rows`` int32 [V,4] = (T, F, cand_slot, fresh_slot)
    per seat, a HOST array the library reads during the call, and where each seat's slices of the pooled arrays begin:
    ``oT`` / ``oF`` / ``oP`` / ``oTP`` = sums of T, F, T + F, T * (T + F) over the seats before it (V + 1 entries: the last is the
    total).  A seat with T = 0 is empty: its F counts as 0."""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 4))
        self.V = int(self.rows.shape[0])
        self.T = self.rows[:, 0].astype(np.int64)
        self.F = np.where(self.T > 0, self.rows[:, 1], 0).astype(np.int64)
        self.P = self.T + self.F
        z = np.zeros((1,), np.int64)
        self.oT, self.oF = np.concatenate((z, np.cumsum(self.T))), np.concatenate((z, np.cumsum(self.F)))
        self.oP, self.oTP = np.concatenate((z, np.cumsum(self.P))), np.concatenate((z, np.cumsum(self.T * self.P)))

    @property
    def ptr(self) -> int:
        return self.rows.ctypes.data

    def views(self, s: Dict[str, torch.Tensor], v: int) -> Dict[str, torch.Tensor]:
        """Seat ``v``'s part of ``track_scores_seats``' / ``mask_overlap_seats``' pooled results, in ``track_scores``' shapes."""
        T, P, oT, oP, oTP = (int(x) for x in (self.T[v], self.P[v], self.oT[v], self.oP[v], self.oTP[v]))
        shapes = {"inter": (oTP, (T, P)), "area_p": (oP, (P,)), "area_t": (oT, (T,)), "planes": (5 * oTP, (5, T, P)),
                  "weighted": (oTP + oT, (T, P + 1)), "selected": (oT, (T,)), "final_score": (oT, (T,)), "object_score": (oT, (T,))}
        return {k: s[k][shapes[k][0]:shapes[k][0] + int(np.prod(shapes[k][1]))].view(shapes[k][1]) for k in s if k in shapes}


def mask_overlap_seats(pool: torch.Tensor, seats: SeatTable) -> Dict[str, torch.Tensor]:
    """premvos_mask_overlap_seats_u8 -> {"inter" int64 [sum T*P], "area_p" [sum P], "area_t" [sum T]} pooled in seat order: per seat what
    ``mergetrack.mask_overlap(the seat's proposals, its templates)`` returns.  ``pool`` uint8 [S,h,w] in HBM."""
    _lib.require_gpu()
    assert pool.is_cuda and pool.dtype == torch.uint8 and pool.is_contiguous() and pool.dim() == 3
    dev = pool.device
    out = {"inter": torch.empty((int(seats.oTP[-1]),), dtype=torch.int64, device=dev),
           "area_p": torch.empty((int(seats.oP[-1]),), dtype=torch.int64, device=dev),
           "area_t": torch.empty((int(seats.oT[-1]),), dtype=torch.int64, device=dev)}
    _lib.check(_lib.load().premvos_mask_overlap_seats_u8(pool.data_ptr(), pool.shape[0], pool.shape[1] * pool.shape[2], seats.ptr, seats.V,
                                                         out["inter"].data_ptr(), out["area_p"].data_ptr(), out["area_t"].data_ptr(),
                                                         _lib.current_stream()), "mask_overlap_seats")
    return out


def track_scores_seats(overlap: Dict[str, torch.Tensor], cand_score: torch.Tensor, cand_emb: torch.Tensor, templ_emb: torch.Tensor,
                       fresh_score: Optional[torch.Tensor], fresh_emb: Optional[torch.Tensor], seats: SeatTable, weights=None,
                       score_thresh: float = SCORE_THRESH) -> Dict[str, torch.Tensor]:
    """premvos_track_scores_seats_f64: ``track_scores`` per seat in one launch (one workgroup per seat).  ``overlap``: what
    ``mask_overlap_seats`` returned; ``cand_score`` [sum T], ``cand_emb`` / ``templ_emb`` [sum T,128], ``fresh_score`` [sum F],
    ``fresh_emb`` [sum F,128]: float64 CUDA tensors, pooled in seat order (the fresh pair may be None when no seat has fresh rows).
    -> ``track_scores``' keys, pooled and flat (``seats.views`` shapes a seat's part); "selected" is seat-local."""
    _lib.require_gpu()
    dev = cand_score.device
    nT, nF, nTP = int(seats.oT[-1]), int(seats.oF[-1]), int(seats.oTP[-1])
    wts = np.ascontiguousarray(NORMALISED_WEIGHTS if weights is None else weights, dtype=np.float64)
    assert wts.shape == (5,)
    for t, shape in ((cand_score, (nT,)), (cand_emb, (nT, EMB)), (templ_emb, (nT, EMB))) + (((fresh_score, (nF,)), (fresh_emb, (nF, EMB))) if nF else ()):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape, (t.shape, shape)
    assert overlap["inter"].shape == (nTP,) and overlap["area_p"].shape == (int(seats.oP[-1]),) and overlap["area_t"].shape == (nT,)
    out = {"planes": torch.empty((5 * nTP,), dtype=torch.float64, device=dev),
           "weighted": torch.empty((nTP + nT,), dtype=torch.float64, device=dev),
           "selected": torch.empty((nT,), dtype=torch.int32, device=dev),
           "final_score": torch.empty((nT,), dtype=torch.float64, device=dev),
           "object_score": torch.empty((nT,), dtype=torch.float64, device=dev)}
    _lib.check(_lib.load().premvos_track_scores_seats_f64(
        overlap["inter"].data_ptr(), overlap["area_p"].data_ptr(), overlap["area_t"].data_ptr(), cand_score.data_ptr(), cand_emb.data_ptr(),
        templ_emb.data_ptr(), fresh_score.data_ptr() if nF else None, fresh_emb.data_ptr() if nF else None, seats.ptr, seats.V,
        wts.ctypes.data, float(score_thresh), out["planes"].data_ptr(), out["weighted"].data_ptr(), out["selected"].data_ptr(),
        out["final_score"].data_ptr(), out["object_score"].data_ptr(), _lib.current_stream()), "track_scores_seats")
    return out


def track_paint_seats(pool: torch.Tensor, seats: SeatTable, selected: torch.Tensor, final_score: torch.Tensor, ids: torch.Tensor,
                      refined_slots=None, labels: Optional[torch.Tensor] = None, idmap: Optional[torch.Tensor] = None,
                      refined: Optional[torch.Tensor] = None):
    """premvos_track_paint_seats_u8 -> (labels [V,h,w], idmap [V,h,w], refined [R,h,w]) uint8 CUDA tensors: ``track_paint`` per seat in
    one launch.  Seat v's template t goes to plane ``refined_slots[v] + t`` of ``refined`` (default: pooled in seat order, R = sum T).
    ``selected`` int32 / ``final_score`` float64 / ``ids`` int32 [sum T] are read from device memory.  The planes of empty seats are not
    written (zero where this call makes the tensors)."""
    _lib.require_gpu()
    dev = pool.device
    S, h, w = pool.shape
    nT = int(seats.oT[-1])
    slots = np.ascontiguousarray(seats.oT[:-1] if refined_slots is None else refined_slots, dtype=np.int32)
    assert slots.shape == (seats.V,)
    for t, dt in ((selected, torch.int32), (final_score, torch.float64), (ids, torch.int32)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (nT,), (t.shape, nT)
    labels = torch.zeros((seats.V, h, w), dtype=torch.uint8, device=dev) if labels is None else labels
    idmap = torch.zeros((seats.V, h, w), dtype=torch.uint8, device=dev) if idmap is None else idmap
    refined = torch.empty((max(nT, 1), h, w), dtype=torch.uint8, device=dev) if refined is None else refined
    for t in (labels, idmap):
        assert t.is_contiguous() and t.dtype == torch.uint8 and tuple(t.shape) == (seats.V, h, w), t.shape
    assert pool.is_contiguous() and refined.is_contiguous() and refined.dtype == torch.uint8 and tuple(refined.shape[1:]) == (h, w)
    _lib.check(_lib.load().premvos_track_paint_seats_u8(pool.data_ptr(), S, h, w, seats.ptr, seats.V, selected.data_ptr(),
                                                        final_score.data_ptr(), ids.data_ptr(), labels.data_ptr(), idmap.data_ptr(),
                                                        refined.data_ptr(), refined.shape[0], slots.ctypes.data, _lib.current_stream()),
               "track_paint_seats")
    return labels, idmap, refined


def track_scores_sets(overlap: Dict[str, torch.Tensor], cand_score: torch.Tensor, cand_emb: torch.Tensor, templ_emb: torch.Tensor,
                      fresh_score: Optional[torch.Tensor], fresh_emb: Optional[torch.Tensor], seats: SeatTable, weight_sets,
                      score_thresh: float = SCORE_THRESH) -> Dict[str, torch.Tensor]:
    """premvos_track_scores_sets_f64: ``track_scores_seats`` with a weight row per seat (``weight_sets`` float64 [V,5], host) and ONE block
    of fresh rows that every occupied seat reads -- ``fresh_score`` [F], ``fresh_emb`` [F,128], F = the F every occupied seat carries in
    the table (None when F = 0).  The results are laid out as ``seats`` says: ``seats.views`` shapes a seat's part."""
    _lib.require_gpu()
    dev = cand_score.device
    nT, nTP = int(seats.oT[-1]), int(seats.oTP[-1])
    Fs = {int(f) for f, t in zip(seats.F, seats.T) if t}
    assert len(Fs) <= 1, f"the seats of a weight search share one block of fresh rows (got F = {sorted(Fs)})"
    F = Fs.pop() if Fs else 0
    wts = np.ascontiguousarray(weight_sets, dtype=np.float64)
    assert wts.shape == (seats.V, 5), (wts.shape, seats.V)
    for t, shape in ((cand_score, (nT,)), (cand_emb, (nT, EMB)), (templ_emb, (nT, EMB))) + (((fresh_score, (F,)), (fresh_emb, (F, EMB))) if F else ()):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape, (t.shape, shape)
    assert overlap["inter"].shape == (nTP,) and overlap["area_p"].shape == (int(seats.oP[-1]),) and overlap["area_t"].shape == (nT,)
    out = {"planes": torch.empty((5 * nTP,), dtype=torch.float64, device=dev),
           "weighted": torch.empty((nTP + nT,), dtype=torch.float64, device=dev),
           "selected": torch.empty((nT,), dtype=torch.int32, device=dev),
           "final_score": torch.empty((nT,), dtype=torch.float64, device=dev),
           "object_score": torch.empty((nT,), dtype=torch.float64, device=dev)}
    _lib.check(_lib.load().premvos_track_scores_sets_f64(
        overlap["inter"].data_ptr(), overlap["area_p"].data_ptr(), overlap["area_t"].data_ptr(), cand_score.data_ptr(), cand_emb.data_ptr(),
        templ_emb.data_ptr(), fresh_score.data_ptr() if F else None, fresh_emb.data_ptr() if F else None, seats.ptr, seats.V,
        wts.ctypes.data, float(score_thresh), out["planes"].data_ptr(), out["weighted"].data_ptr(), out["selected"].data_ptr(),
        out["final_score"].data_ptr(), out["object_score"].data_ptr(), _lib.current_stream()), "track_scores_sets")
    return out


def track_eval_seats(planes: torch.Tensor, gt: torch.Tensor, first_planes, T0: int, counts: torch.Tensor, t: int) -> None:
    """premvos_track_eval_seats_i64: ``counts[v, t, k]`` += |R and G|, |R or G|, |R| with R = plane ``first_planes[v] + k`` of ``planes``
    (uint8 [R,h,w], ``track_paint_seats``' ``refined``) and G = (``gt`` == k + 1), ``gt`` uint8 [h,w]; ``counts`` int64 [V,N,T0,3], all
    CUDA, zeroed by the caller once per video (``prewarp.search``'s layout: ``prewarp.scores_from_counts`` makes the objective)."""
    _lib.require_gpu()
    V, N = int(counts.shape[0]), int(counts.shape[1])
    first = np.ascontiguousarray(first_planes, dtype=np.int32)
    assert counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and tuple(counts.shape) == (V, N, T0, 3), counts.shape
    assert first.shape == (V,) and 0 <= t < N, (first.shape, V, t, N)
    assert planes.is_cuda and planes.dtype == torch.uint8 and planes.is_contiguous() and planes.dim() == 3, planes.shape
    h, w = int(planes.shape[1]), int(planes.shape[2])
    assert gt.is_cuda and gt.dtype == torch.uint8 and gt.is_contiguous() and tuple(gt.shape) == (h, w), (gt.dtype, gt.shape, (h, w))
    if T0 == 0:
        return
    _lib.check(_lib.load().premvos_track_eval_seats_i64(planes.data_ptr(), planes.shape[0], h, w, gt.data_ptr(), V, int(T0), first.ctypes.data,
                                                        counts[0, t].data_ptr(), N * int(T0) * 3, _lib.current_stream()), "track_eval_seats")


MIN_ENSEMBLE, DEFAULT_TOP = 2, 3                                              # (an ensemble has 2 .. MAX_SEATS members)


def vote_idmaps(maps: torch.Tensor, out: Optional[torch.Tensor] = None, votes: Optional[torch.Tensor] = None,
                hist: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """premvos_idmap_vote_u8: ``maps`` uint8 [K, ...] (CUDA, K = 1 .. 8 id maps of one shape; set k may be a strided view as long as each
    set is dense) -> {"voted": uint8 [...] the label most sets painted at each pixel (a tie: the set listed first wins), "votes": uint8
    [...] how many sets agree with it, "hist": int64 [K + 1], ``hist[v]`` += the pixels decided by v votes}.  ``out`` / ``votes`` /
    ``hist``: tensors to fill instead of new ones; ``hist`` is ADDED to (a new one starts at zero).  Queued on the current stream."""
    _lib.require_gpu()
    assert maps.is_cuda and maps.dtype == torch.uint8 and maps.dim() >= 1 and 1 <= maps.shape[0] <= MAX_SEATS, (maps.dtype, maps.shape)
    K, shape = int(maps.shape[0]), tuple(maps.shape[1:])
    pixels = int(np.prod(shape, dtype=np.int64))
    assert maps[0].is_contiguous() and (K == 1 or pixels == 0 or maps.stride(0) >= pixels), (maps.shape, maps.stride())
    dev = maps.device
    out = torch.empty(shape, dtype=torch.uint8, device=dev) if out is None else out
    votes = torch.empty(shape, dtype=torch.uint8, device=dev) if votes is None else votes
    hist = torch.zeros((K + 1,), dtype=torch.int64, device=dev) if hist is None else hist
    for t in (out, votes):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == shape, (t.dtype, t.shape, shape)
    assert hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and tuple(hist.shape) == (K + 1,), (hist.dtype, hist.shape)
    if pixels:                                                                # (a tensor without elements has no storage to point at)
        _lib.check(_lib.load().premvos_idmap_vote_u8(maps.data_ptr(), K, int(maps.stride(0)) if K > 1 else pixels, pixels, out.data_ptr(),
                                                     votes.data_ptr(), hist.data_ptr(), _lib.current_stream()), "vote_idmaps")
    return {"voted": out, "votes": votes, "hist": hist}


# ------------------------------------------------------------------------------------------------------------------- PNG output
def voc_palette() -> np.ndarray:
    """The 256-entry PASCAL VOC colour table (uint8 [256,3]) by its bit-reversal formula; equals the table of
    merge_functions.py:250-506 after its ``* 255`` and rounding."""
    pal = np.zeros((256, 3), np.uint8)
    for i in range(256):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        pal[i] = (r, g, b)
    return pal


def write_png(filename: str, idmap: np.ndarray) -> None:
    """merge_functions.py:508-514: a mode-P PNG whose pixel value is the palette index (the object id)."""
    from PIL import Image
    arr = np.ascontiguousarray(np.squeeze(idmap).astype(np.uint8))
    im = Image.frombytes("P", (arr.shape[1], arr.shape[0]), arr.tobytes())
    im.putpalette(voc_palette().reshape(-1).tolist())
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    im.save(filename)


# ---------------------------------------------------------------------------------------- the reference's functions, on dict lists
def read_ann(ann_fn: str) -> List[Dict]:
    """merge_functions.py:14-25."""
    from PIL import Image
    ann = np.array(Image.open(ann_fn))
    ids = [i for i in np.unique(ann) if i != 0]
    out = []
    for id_ in ids:
        seg = rle.encode((ann == id_).astype(np.uint8))
        out.append({"id": id_, "bbox": np.array(rle.to_bbox(seg)), "segmentation": seg, "conf_score": "1.0", "score": 1.0})
    return out


def read_props(prop_fn: str) -> List[Dict]:
    """merge_functions.py:27-36: a proposal without 'ReID' gets an all-inf embedding; an unreadable file is an empty list."""
    try:
        with open(prop_fn, "r") as f:
            proposals = json.load(f)
        for prop in proposals:
            if "ReID" not in prop.keys():
                prop["ReID"] = np.inf * np.ones((EMB))
    except Exception:            # noqa: BLE001 -- as the reference: whatever is wrong with the file, the frame has no fresh proposals
        proposals = []
    return proposals


def _scores_on_device(proposals: Sequence[Dict], templates: Sequence[Dict], weights=None, score_thresh: float = SCORE_THRESH):
    masks = decode_segmentations([p["segmentation"] for p in proposals] + [t["segmentation"] for t in templates])
    P = len(proposals)
    inter, area_p, area_t = mergetrack.mask_overlap(masks[:P], masks[P:])
    return track_scores(inter, area_p, area_t, [float(t["score"]) for t in templates], [float(p["score"]) for p in proposals],
                        np.array([np.asarray(p["ReID"], np.float64) for p in proposals]),
                        np.array([np.asarray(t["ReID"], np.float64) for t in templates]), weights, score_thresh)


def calculate_scores(proposals: Sequence[Dict], templates: Sequence[Dict]) -> np.ndarray:
    """merge_functions.py:38-76 -> float64 [5, T, P] (mask, ReID, other ReID, warp, other warp)."""
    return _scores_on_device(proposals, templates)["planes"].cpu().numpy()


def label_map_of(gt_props: Sequence[Dict], T: int, h: int, w: int) -> np.ndarray:
    """The id map ``calculate_gt_scores``' ``gt_props`` (``read_ann`` of the frame's annotation) came from: uint8 [h,w].  An id outside
    1 .. T is refused (the reference's ``gt_segs[init_id-1]`` raises or, for id 0, takes the last object's place); so are masks that
    overlap (an id map's never do)."""
    labels = np.zeros((h, w), np.uint8)
    for g in gt_props:
        i = int(g["id"])
        if not 1 <= i <= T:
            raise _lib.PremvosError(f"calculate_gt_scores: annotation id {i} has no template (the oracle scores row k against id k + 1 of {T})")
        m = rle.decode(g["segmentation"]).astype(bool)
        if labels[m].any():
            raise _lib.PremvosError("calculate_gt_scores: the annotation's masks overlap (they are the objects of one id map)")
        labels[m] = i
    return labels


def calculate_gt_scores(proposals: Sequence[Dict], gt_props: Sequence[Dict], templates: Sequence[Dict]) -> np.ndarray:
    """merge_functions.py:78-94 -> float64 [5, T, P], every plane the IoU of proposal p with the annotation of id t + 1 (all zeros for an
    object the annotation lacks)."""
    masks = decode_segmentations([p["segmentation"] for p in proposals])
    T = len(templates)
    labels = torch.from_numpy(label_map_of(gt_props, T, int(masks.shape[1]), int(masks.shape[2]))).to(masks.device)
    return track_gt_scores(*track_label_overlap(masks, labels, T))["planes"].cpu().numpy()


def probabilitic_combination(proposals: Sequence[Dict], weighted_scores: np.ndarray, templates: Sequence[Dict], score_thresh: float) -> List[Dict]:
    """merge_functions.py:151-195 (the reference's spelling; ``score_thresh`` is unused there too): the soft merge of ALL proposals
    instead of ``calculate_selected_props`` + ``remove_mask_overlap``.  'id' is the template's (the reference writes index + 1 and
    marks it wrong); a non-finite weighted score counts as 0."""
    masks = decode_segmentations([p["segmentation"] for p in proposals])
    dev = masks.device
    ws = _f64(np.asarray(weighted_scores, np.float64).reshape(len(templates), len(proposals)), dev)
    r = track_combine(masks, ws, torch.tensor([int(t["id"]) for t in templates], dtype=torch.int32, device=dev))
    segs = mergetrack.encode_masks(r["refined"])
    refined, best = r["refined"].cpu().numpy(), r["final_score"].cpu().numpy()
    return [{"segmentation": segs[i], "bbox": np.array(rle.to_bbox(segs[i])), "final_score": best[i], "mask": refined[i],
             "id": templates[i]["id"]} for i in range(len(templates))]


def calculate_selected_props(proposals: List[Dict], weighted_scores: np.ndarray, templates: Sequence[Dict], score_thresh: float,
                             object_scores: np.ndarray) -> List[Dict]:
    """merge_functions.py:96-121 (appends the empty proposal to ``proposals``, like the reference)."""
    h, w = proposals[0]["segmentation"]["size"]
    empty_seg = rle.encode(np.zeros((h, w), np.uint8))
    proposals.append({"segmentation": empty_seg, "bbox": np.array(rle.to_bbox(empty_seg))})
    ws = np.append(np.asarray(weighted_scores, np.float64), score_thresh * np.ones((len(weighted_scores), 1)), axis=1)
    ws[np.logical_not(np.isfinite(ws))] = 0
    best, index, best_obj = ws.max(axis=1), ws.argmax(axis=1), np.asarray(object_scores).max(axis=1)
    selected = [proposals[i].copy() for i in index]
    for prop, score, template, object_score in zip(selected, best, templates, best_obj):
        prop["final_score"], prop["object_score"], prop["id"] = score, object_score, template["id"]
    return selected


def remove_mask_overlap(proposals: Sequence[Dict]) -> List[Dict]:
    """merge_functions.py:123-149: every pixel goes to the selection with the highest final score that covers it."""
    scores = [p["final_score"] if p["final_score"] else 0 for p in proposals]
    object_scores = [p["object_score"] if p["object_score"] else 0 for p in proposals]
    masks = decode_segmentations([p["segmentation"] for p in proposals])
    T = len(proposals)
    dev = masks.device
    _, _, refined = track_paint(masks, torch.arange(T, dtype=torch.int32, device=dev), _f64(scores, dev),
                                torch.zeros((T,), dtype=torch.int32, device=dev))
    segs = mergetrack.encode_masks(refined)
    refined = refined.cpu().numpy()
    return [{"segmentation": segs[i], "bbox": np.array(rle.to_bbox(segs[i])), "final_score": scores[i], "object_score": object_scores[i],
             "mask": refined[i], "id": proposals[i]["id"]} for i in range(T)]


def update_templates(templates: Sequence[Dict], next_props: Sequence[Dict]) -> List[Dict]:
    """merge_functions.py:243-248: the refined candidates become the templates; ReID and id stay the first frame's."""
    new_templates = copy(list(next_props))
    for prop, template in zip(new_templates, templates):
        prop["ReID"] = template["ReID"]
        prop["id"] = template["id"]
    return new_templates


def save_pngs(proposals: Sequence[Dict], output_fn: str, empty: bool = False) -> None:
    """merge_functions.py:516-525 (masks that remove_mask_overlap made are disjoint: the order of the list does not matter then)."""
    first = proposals[0]["mask"]
    first = first.cpu().numpy() if isinstance(first, torch.Tensor) else np.asarray(first)
    png = np.zeros_like(first)
    if not empty:
        for prop in proposals:
            m = prop["mask"]
            m = m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
            png[m.astype("bool")] = prop["id"]
    write_png(output_fn, png)


# ---------------------------------------------------------------------------------------------------------------- engines
def _default_engine_calls(do_refinement, add_ReID):
    from .refinement.driver import do_refinement as dr
    from .reid.driver import add_ReID as ar
    return do_refinement or dr, add_ReID or ar


def _image_size(image_fn: str):
    from PIL import Image
    with Image.open(image_fn) as im:
        return im.size[1], im.size[0]


def _gt_idmap(gt, hw, who: str) -> torch.Tensor:
    """A frame's annotation id map (uint8 [h,w] array or tensor) as a tensor, for ``who`` ("the oracle merge", ...); not moved."""
    g = gt if isinstance(gt, torch.Tensor) else torch.from_numpy(np.array(gt))                  # (a copy: PIL's arrays are read-only)
    if g.dtype != torch.uint8 or tuple(g.shape) != tuple(hw):
        raise _lib.PremvosError(f"{who}: gt must be a uint8 id map of shape {tuple(hw)} (got {g.dtype}, {tuple(g.shape)})")
    return g


def _flow_tensor(flow) -> torch.Tensor:
    """A flow given as .flo name, [h,w,2] array or tensor -> a float32 tensor (a tensor is passed through untouched)."""
    if isinstance(flow, torch.Tensor):
        return flow
    flow = mergetrack.get_flow(flow) if isinstance(flow, str) else flow
    return torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32))


def _frame_array(frame):
    """A frame given as image name -> its uint8 [h,w,3] RGB array; an array or a tensor is passed through untouched."""
    if isinstance(frame, str):
        from PIL import Image
        return np.asarray(Image.open(frame).convert("RGB"))
    return frame


def _log_engine_calls(log: List[Dict], image_fn, bbox: np.ndarray, mask: np.ndarray, reid: np.ndarray) -> None:
    """What the engines returned for one advance, as ``engine_log`` keeps it: a "refine" and a "reid" record."""
    log.append({"call": "refine", "image_fn": image_fn, "bbox": bbox, "mask": mask})
    log.append({"call": "reid", "image_fn": image_fn, "ReID": reid})


class IdMapSlot:
    """One id map on its way to the host: a page-locked buffer and the event recorded behind its copy."""

    def __init__(self, buf: torch.Tensor, event, ring):
        self.buf, self.event, self._ring = buf, event, ring

    def wait(self) -> np.ndarray:
        self.event.synchronize()
        return self.buf.numpy()

    def release(self) -> None:
        self._ring.put(self)


class _TrackerBase:
    """What ``Tracker`` and ``TrackerGroup`` share besides the loop: the phase ``timer`` and the page-locked id-map buffers in flight to
    the PNG writer -- ``ring_slots`` of them, made on first use, reused once their reader released them."""

    def __init__(self):
        self.timer: Optional[Callable[[str], None]] = None     # tools/time_track_*.py: called with a phase name when the phase ends
        self.ring_slots = 16                      # page-locked id-map buffers in flight to the PNG writer
        self._ring = None
        self.ring_alive: Optional[Callable[[], bool]] = None     # is whoever releases the id-map buffers still at work?

    def _tick(self, phase: str) -> None:
        if self.timer is not None:
            self.timer(phase)

    def _idmap_slot(self, *shape: int) -> "IdMapSlot":
        """A page-locked uint8 buffer of ``shape`` ([h,w]; a group: [seats,h,w]) + event from the ring (made on first use, reused once its
        reader released it)."""
        import queue
        if self._ring is None:
            self._ring, self._ring_made = queue.Queue(), 0
        while True:
            try:
                slot = self._ring.get_nowait()
            except queue.Empty:
                if self._ring_made >= self.ring_slots:                        # every slot is with the PNG writer: wait for one (host only)
                    try:
                        slot = self._ring.get(timeout=0.5)
                    except queue.Empty:                                       # (only the writer returns slots: do not outwait its failure)
                        if self.ring_alive is not None and not self.ring_alive():
                            raise _lib.PremvosError("the PNG writer failed while id maps were waiting for their buffers")
                        continue
                else:
                    self._ring_made += 1
                    return IdMapSlot(torch.empty(shape, dtype=torch.uint8).pin_memory(), torch.cuda.Event(), self._ring)
            if tuple(slot.buf.shape) == tuple(shape):
                return slot
            self._ring_made -= 1                                              # another frame size: dropped, a new one is made

    def pin_idmap_ring(self, *shape: int) -> None:
        """Make the ring's page-locked buffers now (a page-locked allocation blocks the host): call it once per video, before the
        first ``step_resident``; without it the buffers are made as the first ``ring_slots`` frames need them."""
        slots = []
        while (self._ring_made if self._ring is not None else 0) < self.ring_slots:
            slots.append(self._idmap_slot(*shape))
        for s in slots:
            s.release()


class Tracker(_TrackerBase):
    """The resident form of one video's loop.  ``do_refinement(proposals, image_fn, refinement_net)`` and ``add_ReID(proposals,
    image_fn, ReID_net)`` have the reference's call shapes (MergeTrack/refinement_net_functions.py:38, ReID_net_functions.py:26) and
    default to this package's; with this package's engines the warped boxes go through the nets without their masks leaving HBM,
    any other pair (a test's stubs) is called on proposal dicts and its 'segmentation' / 'ReID' results are uploaded."""

    def __init__(self, refinement_net, ReID_net, do_refinement: Optional[Callable] = None, add_ReID: Optional[Callable] = None,
                 weights=None, score_thresh: float = SCORE_THRESH, device=None, record: bool = False, combine: str = "argmax",
                 oracle: bool = False, viz: bool = False):
        _lib.require_gpu()
        super().__init__()
        from .refinement.driver import RefinementEngine
        from .reid.driver import ReIDEngine
        if combine not in COMBINE_MODES:
            raise ValueError(f"combine: one of {COMBINE_MODES} (got {combine!r})")
        # combine="probabilistic": probabilitic_combination instead of calculate_selected_props + remove_mask_overlap;
        # oracle: calculate_gt_scores instead of calculate_scores (merge.py:50-52's two swaps); the defaults are merge.py:69-115
        self.combine, self.oracle = combine, bool(oracle)
        self.refinement_net, self.ReID_net = refinement_net, ReID_net
        self._direct = (do_refinement is None and add_ReID is None and isinstance(refinement_net, RefinementEngine)
                        and isinstance(ReID_net, ReIDEngine))
        self.do_refinement, self.add_ReID = _default_engine_calls(do_refinement, add_ReID)
        self.weights = np.ascontiguousarray(NORMALISED_WEIGHTS if weights is None else weights, dtype=np.float64)
        self.score_thresh = score_thresh
        self.device = _lib.resolve_device(device)
        self.record = record
        self.engine_log: List[Dict] = []          # record=True: what the engines returned, call by call (replayed by tests)
        self.T = 0
        self.ids: List = []
        self.ids_dev = self.templ_emb = self.cand_masks = self.cand_emb = self.cand_score = self._fos = None
        self.evaluator = None                     # --eval: a premvos_amd.evaluate.LoopEval, handed every id map right after the paint
        self.on_idmap: Optional[Callable] = None  # step_resident: called with the id map (CUDA tensor) right after the paint (--overlay)
        # viz: viz_scores (merge_functions.py:547-611) right after the scores of every ``step`` (premvos_amd.viz.sheet)
        self.viz = bool(viz)
        self.cand_boxes: Optional[np.ndarray] = None     # the carried candidates' 'bbox' (x, y, w, h), float64 [T,4]: read_ann's, then the warped masks'
        self.on_sheet: Optional[Callable] = None  # step, viz: called with the frame's score sheet (uint8 CUDA tensor) right after the scores
        self.viz_tint = None                      # viz: draw_mask's colour (None: premvos_amd.viz.default_tint())
        self._viz_inputs = self._viz_record = None

    # -- first frame ---------------------------------------------------------------------------------------------------------
    def add_templates(self, new_templates: List[Dict], image_fn: Optional[str]) -> None:
        """merge.py:79-82: annotation objects become templates and, unchanged, the candidates of their own frame.  ``image_fn`` None:
        the templates carry their 'ReID' already."""
        if not new_templates:
            return
        if image_fn is not None:
            new_templates = self.add_ReID(new_templates, image_fn, self.ReID_net)
        if self.record:
            self.engine_log.append({"call": "reid", "image_fn": image_fn, "ReID": np.array([t["ReID"] for t in new_templates], np.float64)})
        dev = self.device
        masks = decode_segmentations([t["segmentation"] for t in new_templates], device=dev)
        emb = _f64(np.array([np.asarray(t["ReID"], np.float64) for t in new_templates]), dev)
        score = _f64([float(t["score"]) for t in new_templates], dev)
        ids = torch.tensor([int(t["id"]) for t in new_templates], dtype=torch.int32, device=dev)
        boxes = np.array([np.asarray(t["bbox"] if "bbox" in t else rle.to_bbox(t["segmentation"]), np.float64) for t in new_templates]).reshape(-1, 4)
        if self.T:                                                            # (None: the carried boxes stayed in HBM, step_resident)
            boxes = None if self.cand_boxes is None else np.concatenate([self.cand_boxes, boxes])
        self.cand_boxes = boxes
        if self.T:
            assert masks.shape[1:] == self.cand_masks.shape[1:]
            masks, score = torch.cat([self.cand_masks, masks]), torch.cat([self.cand_score, score])
            self.templ_emb, self.cand_emb = torch.cat([self.templ_emb, emb]), torch.cat([self.cand_emb, emb])
            ids = torch.cat([self.ids_dev, ids])
        else:
            self.templ_emb, self.cand_emb = emb, emb.clone()
        self.cand_masks, self.cand_score, self.ids_dev = masks, score, ids
        self.ids += [t["id"] for t in new_templates]
        self.T = len(self.ids)

    # -- score, then select and paint: the part of a frame both forms of the step share ---------------------------------------------
    def _score_select_paint(self, masks: torch.Tensor, pscore: torch.Tensor, emb_p: torch.Tensor, gt):
        """``masks`` uint8 [P,h,w] (the first T: the carried candidates = the templates' masks), the proposal side's scores and
        embeddings -> (``track_scores``' dict, labels, idmap, refined).  The defaults: premvos_mask_overlap_u8, premvos_track_scores_f64,
        premvos_track_paint_u8.  ``oracle``: the scores are the IoUs with ``gt`` (the frame's annotation id map);
        ``combine="probabilistic"``: premvos_track_combine_f64 paints, and "final_score" becomes the row maximum it takes
        (merge_functions.py:181); "probs" joins the dict."""
        T = self.T
        if self.oracle:
            if gt is None:
                raise _lib.PremvosError("the oracle merge needs the frame's annotation: step(..., gt=<uint8 [h,w] id map>)")
            if [int(i) for i in self.ids] != list(range(1, T + 1)):
                raise _lib.PremvosError(f"the oracle merge scores row k against annotation id k + 1: the template ids must be 1 .. {T} in "
                                        f"order (got {[int(i) for i in self.ids]})")
            inter, area_p, area_l = track_label_overlap(masks, _gt_idmap(gt, masks.shape[1:], "the oracle merge").to(masks.device), T)
            self._tick("label_overlap")
            s = track_gt_scores(inter, area_p, area_l, self.weights, self.score_thresh)
            self._tick("gt_scores")
        else:
            # templates' masks and scores ARE the warped candidates' (update_templates copies them): the first T rows
            inter, area_p, area_t = mergetrack.mask_overlap(masks, masks[:T])
            self._tick("overlap")
            s = track_scores(inter, area_p, area_t, self.cand_score, pscore, emb_p, self.templ_emb, self.weights, self.score_thresh)
            self._tick("scores")
        if self._viz_inputs is not None:
            self._sheet(masks, s, gt)
        if self.combine == "probabilistic":
            c = track_combine(masks, s["weighted"], self.ids_dev)
            s = dict(s, final_score=c["final_score"], probs=c["probs"])
            return s, c["labels"], c["idmap"], c["refined"]
        labels, idmap, refined = track_paint(masks, s["selected"], s["final_score"], self.ids_dev)
        return s, labels, idmap, refined

    def _sheet(self, masks: torch.Tensor, s: Dict[str, torch.Tensor], gt) -> None:
        """viz_scores for the frame at hand: where merge.py would call it, between the scores and the selection.  The gt row of template k
        is the IoU with the annotation's object ``ids[k]`` (ids 1 .. T in order, the reference's case: label k + 1): with ``oracle`` the
        planes ARE those IoUs, without it one more premvos_mask_label_overlap_u8 + premvos_track_gt_scores_f64 on the same masks."""
        from . import viz
        frame, boxes = self._viz_inputs
        self._viz_inputs = None
        if self.oracle:
            gt_iou = s["planes"][0]
        else:
            if gt is None:
                raise _lib.PremvosError("the score sheet needs the frame's annotation: step(..., gt=<uint8 [h,w] id map>)")
            g = _gt_idmap(gt, masks.shape[1:], "the score sheet").to(masks.device)
            ids = [int(i) for i in self.ids]
            if ids != list(range(1, self.T + 1)):                              # label ids[k] -> k + 1, everything else -> 0
                lut = np.zeros((256,), np.uint8)
                for k, i in enumerate(ids):
                    if 0 < i < 256:
                        lut[i] = k + 1
                g = torch.from_numpy(lut).to(masks.device)[g.long()]
            gt_iou = track_gt_scores(*track_label_overlap(masks, g, self.T), self.weights, self.score_thresh)["planes"][0]
        sheet = viz.sheet(frame, masks, boxes, s["planes"], s["weighted"], gt_iou, self.viz_tint)
        if self.on_sheet is not None:
            self.on_sheet(sheet)
        if self.record:
            self._viz_record = {"viz_boxes": boxes.cpu().numpy(), "viz_gt": gt_iou.cpu().numpy(), "viz_masks": masks.cpu().numpy(),
                                "sheet": sheet.cpu().numpy()}
        self._tick("sheet")

    def _tick_painted(self) -> None:
        if self.combine == "probabilistic":
            self._tick("combine")
        else:
            self._tick("paint")

    # -- one frame -------------------------------------------------------------------------------------------------------------
    def step(self, fresh: List[Dict], flow=None, next_image_fn: Optional[str] = None, gt=None, frame=None) -> Dict[str, object]:
        """The frame's fresh proposals (``read_props``) against the templates: -> {"idmap": uint8 [h,w] CUDA tensor (what the PNG
        holds)} and, with ``record``, host copies of "selected", "weighted", "planes", "final_score", "object_score".  ``flow``
        ([h,w,2] array / CUDA tensor / .flo name, None on the last frame) carries the selection to ``next_image_fn``.  ``gt``: the
        frame's annotation id map, uint8 [h,w] array or CUDA tensor; required with ``oracle``, unused without.  With
        ``combine="probabilistic"`` the record also carries "probs".  ``frame``: with ``viz``, the frame itself (image name, uint8
        [h,w,3] array or CUDA tensor) -- its score sheet goes to ``on_sheet`` and, with ``record``, into the result ("sheet",
        "viz_boxes", "viz_gt", "viz_masks"); ``gt`` is required then too."""
        assert self.T > 0, "no templates: call add_templates first"
        dev, T = self.device, self.T
        _, h, w = self.cand_masks.shape
        F = len(fresh)
        P = T + F
        if self.viz:
            if frame is None or self.cand_boxes is None:
                raise _lib.PremvosError("the score sheet needs the frame and the candidates' boxes: step(..., frame=<image>) on a tracker "
                                        "that advanced through step")
            from . import jpeg
            boxes = np.concatenate([self.cand_boxes] + [np.asarray(p["bbox"], np.float64).reshape(1, 4) for p in fresh])
            self._viz_inputs = (jpeg.to_device(_frame_array(frame), dev), _f64(boxes, dev))
        masks = torch.empty((P, h, w), dtype=torch.uint8, device=dev)
        masks[:T].copy_(self.cand_masks)
        pscore, emb_p = self.cand_score, self.cand_emb
        if F:
            decode_segmentations([p["segmentation"] for p in fresh], out=masks[T:])
            pscore = torch.cat([pscore, _f64([float(p["score"]) for p in fresh], dev)])
            emb_p = torch.cat([emb_p, _f64(np.array([np.asarray(p["ReID"], np.float64) for p in fresh]), dev)])
        self._tick("decode")
        s, labels, idmap, refined = self._score_select_paint(masks, pscore, emb_p, gt)
        if self.evaluator is not None:
            self.evaluator.frame(idmap)
        self._tick_painted()
        out: Dict[str, object] = {"idmap": idmap}
        if self.record:
            out.update({k: s[k].cpu().numpy() for k in ("selected", "weighted", "planes", "final_score", "object_score", "probs") if k in s})
            out["labels"] = labels.cpu().numpy()
            if self._viz_record is not None:
                out.update(self._viz_record)
                self._viz_record = None
        if flow is not None:
            self._advance(refined, s["final_score"], flow, next_image_fn)
        return out

    # -- one frame, everything resident ---------------------------------------------------------------------------------------------
    def step_resident(self, fresh_masks: Optional[torch.Tensor], reid_rows: Optional[torch.Tensor], scores: Optional[torch.Tensor],
                      flow: Optional[torch.Tensor] = None, next_frame: Optional[torch.Tensor] = None,
                      stack: Optional[torch.Tensor] = None, next_slots: Optional[torch.Tensor] = None, gt=None) -> Dict[str, object]:
        """``step`` for a caller whose arrays are in HBM already (premvos_amd.stream --track): ``fresh_masks`` uint8 [F,h,w],
        ``reid_rows`` float32 [F,132] (``ReIDNet.embed_masks``: 128 embedding values + the mask's box as int32 bits; a box with
        w <= 0 or h <= 0 = no embedding), ``scores`` float64 [F], ``flow`` float32 [h,w,2] and ``next_frame`` uint8 [h,w,3] (both None
        on a video's last frame), all CUDA; F = 0: the three may be None.  Everything is queued on the current stream: no host
        synchronisation, no RLE, nothing copied to the host but the id map -- into a page-locked ring buffer, with an event.
        -> {"idmap": ``IdMapSlot`` (``wait()`` -> the [h,w] array once the event has passed; ``release()`` when done), "selected",
        "weighted", "planes", "final_score", "object_score", "labels": CUDA tensors}.
        ``stack``: uint8 [T + F,h,w] whose last F entries ARE ``fresh_masks`` and whose first T are free for the candidates (the feed
        lays its store out like this: no gather); ``next_slots``: uint8 [T,h,w], where the refined candidates of the next frame go (the
        first T entries of the next call's ``stack``).  Both optional: without them the tracker uses stores of its own.  ``gt``: as in
        ``step``; with ``combine="probabilistic"`` the result also carries "probs"."""
        assert self.T > 0, "no templates: call add_templates first"
        if not self._direct:
            raise _lib.PremvosError("step_resident needs this package's engines (RefinementEngine, ReIDEngine)")
        if self.viz:
            raise _lib.PremvosError("the score sheets are drawn by step (premvos_amd.track --viz), not by step_resident")
        dev, T, lib = self.device, self.T, _lib.load()
        _, h, w = self.cand_masks.shape
        F = 0 if fresh_masks is None else int(fresh_masks.shape[0])
        P = T + F
        if stack is None:
            stack = torch.empty((P, h, w), dtype=torch.uint8, device=dev)
            if F:
                stack[T:].copy_(fresh_masks)
        assert stack.is_contiguous() and tuple(stack.shape) == (P, h, w) and stack.dtype == torch.uint8, (stack.shape, P, h, w)
        if self.cand_masks.data_ptr() != stack.data_ptr():                    # (a video's first frame, or a caller without next_slots)
            stack[:T].copy_(self.cand_masks)
        pscore = torch.empty((P,), dtype=torch.float64, device=dev)
        emb_p = torch.empty((P, EMB), dtype=torch.float64, device=dev)
        if F:
            assert reid_rows.is_contiguous() and tuple(reid_rows.shape) == (F, EMB + 4) and reid_rows.dtype == torch.float32
            assert scores.is_contiguous() and tuple(scores.shape) == (F,) and scores.dtype == torch.float64
        _lib.check(lib.premvos_track_inputs_f64(self.cand_score.data_ptr(), self.cand_emb.data_ptr(), scores.data_ptr() if F else None,
                                                reid_rows.data_ptr() if F else None, T, F, pscore.data_ptr(), emb_p.data_ptr(),
                                                _lib.current_stream()), "track_inputs")
        self._tick("inputs")
        s, labels, idmap, refined = self._score_select_paint(stack, pscore, emb_p, gt)
        slot = self._idmap_slot(h, w)
        slot.buf.copy_(idmap, non_blocking=True)
        slot.event.record(torch.cuda.current_stream(dev))
        if self.evaluator is not None:                                        # (behind the id map's event: the PNG does not wait for it)
            self.evaluator.frame(idmap)
        if self.on_idmap is not None:
            self.on_idmap(idmap)
        self._tick_painted()
        out: Dict[str, object] = dict(s, idmap=slot, labels=labels)
        if flow is None:
            return out
        if T > min(self.refinement_net.max_boxes, self.ReID_net.max_boxes):
            raise _lib.PremvosError(f"{T} objects in one video: the resident tracker runs at most "
                                    f"{min(self.refinement_net.max_boxes, self.ReID_net.max_boxes)} (the engines' max_boxes) per launch; "
                                    "run premvos_amd.stream --reid and premvos_amd.track for this video")
        from .refinement.driver import _bucket
        from .reid.driver import _bucket as _reid_bucket
        warped = mergetrack.warp_masks(refined, flow)
        self._tick("warp")
        if self._fos is None or self._fos.shape[0] != T:
            self._fos = torch.zeros((T,), dtype=torch.int32, device=dev)
        # the ReID plan finds the warped masks' rleToBbox boxes itself (and their context boxes, and crops by them): the candidates'
        # 'bbox' stays the WARPED one, as in _advance; an empty warped mask gets the embedding of the box 0 0 0 0 -- what the host route
        # embed(image, [[0, 0, 0, 0]], feed=True) gives it, finite and used by the next frame's scores (pinned bit for bit by
        # tests/test_gpu_track_resident.py::test_resident_advance_equals_the_dict_advance_with_the_real_engines)
        emb, bbox = self.ReID_net.net.embed_masks(next_frame[None], warped, self._fos, max_slots=_reid_bucket(T), feed=True)
        cand_emb = emb.to(torch.float64)
        cand_score, yx = track_next(s["final_score"], bbox)
        self._tick("boxes+reid")
        p = self.refinement_net.net.refine(next_frame, yx, max_boxes=_bucket(T))
        dest = next_slots if next_slots is not None else torch.empty((T, h, w), dtype=torch.uint8, device=dev)
        assert tuple(dest.shape) == (T, h, w) and dest.is_contiguous()
        dest.copy_(p.mask[:T])
        self.cand_masks, self.cand_emb, self.cand_score = dest, cand_emb, cand_score
        self.cand_boxes = None                                                # (the warped boxes stayed in HBM: bbox)
        self._tick("refine")
        return out

    def _advance(self, refined: torch.Tensor, final_score: torch.Tensor, flow, next_image_fn) -> None:
        """merge.py:98-102: warp_proposals, do_refinement, add_ReID, update_templates.  With this package's engines ``next_image_fn``
        may also be the decoded frame (uint8 [h,w,3] array or CUDA tensor)."""
        warped = mergetrack.warp_masks(refined, _flow_tensor(flow))
        segs = mergetrack.encode_masks(warped)                                        # run boundaries on the GPU; strings + boxes on the host
        boxes = [rle.to_bbox(sg) for sg in segs]
        self.cand_boxes = np.array(boxes, np.float64).reshape(-1, 4)                  # 'bbox' stays the WARPED mask's (merge_functions.py:233)
        self.cand_score = 0.5 * (final_score + 1)                                     # 'score' of a warped proposal (merge_functions.py:234)
        self._tick("warp+rle+bbox")
        if self._direct and self.T <= self.refinement_net.max_boxes:
            from . import jpeg
            from .refinement.driver import _bucket
            image = _frame_array(next_image_fn)
            frame = jpeg.to_device(image, self.refinement_net.net.device)
            yx = np.array([[b[1], b[0], b[1] + b[3], b[0] + b[2]] for b in boxes], np.float32)
            p = self.refinement_net.net.refine(frame, torch.from_numpy(yx).to(self.refinement_net.net.device), max_boxes=_bucket(self.T))
            self.cand_masks = p.mask[:self.T].to(self.device).clone()
            self._tick("refine")
            emb = self.ReID_net.embed(image, boxes, feed=True)
            self.cand_emb = _f64(emb.astype(np.float64), self.device)
            self._tick("reid")
            if self.record:
                _log_engine_calls(self.engine_log, next_image_fn, np.array(boxes), self.cand_masks.cpu().numpy(), emb.astype(np.float64))
            return
        fs = final_score.cpu().numpy()
        props = [{"segmentation": segs[i], "bbox": boxes[i], "score": 0.5 * (fs[i] + 1), "final_score": fs[i], "mask": warped[i],
                  "id": self.ids[i]} for i in range(self.T)]
        props = self.do_refinement(props, next_image_fn, self.refinement_net)
        props = self.add_ReID(props, next_image_fn, self.ReID_net)
        self.cand_masks = decode_segmentations([p["segmentation"] for p in props], device=self.device)
        self.cand_emb = _f64(np.array([np.asarray(p["ReID"], np.float64) for p in props]), self.device)
        if self.record:
            _log_engine_calls(self.engine_log, next_image_fn, np.array(boxes), self.cand_masks.cpu().numpy(), self.cand_emb.cpu().numpy())


def parse_fresh(props: Sequence[Dict]) -> Dict[str, object]:
    """The host half of one seat's fresh proposals for ``TrackerGroup.step`` (pure host work: ``track --lockstep`` runs it ahead on the
    io pool): run boundaries, scores and embeddings as arrays."""
    segs = [p["segmentation"] for p in props]
    assert all(list(sg["size"]) == list(segs[0]["size"]) for sg in segs), "masks of one frame have one size"
    pool, offsets = boundaries_from_segmentations(segs)
    return {"F": len(props), "size": tuple(int(x) for x in segs[0]["size"]) if segs else None, "pool": pool, "offsets": offsets,
            "score": np.array([float(p["score"]) for p in props], np.float64),
            "emb": np.array([np.asarray(p["ReID"], np.float64) for p in props], np.float64).reshape(len(props), EMB)}


class Seat:
    """One of a ``TrackerGroup``'s places: the video in it (``T`` objects, 0 = empty) and what ``Tracker`` keeps per video besides
    the arrays -- ``ids``, ``evaluator``, ``on_idmap``, ``engine_log``."""

    def __init__(self, group: "TrackerGroup", index: int):
        self.group, self.index = group, index
        self.T = 0
        self.ids: List = []
        self.engine_log: List[Dict] = []
        self.evaluator = None                     # as Tracker.evaluator: handed the seat's view of every id map right after the paint
        self.on_idmap: Optional[Callable] = None  # as Tracker.on_idmap

    def add_templates(self, new_templates: List[Dict], image_fn: Optional[str]) -> None:
        """``Tracker.add_templates`` for the video that takes this (empty) seat: the host route, once per video."""
        self.group._seat_video(self.index, new_templates, image_fn)

    def clear(self) -> None:
        """The video has ended: the seat is empty and may take the next one."""
        self.group._vacate(self.index)
        self.evaluator = self.on_idmap = None
        self.engine_log = []


class TrackerGroup(_TrackerBase):
    """``Tracker.step_resident``'s work for up to 8 videos of one frame size in lockstep: a step advances every occupied seat by one frame
    with ONE launch each of decode, overlap, scores, paint and warp (the ``*_seats_*`` entry points), one ``embed_masks`` and one
    ``refine_group`` over the seats' next frames, and one id-map copy to the host.  The state is pooled in seat order: ``pool`` uint8
    [seats * cap + fresh, h, w] (seat v's candidates from slot v * cap, the step's fresh masks behind them as one block),
    ``templ_emb`` / ``cand_emb`` [sum T,128], ``cand_score`` [sum T] float64, ``ids_dev`` int32 [sum T].  ``cap`` = the refinement plan's
    boxes per frame (``_bucket`` of the largest T, ``max_objects`` if the caller knows it): fixed while the group runs, like G = seats,
    so a seat that empties does not build a new plan.  With one seat the plans and launches are ``Tracker``'s and so are the bytes; with
    more, the nets see other batch sizes (another k-split: posteriors agree to 1e-5, a mask may differ where one is within 1e-4 of 0.5),
    so the promise is the loop of merge.py:69-115 on what the engines returned, not the sequential run's bytes."""

    def __init__(self, refinement_net, ReID_net, seats: int = 2, max_objects: Optional[int] = None, weights=None,
                 score_thresh: float = SCORE_THRESH, device=None, record: bool = False):
        _lib.require_gpu()
        super().__init__()
        from .refinement.driver import RefinementEngine
        from .reid.driver import ReIDEngine
        if not (isinstance(refinement_net, RefinementEngine) and isinstance(ReID_net, ReIDEngine)):
            raise _lib.PremvosError("TrackerGroup needs this package's engines (RefinementEngine, ReIDEngine)")
        if not 1 <= int(seats) <= MAX_SEATS:
            raise ValueError(f"1 to {MAX_SEATS} seats (got {seats})")
        self.refinement_net, self.ReID_net = refinement_net, ReID_net
        self.max_boxes = min(refinement_net.max_boxes, ReID_net.max_boxes)
        self.weights = np.ascontiguousarray(NORMALISED_WEIGHTS if weights is None else weights, dtype=np.float64)
        self.score_thresh = score_thresh
        self.device = _lib.resolve_device(device)
        self.record = record
        self.V = int(seats)
        self.seats = [Seat(self, v) for v in range(self.V)]
        self.max_objects = max_objects
        self.cap = 0
        self.pool = self.templ_emb = self.cand_emb = self.cand_score = self.ids_dev = None
        self._index: Dict = {}

    def seat(self, v: int) -> Seat:
        return self.seats[v]

    def _lo(self, v: int) -> int:
        return sum(s.T for s in self.seats[:v])

    # -- seats ---------------------------------------------------------------------------------------------------------------------
    def _layout(self, h: int, w: int, T: int, fresh: int) -> None:
        """Make or grow the pooled buffers: ``cap`` candidate slots per seat, room for ``fresh`` fresh masks."""
        from .refinement.driver import _bucket
        dev, V = self.device, self.V
        cap = max(self.cap, _bucket(max(T, self.max_objects or 1)))
        if self.pool is None:
            self.h, self.w = h, w
            self.labels = torch.zeros((V, h, w), dtype=torch.uint8, device=dev)
            self.idmap = torch.zeros((V, h, w), dtype=torch.uint8, device=dev)
            self.frames = torch.zeros((V, h, w, 3), dtype=torch.uint8, device=dev)
            self.flows = torch.zeros((V, h, w, 2), dtype=torch.float32, device=dev)
        assert (h, w) == (self.h, self.w), f"the videos of one group have one frame size (got {(h, w)}, the group runs {(self.h, self.w)})"
        fresh_cap = 0 if self.pool is None else self.pool.shape[0] - V * self.cap
        if self.pool is not None and cap == self.cap and fresh <= fresh_cap:
            return
        fresh_cap = max(fresh_cap, 64, fresh + fresh // 2)
        pool = torch.empty((V * cap + fresh_cap, h, w), dtype=torch.uint8, device=dev)
        for v, s in enumerate(self.seats):                                    # (a rare regrow: the occupied seats' candidates move)
            if s.T:
                pool[v * cap:v * cap + s.T].copy_(self.pool[v * self.cap:v * self.cap + s.T])
        if cap != self.cap:
            self.refined = torch.empty((V * cap, h, w), dtype=torch.uint8, device=dev)
            self.warped = torch.zeros((V * cap, h, w), dtype=torch.uint8, device=dev)
            self.boxes = torch.zeros((V, cap, 4), dtype=torch.float32, device=dev)
            self._index = {}
        self.pool, self.cap = pool, cap

    def _seat_video(self, v: int, new_templates: List[Dict], image_fn: Optional[str]) -> None:
        seat = self.seats[v]
        assert seat.T == 0, f"seat {v} is occupied"
        if not new_templates:
            return
        T = len(new_templates)
        if T > self.max_boxes:
            raise _lib.PremvosError(f"{T} objects in one video: the lockstep tracker runs at most {self.max_boxes} (the engines' max_boxes) "
                                    "per launch; run premvos_amd.track without --lockstep for this video")
        if image_fn is not None:
            from .reid.driver import add_ReID
            new_templates = add_ReID(new_templates, image_fn, self.ReID_net)
        if self.record:
            seat.engine_log.append({"call": "reid", "image_fn": image_fn, "ReID": np.array([t["ReID"] for t in new_templates], np.float64)})
        dev = self.device
        h, w = (int(x) for x in new_templates[0]["segmentation"]["size"])
        self._layout(h, w, T, 0)
        decode_segmentations([t["segmentation"] for t in new_templates], out=self.pool[v * self.cap:v * self.cap + T])
        emb = _f64(np.array([np.asarray(t["ReID"], np.float64) for t in new_templates]), dev)
        score = _f64([float(t["score"]) for t in new_templates], dev)
        ids = torch.tensor([int(t["id"]) for t in new_templates], dtype=torch.int32, device=dev)
        lo = self._lo(v)

        def insert(a, new):
            return new if a is None or a.shape[0] == 0 else torch.cat([a[:lo], new, a[lo:]])
        self.templ_emb, self.cand_emb = insert(self.templ_emb, emb), insert(self.cand_emb, emb.clone())
        self.cand_score, self.ids_dev = insert(self.cand_score, score), insert(self.ids_dev, ids)
        seat.ids = [t["id"] for t in new_templates]
        seat.T = T

    def _vacate(self, v: int) -> None:
        seat = self.seats[v]
        if seat.T:
            lo, hi = self._lo(v), self._lo(v) + seat.T
            self.templ_emb, self.cand_emb = torch.cat([self.templ_emb[:lo], self.templ_emb[hi:]]), torch.cat([self.cand_emb[:lo], self.cand_emb[hi:]])
            self.cand_score, self.ids_dev = torch.cat([self.cand_score[:lo], self.cand_score[hi:]]), torch.cat([self.ids_dev[:lo], self.ids_dev[hi:]])
        seat.T, seat.ids = 0, []

    def _indices(self, adv: Sequence[int]) -> Dict[str, object]:
        """What a step's advance needs in device memory besides the arrays, per (seating, advancing seats): uploaded when either changes."""
        key = (tuple(s.T for s in self.seats), tuple(adv))
        idx = self._index.get(key)
        if idx is None:
            dev = self.device
            occupied = [v for v in range(self.V) if self.seats[v].T]
            seat_of = [v for v in adv for _ in range(self.seats[v].T)]
            rows = [self._lo(v) + t for v in adv for t in range(self.seats[v].T)]
            idx = {"seat_of": torch.tensor(seat_of, dtype=torch.int32, device=dev),            # frame_of_slot and flow_of_mask
                   "rows": None if list(adv) == occupied else torch.tensor(rows, dtype=torch.int64, device=dev),
                   "box": torch.tensor([v * self.cap + t for v in adv for t in range(self.seats[v].T)], dtype=torch.int64, device=dev),
                   "counts": torch.tensor([self.seats[v].T if v in adv else 0 for v in range(self.V)], dtype=torch.int32, device=dev)}
            if len(self._index) >= 64:
                self._index.clear()
            self._index[key] = idx
        return idx

    # -- one frame of every occupied seat ----------------------------------------------------------------------------------------------
    def step(self, fresh_per_seat: Sequence, flows: Sequence, next_frames: Sequence) -> Dict[str, object]:
        """One frame of every occupied seat.  Per seat (entries of empty seats are ignored): ``fresh_per_seat[v]`` the frame's fresh
        proposals (``read_props``' list, or ``parse_fresh`` of it), ``flows[v]`` ([h,w,2] array / CUDA tensor / .flo name; None: the seat
        does not advance -- its video's last frame) and ``next_frames[v]`` (image name, uint8 [h,w,3] array or CUDA tensor).
        Everything is queued on the current stream; nothing is copied to the host but the id maps, as ONE [seats,h,w] copy into a
        page-locked ring buffer with an event.  The step itself never waits for the GPU; what goes UP from pageable host memory (the fresh
        proposals' arrays, and flows / frames given as arrays or names, as ``do_videos_lockstep`` gives them) is copied as ``Tracker.step``
        copies it, and the runtime finishes such a copy on the host -- only CUDA tensors make the whole step asynchronous.  -> {"idmap": ``IdMapSlot`` (``wait()`` -> the [seats,h,w] array; ``release()`` when
        done), "seats": per seat None or, with ``record``, host copies of "selected", "weighted", "planes", "final_score",
        "object_score", "labels"}.  A seat whose video has ended is emptied with ``seat(v).clear()`` between steps."""
        V, dev, cap = self.V, self.device, self.cap
        occupied = [v for v in range(V) if self.seats[v].T]
        assert occupied, "no templates: seat a video first (seat(v).add_templates)"
        adv = [v for v in occupied if flows[v] is not None]
        h, w = self.h, self.w
        parsed = {v: (fresh_per_seat[v] if isinstance(fresh_per_seat[v], dict) else parse_fresh(fresh_per_seat[v] or [])) for v in occupied}
        assert all(p["size"] in (None, (h, w)) for p in parsed.values()), "masks of one group have one size"
        nF = sum(p["F"] for p in parsed.values())
        self._layout(h, w, 0, nF)
        rows, at = [], V * cap
        for v in range(V):
            F = parsed[v]["F"] if v in parsed else 0
            rows.append((self.seats[v].T, F, v * cap, at))
            at += F
        st = SeatTable(rows)
        fresh_score, fresh_emb = self._decode_fresh([parsed[v] for v in occupied])
        self._tick("decode")
        ov = mask_overlap_seats(self.pool, st)
        self._tick("overlap")
        s = track_scores_seats(ov, self.cand_score, self.cand_emb, self.templ_emb, fresh_score, fresh_emb, st, self.weights, self.score_thresh)
        self._tick("scores")
        # the (labels == t + 1) planes: the advancing seats' first, packed in seat order (what the warp and the nets read)
        slots, at = np.zeros((V,), np.int32), 0
        for v in adv + [u for u in occupied if u not in adv]:
            slots[v] = at
            at += self.seats[v].T
        nT, nA = at, sum(self.seats[v].T for v in adv)
        track_paint_seats(self.pool, st, s["selected"], s["final_score"], self.ids_dev, slots, self.labels, self.idmap, self.refined)
        slot = self._idmap_slot(V, h, w)
        slot.buf.copy_(self.idmap, non_blocking=True)
        slot.event.record(torch.cuda.current_stream(dev))
        for v in occupied:
            if self.seats[v].evaluator is not None:
                self.seats[v].evaluator.frame(self.idmap[v])
            if self.seats[v].on_idmap is not None:
                self.seats[v].on_idmap(self.idmap[v])
        self._tick("paint")
        out: Dict[str, object] = {"idmap": slot, "seats": [None] * V}
        if self.record:
            for v in occupied:
                out["seats"][v] = self._seat_record(st, s, v)
        if not adv:
            return out
        idx = self._indices(adv)
        for v in adv:
            self._upload(v, flows[v], next_frames[v])
        self._advance_seats(idx, nA, s["final_score"], self.flows, self.frames, [(v, next_frames[v]) for v in adv])
        return out

    # -- what a step of this group and of ``SearchGroup`` share ------------------------------------------------------------------------
    def _decode_fresh(self, parsed: Sequence[Dict]):
        """The step's fresh proposals (``parse_fresh`` dicts in seat order; ``_layout`` has made room) decoded into the pool's fresh
        block as one run of masks -> their (``fresh_score`` [sum F], ``fresh_emb`` [sum F,128]) in device memory, (None, None) without any."""
        live = [p for p in parsed if p["F"]]
        if not live:
            return None, None
        at = self.V * self.cap
        starts = np.cumsum([0] + [len(p["pool"]) for p in live])
        offsets = np.concatenate([p["offsets"][:-1].astype(np.int64) + s for p, s in zip(live, starts)] + [starts[-1:]]).astype(np.int32)
        decode_boundaries(np.concatenate([p["pool"] for p in live]), offsets, self.h, self.w, out=self.pool[at:at + sum(p["F"] for p in live)])
        return _f64(np.concatenate([p["score"] for p in live]), self.device), _f64(np.concatenate([p["emb"] for p in live]), self.device)

    def _seat_record(self, st: SeatTable, s: Dict[str, torch.Tensor], v: int) -> Dict[str, np.ndarray]:
        """``record``: host copies of seat ``v``'s part of the step's scores, and of its "labels"."""
        rec = {k: x.cpu().numpy() for k, x in st.views(s, v).items()}
        rec["labels"] = self.labels[v].cpu().numpy()
        return rec

    def _upload(self, v: int, flow, next_frame) -> None:
        """Seat ``v``'s flow and next frame (as ``step`` takes them) into ``flows[v]`` / ``frames[v]``."""
        from . import jpeg
        self.flows[v].copy_(_flow_tensor(flow), non_blocking=True)
        self.frames[v].copy_(jpeg.to_device(_frame_array(next_frame), self.device))

    def _advance_seats(self, idx: Dict[str, object], nA: int, final_score: torch.Tensor, flows: torch.Tensor, frames: torch.Tensor,
                       advancing: Sequence) -> None:
        """The advance of a step, merge.py:98-102 for every advancing seat at once: the painted planes ``refined[:nA]`` warped by
        ``flows`` (premvos_mask_warp_seats_u8), embedded on ``frames`` (``embed_masks``), their next 'score' and boxes
        (premvos_track_next_f32), refined on the group's ``self.frames`` (``refine`` with one seat, ``refine_group`` with more) into the
        candidate slots of the pool, and with ``record`` the seats' ``engine_log`` records.  ``idx``: ``_indices``' dict ("seat_of" indexes
        ``flows`` and ``frames``; "rows" None: every occupied seat advances); ``final_score`` [sum T]: the step's, in seat order;
        ``advancing``: (seat, its next frame's name for the log) in seat order."""
        from .reid.driver import _bucket as _reid_bucket
        V, cap, h, w = self.V, self.cap, self.h, self.w
        warped = mergetrack.warp_masks_seats(self.refined[:nA], idx["seat_of"], flows, out=self.warped[:nA])
        self._tick("warp")
        # as in step_resident: the ReID plan finds the warped masks' boxes itself; an empty warped mask gets the embedding of the box 0 0 0 0
        if nA <= self.ReID_net.max_boxes:
            emb, bbox = self.ReID_net.net.embed_masks(frames, warped, idx["seat_of"], max_slots=_reid_bucket(nA), feed=True)
        else:
            emb, bbox = self.ReID_net.embed_masks(frames, warped, idx["seat_of"], feed=True)
            bbox = bbox.contiguous()
        cand_emb = emb.to(torch.float64)
        cand_score, yx = track_next(final_score if idx["rows"] is None else final_score.index_select(0, idx["rows"]), bbox)
        self._tick("boxes+reid")
        if V == 1:                                                            # Tracker's own plan and launch
            from .refinement.driver import _bucket
            p = self.refinement_net.net.refine(self.frames[0], yx, max_boxes=_bucket(nA))
            self.pool[:nA].copy_(p.mask[:nA])
        else:
            self.boxes.view(-1, 4).index_copy_(0, idx["box"], yx)
            p = self.refinement_net.net.refine_group(self.frames, self.boxes, idx["counts"])
            if idx["rows"] is None:                                           # refined masks straight into the candidate slots
                self.pool[:V * cap].view(V, cap, h, w).copy_(p.mask_g)
            else:                                                             # (a seat that stays keeps its candidates)
                for v, _ in advancing:
                    self.pool[v * cap:v * cap + self.seats[v].T].copy_(p.mask_g[v, :self.seats[v].T])
        if idx["rows"] is None:
            self.cand_emb, self.cand_score = cand_emb, cand_score
        else:
            self.cand_emb.index_copy_(0, idx["rows"], cand_emb)
            self.cand_score.index_copy_(0, idx["rows"], cand_score)
        self._tick("refine")
        if self.record:
            at = 0
            bbox_h, emb_h = bbox.cpu().numpy(), cand_emb.cpu().numpy()
            for v, image_fn in advancing:
                T = self.seats[v].T
                _log_engine_calls(self.seats[v].engine_log, image_fn, bbox_h[at:at + T].copy(), self.pool[v * cap:v * cap + T].cpu().numpy(),
                                  emb_h[at:at + T].copy())
                at += T


class SearchGroup(TrackerGroup):
    """``track --search W``: the seats of a ``TrackerGroup`` hold ONE video under up to 8 weight sets (what MergeTrack/oldmerge.py:225-227,
    253-255 does one full run per set at a time).  Shared by the seats: the frame's fresh proposals (parsed once, decoded once into the
    pool's one fresh block, which every seat's table row points at), the flow (``flows[:1]``), the next frame, the annotation and the
    templates' embeddings (``add_ReID`` once).  Per seat: the candidates, the scores, the selection, the painted planes and their counts
    against the annotation (premvos_track_eval_seats_i64 into ``counts`` int64 [seats,frames,T,3], which stays in HBM until the video
    ends).  One launch per step of premvos_mask_overlap_seats_u8, premvos_track_scores_sets_f64, premvos_track_paint_seats_u8,
    premvos_track_eval_seats_i64, premvos_mask_warp_seats_u8, of ``embed_masks`` (one frame, seats x T masks) and of ``refine_group``
    (the frame replicated on the device into the group's [seats,h,w,3] buffer: the plans are ``TrackerGroup``'s).  With one seat the plans
    and launches are ``Tracker``'s and so are the bytes; with more, a seat promises the loop of merge.py:69-115 on what the engines
    returned to it, under its weights."""

    def __init__(self, refinement_net, ReID_net, sets: int = 1, score_thresh: float = SCORE_THRESH, device=None, record: bool = False):
        super().__init__(refinement_net, ReID_net, seats=sets, score_thresh=score_thresh, device=device, record=record)
        self.weight_sets: Optional[np.ndarray] = None
        self.counts: Optional[torch.Tensor] = None
        self.t = 0

    def seat_video(self, templates: List[Dict], image_fn: Optional[str], weight_sets, frames: int) -> None:
        """The video's first-frame objects take every seat: ``add_ReID`` and the decode run once (seat 0, ``TrackerGroup``'s route), the
        other seats get copies.  ``weight_sets`` [seats,5]: used as given, like ``Tracker(weights=)`` (``live_search_weights``' rows are
        normalised; dividing set 0 by its sum once more would move its last bits away from ``NORMALISED_WEIGHTS``); ``frames``: the
        video's length (``counts``)."""
        assert all(s.T == 0 for s in self.seats), "the group is occupied: end_video first"
        ws = np.asarray(weight_sets, np.float64).reshape(-1, 5)
        assert ws.shape[0] == self.V and np.isfinite(ws).all() and (ws >= 0).all() and (ws.sum(axis=1) > 0).all(), ws
        self.weight_sets = np.ascontiguousarray(ws)
        self.max_objects = max(self.max_objects or 1, len(templates))
        self._seat_video(0, templates, image_fn)
        T, cap, V = self.seats[0].T, self.cap, self.V
        assert T > 0, "a video without templates has nothing to search"
        for v in range(1, V):
            self.pool[v * cap:v * cap + T].copy_(self.pool[:T])
            self.seats[v].T, self.seats[v].ids = T, list(self.seats[0].ids)
            self.seats[v].engine_log = [dict(c) for c in self.seats[0].engine_log]
        if V > 1:
            self.templ_emb, self.cand_emb = self.templ_emb.repeat(V, 1), self.cand_emb.repeat(V, 1)
            self.cand_score, self.ids_dev = self.cand_score.repeat(V), self.ids_dev.repeat(V)
        self.counts = torch.zeros((V, int(frames), T, 3), dtype=torch.int64, device=self.device)
        self.t = 0

    def end_video(self) -> np.ndarray:
        """-> ``counts`` on the host (int64 [seats,frames,T,3]: the one copy of the video); the seats are empty again."""
        counts = self.counts.cpu().numpy()
        for s in self.seats:
            s.clear()
        self.counts, self.weight_sets = None, None
        return counts

    def _search_indices(self, T: int) -> Dict[str, torch.Tensor]:
        key = ("search", T)
        idx = self._index.get(key)
        if idx is None:
            dev, V = self.device, self.V
            idx = {"seat_of": torch.zeros((V * T,), dtype=torch.int32, device=dev),             # every mask: flow 0, frame 0
                   "rows": None,                                                                # every seat advances
                   "box": torch.tensor([v * self.cap + t for v in range(V) for t in range(T)], dtype=torch.int64, device=dev),
                   "counts": torch.full((V,), T, dtype=torch.int32, device=dev)}
            self._index[key] = idx
        return idx

    def _after_paint(self, gt, slots: np.ndarray, T: int) -> None:
        """What a step does with the seats' painted planes and id maps before the seats advance: here, the counts against ``gt``."""
        track_eval_seats(self.refined, _gt_idmap(gt, (self.h, self.w), "the weight search").to(self.device).contiguous(), slots, T, self.counts,
                         self.t)
        self.t += 1
        self._tick("eval")

    def step(self, fresh, flow, next_frame, gt) -> Dict[str, object]:  # noqa: D401 -- one frame of the video, for every weight set
        """One frame under every weight set: ``fresh`` the frame's proposals (``read_props``' list or ``parse_fresh`` of it), ``flow`` /
        ``next_frame`` as one seat's of ``TrackerGroup.step`` (``flow`` None: the video's last frame), ``gt`` the frame's annotation id map
        (uint8 [h,w] array or CUDA tensor).  Nothing returns to the host; with ``record`` -> {"seats": per seat host copies of "selected",
        "weighted", "planes", "final_score", "object_score", "labels" and "idmap" (no PNG is written)}."""
        V, cap = self.V, self.cap
        T = self.seats[0].T
        assert T and self.counts is not None, "no templates: seat_video first"
        h, w = self.h, self.w
        parsed = fresh if isinstance(fresh, dict) else parse_fresh(fresh or [])
        assert parsed["size"] in (None, (h, w)), "masks of one group have one size"
        F = parsed["F"]
        self._layout(h, w, 0, F)
        st = SeatTable([(T, F, v * cap, V * cap) for v in range(V)])                            # every seat: the ONE fresh block
        fresh_score, fresh_emb = self._decode_fresh([parsed])
        self._tick("decode")
        ov = mask_overlap_seats(self.pool, st)
        self._tick("overlap")
        s = track_scores_sets(ov, self.cand_score, self.cand_emb, self.templ_emb, fresh_score, fresh_emb, st, self.weight_sets, self.score_thresh)
        self._tick("scores")
        slots = (np.arange(V) * T).astype(np.int32)
        nA = V * T
        track_paint_seats(self.pool, st, s["selected"], s["final_score"], self.ids_dev, slots, self.labels, self.idmap, self.refined)
        self._tick("paint")
        self._after_paint(gt, slots, T)
        out: Dict[str, object] = {"seats": [None] * V}
        if self.record:
            for v in range(V):
                out["seats"][v] = dict(self._seat_record(st, s, v), idmap=self.idmap[v].cpu().numpy())
        if flow is None:
            return out
        idx = self._search_indices(T)
        self._upload(0, flow, next_frame)                                     # the seats share flow 0 and frame 0
        if V > 1:                                                             # refine_group's [V,h,w,3]: replicated on the device
            self.frames[1:].copy_(self.frames[:1].expand(V - 1, h, w, 3))
        self._advance_seats(idx, nA, s["final_score"], self.flows[:1], self.frames[:1], [(v, next_frame) for v in range(V)])
        return out


class EnsembleGroup(SearchGroup):
    """``track --ensemble``: ``SearchGroup``'s seats -- one video under 2 to 8 weight sets, every seat taking the steps it takes in the
    search -- and, instead of the counts against an annotation, after every paint one premvos_idmap_vote_u8 over the seats' id maps
    (``self.idmap`` [V,h,w]) into frame t of ``stack`` uint8 [N,h,w] and into ``hist`` int64 [V+1], both in HBM until the video ends.
    The combination of MergeTrack/oldmerge.py:129-131,220-224's runs under to_ensemble/<n>/: K full runs, then combine -- every seat
    propagates ITS OWN selection, the vote feeds nothing back.  Set 0 breaks ties.  No annotation is read."""

    def seat_video(self, templates: List[Dict], image_fn: Optional[str], weight_sets, frames: int) -> None:
        super().seat_video(templates, image_fn, weight_sets, 0)               # (no counts: N = 0)
        self.stack = torch.empty((int(frames), self.h, self.w), dtype=torch.uint8, device=self.device)
        self.votes = torch.empty((self.h, self.w), dtype=torch.uint8, device=self.device)
        self.hist = torch.zeros((self.V + 1,), dtype=torch.int64, device=self.device)

    def end_video(self):
        """-> (``stack`` uint8 [N,h,w], ``hist`` int64 [V+1]), both in HBM; the seats are empty again."""
        super().end_video()
        stack, hist = self.stack, self.hist
        self.stack = self.votes = self.hist = None
        return stack, hist

    def _after_paint(self, gt, slots: np.ndarray, T: int) -> None:
        assert self.t < self.stack.shape[0], "more steps than the video has frames"
        vote_idmaps(self.idmap, out=self.stack[self.t], votes=self.votes, hist=self.hist)
        self.t += 1
        self._tick("vote")

    def step(self, fresh, flow, next_frame, gt=None) -> Dict[str, object]:
        """``SearchGroup.step`` without an annotation; frame t of ``stack`` is the vote over the seats' id maps."""
        return super().step(fresh, flow, next_frame, None)


def _frame_paths(image_fn: str, lay: Dict[str, str]):
    """-> the frame's annotation, proposal, flow and PNG file names under the roots of ``lay`` (``_layout``'s keys)"""
    stem = os.path.splitext(os.path.relpath(image_fn, lay["images"]))[0]
    return (os.path.join(lay["anns"], stem + ".png"), os.path.join(lay["props"], stem + ".json"), os.path.join(lay["flows"], stem + ".flo"),
            os.path.join(lay["out"], stem + ".png"))


def missing_annotations(image_fn_list: Sequence[str], images: str, anns: str) -> List[str]:
    """The annotation PNGs the oracle merge would read for these frames and does not find."""
    fns = [_frame_paths(fn, {"images": images, "anns": anns, "props": "", "flows": "", "out": ""})[0] for fn in image_fn_list]
    return [fn for fn in fns if not os.path.isfile(fn)]


def require_annotations(image_fn_list: Sequence[str], images: str, anns: str, name: str, what: str) -> None:
    """Refuse the video ``name`` when ``missing_annotations`` finds any; ``what``: who asks, as a clause ("the oracle merge needs")."""
    lacking = missing_annotations(image_fn_list, images, anns)
    if lacking:
        raise _lib.PremvosError(f"{name}: {what} an annotation for every frame; missing: " + ", ".join(lacking))


def do_video(video_dir: str, images: str, anns: str, props: str, flows: str, out: str, refinement_net, ReID_net,
             do_refinement: Optional[Callable] = None, add_ReID: Optional[Callable] = None, resident: bool = True, writer=None,
             record: bool = False, tracker: Optional[Tracker] = None, eval_dir: Optional[str] = None,
             overlay_dir: Optional[str] = None, combine: str = "argmax", oracle: bool = False, viz_dir: Optional[str] = None) -> List[Dict]:
    """merge.py:69-115 for the frames ``video_dir``*.jpg: one PNG per frame under ``out``.  ``images`` / ``anns`` / ``props`` /
    ``flows`` / ``out`` are the five roots the reference keeps in module globals.  PNGs are written on ``writer`` (an
    ``io_pipeline.Writer``; None: one of its own, closed before returning).  -> one dict per frame ("image_fn", "png_fn" and, with
    ``record``, host copies of the selection, the scores and the id map).  ``eval_dir``: also score the id maps against the video's
    annotations while they are in HBM (premvos_amd.evaluate.LoopEval) and write ``eval_dir``/<video>.json; the PNGs are the same.
    ``overlay_dir``: also one JPEG per frame under it, the frame with the id map's objects tinted (premvos_amd.overlay: blended and
    DCT-coded on the GPU from the id map in HBM, Huffman-coded on ``writer``); the PNGs are the same.
    ``combine`` / ``oracle``: ``Tracker``'s two opt-in modes (a ``tracker`` handed in brings its own); the oracle reads
    ``anns``/<video>/<frame>.png for EVERY frame and refuses a video that lacks one.
    ``viz_dir``: also one score sheet per frame under it (``viz_scores``, merge_functions.py:547-611; premvos_amd.viz: drawn and DCT-coded
    on the GPU right after the scores, Huffman-coded on ``writer``); needs an annotation for EVERY frame, like the oracle; the PNGs are
    the same.  A video without templates has no scores and gets no sheets."""
    from . import io_pipeline as iop
    if viz_dir is not None and not resident:
        raise _lib.PremvosError("viz_dir needs the resident tracker (the sheets are drawn from the scores in device memory)")
    if eval_dir is not None and not resident:
        raise _lib.PremvosError("eval_dir needs the resident tracker (the id maps are scored in device memory)")
    if (combine != "argmax" or oracle) and not resident:
        raise _lib.PremvosError("combine / oracle need the resident tracker (the dict form has the functions: calculate_gt_scores, "
                                "probabilitic_combination)")
    own = writer is None
    writer = iop.Writer() if own else writer
    log: List[Dict] = []
    lay = {"images": images, "anns": anns, "props": props, "flows": flows, "out": out}
    try:
        image_fn_list = sorted(glob.glob(video_dir + "*"))
        if resident:
            tr = tracker or Tracker(refinement_net, ReID_net, do_refinement, add_ReID, record=record, combine=combine, oracle=oracle,
                                    viz=viz_dir is not None)
            if tr.oracle:
                require_annotations(image_fn_list, images, anns, video_dir, "the oracle merge needs")
            if viz_dir is not None:
                if not tr.viz:
                    raise _lib.PremvosError("viz_dir: the tracker handed in was made without viz=True")
                require_annotations(image_fn_list, images, anns, video_dir, "the score sheets need")
        else:
            _lib.require_gpu()
            do_ref, add_reid = _default_engine_calls(do_refinement, add_ReID)
            templates: List[Dict] = []
            next_props: List[Dict] = []
        sink = VideoOut(os.path.relpath(video_dir, images).strip("/"), out, writer, tr.device if resident else None, anns, eval_dir, overlay_dir)
        for image_id, image_fn in enumerate(image_fn_list):
            ann_fn, prop_fn, flow_fn, png_fn = _frame_paths(image_fn, lay)
            stem = os.path.splitext(os.path.basename(image_fn))[0]
            rec: Dict[str, object] = {"image_fn": image_fn, "png_fn": png_fn}
            idmap = idmap_dev = None
            has_flow = os.path.exists(flow_fn) and image_id + 1 < len(image_fn_list)
            new_templates = read_ann(ann_fn) if os.path.exists(ann_fn) and "00000.jpg" in image_fn else []
            if resident:
                tr.add_templates(new_templates, image_fn)
                if eval_dir is not None and image_id == 0:
                    tr.evaluator = sink.open(tr.T)
                if tr.T:
                    if tr.evaluator is not None:
                        tr.evaluator.expect(stem)
                    gt = None
                    if tr.oracle or viz_dir is not None:
                        from .evaluate import _read_ids
                        gt = _read_ids(ann_fn)                                # (the read of evaluate.LoopEval)
                    if viz_dir is not None:
                        from . import viz
                        tr.on_sheet = lambda sheet, fn=sink.jpg_path(stem, viz_dir): viz.write_sheet(fn, sheet, writer)
                    r = tr.step(read_props(prop_fn), flow_fn if has_flow else None, image_fn_list[image_id + 1] if has_flow else None, gt=gt,
                                **({"frame": image_fn} if viz_dir is not None else {}))
                    idmap_dev = r.pop("idmap")
                    idmap = idmap_dev.cpu().numpy()
                    rec.update(r)
            else:
                if new_templates:
                    new_templates = add_reid(new_templates, image_fn, ReID_net)
                    templates = templates + copy(new_templates)
                    next_props = next_props + copy(new_templates)
                if templates:
                    proposals = next_props + read_props(prop_fn)
                    s = _scores_on_device(proposals, templates)
                    all_scores, weighted = s["planes"].cpu().numpy(), s["weighted"].cpu().numpy()
                    object_scores = all_scores[0] + all_scores[1]
                    selected = calculate_selected_props(proposals, weighted[:, :-1], templates, SCORE_THRESH, object_scores)
                    rec.update({"selected": s["selected"].cpu().numpy(), "weighted": weighted, "planes": all_scores})
                    selected = remove_mask_overlap(selected)
                    if has_flow:
                        next_props = mergetrack.warp_proposals(selected, flow_fn)
                        next_props = do_ref(next_props, image_fn_list[image_id + 1], refinement_net)
                        next_props = add_reid(next_props, image_fn_list[image_id + 1], ReID_net)
                        templates = update_templates(templates, next_props)
                    idmap = np.zeros_like(selected[0]["mask"])
                    for p in selected:
                        idmap[p["mask"].astype(bool)] = p["id"]
                    if overlay_dir is not None and idmap.any():
                        idmap_dev = torch.from_numpy(np.ascontiguousarray(idmap, dtype=np.uint8)).to(_lib.resolve_device(None))
            if idmap is None:                                                 # no templates
                idmap = sink.blank(stem, image_fn)
            else:
                sink.png(stem, idmap)
                sink.overlay(stem, image_fn, idmap_dev)
            if record:
                rec["png"] = idmap
            log.append(rec)
        if sink.evaluator is not None:
            sink.close()
            tr.evaluator = None
    finally:
        if own:
            writer.close()
    return log


# ------------------------------------------------------------------------------------------------------- several videos in lockstep
def plan_lockstep(videos_with_sizes: Sequence, seats: int) -> List:
    """Pure host: (name, (h, w)) pairs -> [((h, w), [names]), ...], the order in which the videos take the seats of
    ``track --lockstep``.  Videos of one frame size form a class (the group's buffers and plans have one size); the classes run one
    after another, ordered by their first name; inside a class the names are sorted, the first ``seats`` of them start together and
    each later one takes the lowest seat that is free when its turn comes.  One seat: every video is a class of its own, in sorted
    order -- today's loop.  The same input gives the same plan."""
    items = sorted((str(n), (int(s[0]), int(s[1]))) for n, s in videos_with_sizes)
    if seats <= 1:
        return [(s, [n]) for n, s in items]
    classes: Dict = {}
    for n, s in items:
        classes.setdefault(s, []).append(n)
    return sorted(classes.items(), key=lambda kv: kv[1][0])


class _Run:
    """One video of ``do_videos_lockstep``: its frames, where it is, what it has logged, where its files go (``sink``)."""

    def __init__(self, name: str, lay: Dict[str, str], sink):
        self.name, self.lay, self.sink = name, lay, sink
        self.video_dir = os.path.join(lay["images"], name) + "/"
        self.fns = sorted(glob.glob(self.video_dir + "*"))
        self.stems = [os.path.splitext(os.path.basename(fn))[0] for fn in self.fns]
        self.k = 0
        self.log: List[Dict] = []
        self.pending = None
        ann_fn = self.paths(0)[0] if self.fns else None
        self.templates = read_ann(ann_fn) if self.fns and os.path.exists(ann_fn) and "00000.jpg" in self.fns[0] else []

    def paths(self, k: int):
        return _frame_paths(self.fns[k], self.lay)

    def inputs(self, k: int):
        """Frame k's host work (runs ahead on the io pool): the parsed proposal file and, when the loop goes on, flow and next frame."""
        _, prop_fn, flow_fn, _ = self.paths(k)
        has_flow = os.path.exists(flow_fn) and k + 1 < len(self.fns)
        fresh = parse_fresh(read_props(prop_fn))
        if not has_flow:
            return fresh, None, None
        return fresh, mergetrack.get_flow(flow_fn), _frame_array(self.fns[k + 1])


def do_videos_lockstep(videos: Sequence[str], lay: Dict[str, str], seats: int, refinement_net, ReID_net, writer, eval_dir: Optional[str] = None,
                       overlay_dir: Optional[str] = None, record: bool = False, timer: Optional[Callable[[str], None]] = None,
                       engine_logs: Optional[Dict[str, List[Dict]]] = None, weights=None) -> Dict[str, List[Dict]]:
    """``do_video`` for ``videos`` (names under ``lay["images"]``; ``lay`` = the five roots of ``_layout``) with up to ``seats`` of them
    in flight on one GPU (``TrackerGroup``), in the order of ``plan_lockstep``.  The next step's proposal files, flows and frames are
    read and parsed on the io pool while the GPU works; the PNGs, eval files and overlays are written on ``writer``.  A video without
    templates gets its all-zero PNGs on the host, one with more objects than the engines' ``max_boxes`` runs through ``do_video``.
    -> {video: one dict per frame, as ``do_video`` returns them}; with ``record``, ``engine_logs[video]`` = what the engines returned for
    it, call by call (``Tracker.engine_log``).  ``weights``: other merge weights than merge.py:119's (``track --live-weights``)."""
    from . import io_pipeline as iop
    logs: Dict[str, List[Dict]] = {}
    sized = []
    for name in videos:
        fns = sorted(glob.glob(os.path.join(lay["images"], name) + "/*"))
        if fns:
            sized.append((name, _image_size(fns[0])))                         # (PIL reads the header only)
        else:
            logs[name] = []
    max_boxes = min(refinement_net.max_boxes, ReID_net.max_boxes)
    alive = lambda: not getattr(writer, "failed", False)                      # noqa: E731
    with iop.thread_pool(max(1, iop.io_threads()), "premvos-lockstep") as pool:
        for size, names in plan_lockstep(sized, seats):
            runs = [_Run(n, lay, VideoOut(n, lay["out"], writer, None, lay["anns"], eval_dir, overlay_dir)) for n in names]
            fit = [r for r in runs if 0 < len(r.templates) <= max_boxes]
            group = TrackerGroup(refinement_net, ReID_net, seats=max(1, min(seats, len(fit))), record=record, weights=weights,
                                 max_objects=max(len(r.templates) for r in fit)) if fit else None
            if group is not None:
                group.timer, group.ring_alive = timer, alive
            V = group.V if group is not None else 0
            waiting, seated = list(runs), [None] * V
            while True:
                for v in range(V + 1):                                        # (the extra round only drains videos that take no seat)
                    while waiting and (v == V or seated[v] is None):
                        run = waiting[0]
                        if run.templates and len(run.templates) <= max_boxes:
                            if v == V:
                                break
                            waiting.pop(0)
                            seat = group.seat(v)
                            seat.add_templates(run.templates, run.fns[0])
                            seat.evaluator = run.sink.open(True)
                            seated[v] = run
                            continue
                        waiting.pop(0)
                        if run.templates:                                     # too many objects for one launch: the sequential loop
                            logs[run.name] = do_video(run.video_dir, lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"], refinement_net,
                                                      ReID_net, writer=writer, record=record, eval_dir=eval_dir, overlay_dir=overlay_dir,
                                                      **({} if weights is None else {"tracker": Tracker(refinement_net, ReID_net, weights=weights, record=record)}))
                            continue
                        run.sink.open(False)
                        for k, image_fn in enumerate(run.fns):                # no templates: all-zero PNGs, on the host
                            zeros = run.sink.blank(run.stems[k], image_fn, size)
                            run.log.append(dict({"image_fn": image_fn, "png_fn": run.paths(k)[3]}, **({"png": zeros} if record else {})))
                        logs[run.name] = run.log
                live = [v for v in range(V) if seated[v] is not None]
                if not live:
                    break
                fresh, flows, nxt = [None] * V, [None] * V, [None] * V
                for v in live:
                    run = seated[v]
                    fresh[v], flows[v], nxt[v] = run.pending.result() if run.pending is not None else run.inputs(run.k)
                    run.pending = None
                    run.sink.expect(run.stems[run.k])
                res = group.step(fresh, flows, nxt)
                for v in live:                                                # the next step's host work, while the GPU runs this one
                    if seated[v].k + 1 < len(seated[v].fns):
                        seated[v].pending = pool.submit(seated[v].inputs, seated[v].k + 1)
                jobs = []
                for v in live:
                    run = seated[v]
                    image_fn, png_fn = run.fns[run.k], run.paths(run.k)[3]
                    rec: Dict[str, object] = {"image_fn": image_fn, "png_fn": png_fn}
                    if record:
                        rec.update(res["seats"][v])
                        rec["png"] = group.idmap[v].cpu().numpy()
                    run.log.append(rec)
                    jobs.append((v, png_fn))
                    if overlay_dir is not None:
                        run.sink.overlay(run.stems[run.k], image_fn, group.idmap[v])
                writer.submit(write_pngs, res["idmap"], jobs)                 # the step's one [seats,h,w] copy: each seat's PNG
                for v in live:
                    run = seated[v]
                    run.k += 1
                    if run.k == len(run.fns):                                 # the video has ended: its seat may take the next one
                        if record and engine_logs is not None:
                            engine_logs[run.name] = list(group.seat(v).engine_log)
                        run.sink.close()
                        logs[run.name] = run.log
                        group.seat(v).clear()
                        seated[v] = None
    return logs


# ------------------------------------------------------------------------------------------------- the live loop's weight search
def live_search_weights(W: int, seed: int = 0) -> np.ndarray:
    """The weight sets of ``track --search W``: ``prewarp.search_weights(W, seed)``'s seeded draws (sets 1 .. W-1 =
    ``default_rng(seed).random(5)``, normalised) behind set 0 = THIS loop's default weights (merge.py:119) -> float64 [W,5]."""
    from . import prewarp as pw
    ws = pw.search_weights(int(W), seed)
    ws[0] = NORMALISED_WEIGHTS
    return ws


def plan_search_rounds(W: int, seats: int = MAX_SEATS) -> List[tuple]:
    """Pure host: W weight sets -> [(first, last + 1), ...], the rounds of at most ``seats`` sets a video is run in, in set order."""
    return [(a, min(a + seats, int(W))) for a in range(0, int(W), seats)]


def search_skip_reason(templates: Sequence[Dict], sizes, max_boxes: int) -> Optional[str]:
    """Pure host: why ``search_video`` leaves a video out (None: it runs)."""
    if not templates:
        return "no templates (frame 00000 has no annotated object)"
    if len(templates) > max_boxes:
        return f"{len(templates)} objects: more than the engines' max_boxes ({max_boxes})"
    if len(set(sizes)) > 1:
        return f"its frames differ in size ({sorted(set(sizes))})"
    return None


def search_video(name: str, lay: Dict[str, str], weight_sets, refinement_net, ReID_net, pool=None, record: bool = False,
                 timer: Optional[Callable[[str], None]] = None) -> Dict[str, object]:
    """eval_video's objective (merge_functions.py:613-634) of the live loop on video ``name`` for every row of ``weight_sets`` [W,5], in
    rounds of at most ``MAX_SEATS`` sets (``SearchGroup``).  Needs an annotation for EVERY frame and the ids 1 .. T0 in frame 0 (object k
    is scored against annotation id k + 1).  The next step's proposal file, flow, frame and annotation are read on ``pool`` (an executor;
    None: inline) while the GPU works, once for all seats.  -> {"scores": float64 [W,T0], "counts": int64 [W,N,T0,3], "frames": N} or
    {"skipped": reason}; with ``record`` also "idmaps" uint8 [W,N,h,w], "logs" [W][N] (the seats' records) and "engine_logs" [W]."""
    from . import prewarp as pw
    from .evaluate import _read_ids
    ws = np.asarray(weight_sets, np.float64).reshape(-1, 5)
    run = _Run(name, lay, None)
    reason = search_skip_reason(run.templates, [_image_size(fn) for fn in run.fns], min(refinement_net.max_boxes, ReID_net.max_boxes))
    if reason is not None:
        return {"skipped": reason}
    require_annotations(run.fns, lay["images"], lay["anns"], name, "the weight search needs")
    pw.first_frame_ids([{"ann": run.templates}])
    N = len(run.fns)

    def inputs(k):
        return run.inputs(k) + (_read_ids(run.paths(k)[0]),)
    counts, idmaps, logs, engine_logs = [], [], [], []
    for lo, hi in plan_search_rounds(len(ws)):
        group = SearchGroup(refinement_net, ReID_net, sets=hi - lo, record=record)
        group.timer = timer
        group.seat_video(run.templates, run.fns[0], ws[lo:hi], N)
        pending, recs = None, [[] for _ in range(lo, hi)]
        for k in range(N):
            fresh, flow, nxt, gt = pending.result() if pending is not None else inputs(k)
            pending = pool.submit(inputs, k + 1) if pool is not None and k + 1 < N else None
            res = group.step(fresh, flow, nxt, gt)
            if record:
                for v, r in enumerate(res["seats"]):
                    recs[v].append(dict(r, image_fn=run.fns[k]))
        if record:
            engine_logs += [list(group.seat(v).engine_log) for v in range(hi - lo)]
            logs += recs
            idmaps += [np.array([r["idmap"] for r in rs]) for rs in recs]
        counts.append(group.end_video())
    counts = np.concatenate(counts)
    out: Dict[str, object] = {"scores": pw.scores_from_counts(counts), "counts": counts, "frames": N}
    if record:
        out.update(idmaps=np.array(idmaps), logs=logs, engine_logs=engine_logs)
    return out


def live_search_result(per_video: Dict[str, Dict], weight_sets, seed: int) -> Dict[str, object]:
    """Pure host: ``search_video``'s results by video name -> the content of output/live_search.json: prewarp_search.json's keys
    ("videos" -> {"scores": [W][T0]}, "weights", "seed", "mean" per set over all objects of all videos, "frames") + "best" (the set with
    the highest mean, the lowest index on a tie; None when nothing was scored) + "skipped" ({video: reason})."""
    ws = np.asarray(weight_sets, np.float64).reshape(-1, 5)
    ran = {n: r for n, r in per_video.items() if "skipped" not in r}
    result: Dict[str, object] = {"videos": {n: {"scores": np.asarray(r["scores"]).tolist()} for n, r in ran.items()}}
    per_set = [[s for v in result["videos"].values() for s in v["scores"][i]] for i in range(len(ws))]
    mean = [float(np.mean(x)) if x else None for x in per_set]
    scored = [i for i, m in enumerate(mean) if m is not None and m == m]
    best = min(scored, key=lambda i: (-mean[i], i)) if scored else None
    result.update(frames=int(sum(r["frames"] for r in ran.values())), weights=ws.tolist(), seed=int(seed), mean=mean, best=best,
                  skipped={n: r["skipped"] for n, r in per_video.items() if "skipped" in r})
    return result


def search_tree(root: str, videos: Sequence[str], W: int, seed: int, refinement_net, ReID_net, lay: Optional[Dict[str, str]] = None,
                json_name: str = "live_search.json") -> Dict[str, object]:
    """``track --search W`` under ``root``: every video through ``search_video`` with ``live_search_weights(W, seed)``; writes
    output/live_search.json (``json_name``: under ``--refine-tta`` live_search_tta.json) and nothing else (no PNG, eval file or overlay)."""
    from . import io_pipeline as iop
    lay = _layout(root) if lay is None else lay
    ws = live_search_weights(W, seed)
    per_video = {}
    with iop.thread_pool(max(1, iop.io_threads()), "premvos-search") as pool:
        for name in videos:
            per_video[name] = search_video(name, lay, ws, refinement_net, ReID_net, pool=pool)
    result = live_search_result(per_video, ws, seed)
    os.makedirs(os.path.join(root, "output"), exist_ok=True)
    with open(os.path.join(root, "output", json_name), "w") as f:
        json.dump(result, f, indent=1)
    return result


# ------------------------------------------------------------------------------------------------- the ensemble of several weight sets
def parse_ensemble_sets(text: str) -> np.ndarray:
    """Pure host: ``--ensemble``'s "a,b,c,d,e;a,b,c,d,e;..." -> float64 [K,5], K = 2 .. 8, each row five non-negative numbers, not all
    zero, divided by its sum (``--live-weights``' rule per row); the list order is the vote's priority.  ValueError otherwise."""
    rows = str(text).split(";")
    if not MIN_ENSEMBLE <= len(rows) <= MAX_SEATS:
        raise ValueError(f"{len(rows)} weight sets ({MIN_ENSEMBLE} to {MAX_SEATS} sets a,b,c,d,e, separated by ';')")
    out = []
    for r in rows:
        try:
            w = [float(x) for x in r.split(",")]
        except ValueError:
            w = []
        if not (len(w) == 5 and all(np.isfinite(w)) and min(w) >= 0 and sum(w) > 0):
            raise ValueError(f"{r!r} (five non-negative numbers a,b,c,d,e, not all zero)")
        w = np.array(w, np.float64)
        out.append(w / w.sum())
    return np.array(out)


def select_ensemble(result: Dict[str, object], top: int = DEFAULT_TOP) -> np.ndarray:
    """Pure host: the content of output/live_search.json or output/prewarp_search.json (its keys "weights" [W][5] and "mean" [W]) -> the
    ``top`` rows with the highest mean, best first, the lower index first on a tie, as float64 [top,5] (the rows as the search ran them).
    Rows whose mean is null (or NaN) were not scored and are ignored.  ValueError: ``top`` outside 2 .. 8, fewer than 2 scored rows,
    fewer scored rows than ``top``, or a file without the two keys."""
    if not MIN_ENSEMBLE <= int(top) <= MAX_SEATS:
        raise ValueError(f"--top {top}: an ensemble has {MIN_ENSEMBLE} to {MAX_SEATS} weight sets")
    if not isinstance(result, dict) or "weights" not in result or "mean" not in result:
        raise ValueError('not a search result (no "weights" / "mean": expected output/live_search.json or output/prewarp_search.json)')
    ws, mean = np.asarray(result["weights"], np.float64).reshape(-1, 5), list(result["mean"])
    if len(mean) != len(ws):
        raise ValueError(f'{len(ws)} rows of "weights" but {len(mean)} of "mean"')
    scored = [i for i, m in enumerate(mean) if m is not None and m == m]
    if len(scored) < MIN_ENSEMBLE:
        raise ValueError(f"{len(scored)} scored weight sets: an ensemble needs at least {MIN_ENSEMBLE}")
    if len(scored) < int(top):
        raise ValueError(f"--top {top}: the search scored only {len(scored)} weight sets")
    order = sorted(scored, key=lambda i: (-mean[i], i))[:int(top)]
    rows = ws[order]
    if not (np.isfinite(rows).all() and (rows >= 0).all() and (rows.sum(axis=1) > 0).all()):
        raise ValueError(f"weight sets {order}: five non-negative numbers each, not all zero")
    return np.ascontiguousarray(rows)


def ensemble_result(per_video: Dict[str, Dict], K: int, weights, source) -> Dict[str, object]:
    """Pure host: {video: {"frames": N, "hist": int [K+1]}} -> the content of output/ensemble.json (and of the pre-warp form's and the
    tree tool's files): "videos" -> {"frames", "hist", "unanimous" = hist[K] / pixels: the share of pixels on which all K members
    agree}, "frames", "sets" = K, "weights" (the K rows as run, in vote order; None for trees) and "source" (where the members came from)."""
    videos = {}
    for name, r in per_video.items():
        hist = [int(x) for x in r["hist"]]
        assert len(hist) == K + 1 and hist[0] == 0, hist
        pixels = sum(hist)
        videos[name] = {"frames": int(r["frames"]), "hist": hist, "unanimous": hist[K] / pixels if pixels else None}
    return {"videos": videos, "frames": sum(v["frames"] for v in videos.values()), "sets": int(K),
            "weights": None if weights is None else np.asarray(weights, np.float64).reshape(-1, 5).tolist(), "source": source}


def write_ensemble_json(path: str, result: Dict[str, object]) -> None:
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)


def stack_to_host(stack: torch.Tensor):
    """uint8 [N,h,w] in HBM -> (a page-locked host copy, the event after which it is complete): what ``VideoOut.whole_video`` takes."""
    host = torch.empty(tuple(stack.shape), dtype=torch.uint8, pin_memory=True)
    host.copy_(stack, non_blocking=True)
    ready = torch.cuda.Event()
    ready.record()
    return host, ready


def ensemble_video(name: str, lay: Dict[str, str], weight_sets, refinement_net, ReID_net, pool=None, record: bool = False, writer=None,
                   eval_dir: Optional[str] = None, overlay_dir: Optional[str] = None,
                   timer: Optional[Callable[[str], None]] = None) -> Dict[str, object]:
    """Video ``name`` under every row of ``weight_sets`` [K,5] (K = 2 .. 8, used as given, row 0 breaks ties) in lockstep
    (``EnsembleGroup``), the per-pixel vote of the K id maps of every frame into one [N,h,w] stack in HBM, and at the video's end that
    stack through ``VideoOut.whole_video``: the PNGs under ``lay["out"]``, with ``eval_dir`` / ``overlay_dir`` the count file and the
    overlays.  The next step's proposal file, flow and frame are read on ``pool`` (an executor; None: inline) while the GPU works, once
    for all seats; no annotation but frame 00000's is read.  A video without templates gets all-zero PNGs, as in ``do_video``; one
    ``search_skip_reason`` names for another reason is refused with that reason.  -> {"frames": N, "hist": int64 [K+1] (host)}; with
    ``record`` also "members" uint8 [K,N,h,w], "voted" uint8 [N,h,w] (host copies) and "engine_logs" [K]."""
    from . import io_pipeline as iop
    ws = np.asarray(weight_sets, np.float64).reshape(-1, 5)
    K = len(ws)
    if not MIN_ENSEMBLE <= K <= MAX_SEATS:
        raise ValueError(f"an ensemble has {MIN_ENSEMBLE} to {MAX_SEATS} weight sets (got {K})")
    _lib.require_gpu()
    run = _Run(name, lay, None)
    sizes = [_image_size(fn) for fn in run.fns]
    reason = search_skip_reason(run.templates, sizes, min(refinement_net.max_boxes, ReID_net.max_boxes))
    if reason is not None and run.templates:
        raise _lib.PremvosError(f"{name}: the ensemble does not run this video: {reason}")
    N = len(run.fns)
    own = writer is None
    writer = iop.Writer() if own else writer
    try:
        sink = VideoOut(name, lay["out"], writer, _lib.resolve_device(None), lay["anns"], eval_dir, overlay_dir)
        if not run.templates:                                                 # every member would write zeros: they agree everywhere
            sink.open(0)
            for stem, fn in zip(run.stems, run.fns):
                sink.blank(stem, fn)
            hist = np.zeros(K + 1, np.int64)
            hist[K] = sum(h * w for h, w in sizes)
            out: Dict[str, object] = {"frames": N, "hist": hist}
            if record:
                out.update(members=None, voted=None, engine_logs=[])
            return out
        group = EnsembleGroup(refinement_net, ReID_net, sets=K, record=record)
        group.timer = timer
        group.seat_video(run.templates, run.fns[0], ws, N)
        pending, members = None, [[] for _ in range(K)]
        for k in range(N):
            fresh, flow, nxt = pending.result() if pending is not None else run.inputs(k)
            pending = pool.submit(run.inputs, k + 1) if pool is not None and k + 1 < N else None
            res = group.step(fresh, flow, nxt)
            if record:
                for v, r in enumerate(res["seats"]):
                    members[v].append(r["idmap"])
        engine_logs = [list(group.seat(v).engine_log) for v in range(K)] if record else None
        stack, hist_dev = group.end_video()
        host, ready = stack_to_host(stack)
        sink.whole_video(run.fns, {"idmap": host, "ready": ready, "idmap_dev": stack})
        out = {"frames": N, "hist": hist_dev.cpu().numpy()}
        if record:
            out.update(members=np.array(members), voted=stack.cpu().numpy(), engine_logs=engine_logs)
        return out
    finally:
        if own:
            writer.close()


def ensemble_tree(root: str, videos: Sequence[str], weight_sets, refinement_net, ReID_net, lay: Optional[Dict[str, str]] = None, writer=None,
                  eval_dir: Optional[str] = None, overlay_dir: Optional[str] = None, source: str = "--ensemble",
                  json_name: str = "ensemble.json") -> Dict[str, object]:
    """``track --ensemble`` / ``--ensemble-from`` under ``root``: every video through ``ensemble_video``; the PNGs under
    output/final_ensemble/ (never output/final/) and output/ensemble.json (``ensemble_result``; ``json_name``: under ``--refine-tta``
    ensemble_tta.json)."""
    from . import io_pipeline as iop
    lay = mode_layout(root, ensemble=True) if lay is None else lay
    ws = np.asarray(weight_sets, np.float64).reshape(-1, 5)
    own = writer is None
    writer = iop.Writer() if own else writer
    per_video = {}
    try:
        with iop.thread_pool(max(1, iop.io_threads()), "premvos-ensemble") as pool:
            for name in videos:
                per_video[name] = ensemble_video(name, lay, ws, refinement_net, ReID_net, pool=pool, writer=writer, eval_dir=eval_dir,
                                                 overlay_dir=overlay_dir)
    finally:
        if own:
            writer.close()
    result = ensemble_result(per_video, len(ws), ws, source)
    write_ensemble_json(os.path.join(root, "output", json_name), result)
    return result


# ---------------------------------------------------------------------------------------------------------------- command line
def _layout(root: str) -> Dict[str, str]:
    return {"images": os.path.join(root, "data/DAVIS/JPEGImages/480p") + "/", "anns": os.path.join(root, "data/DAVIS/Annotations/480p") + "/",
            "props": os.path.join(root, "output/intermediate/ReID_proposals") + "/", "flows": os.path.join(root, "output/intermediate/flow") + "/",
            "out": os.path.join(root, "output/final") + "/", "overlay": os.path.join(root, "output/overlay") + "/"}


def mode_suffix(combine: str = "argmax", oracle: bool = False, live_weights: bool = False, ensemble: bool = False, tta: bool = False) -> str:
    """"" for the loop as it always ran, else the name the opt-in modes' outputs carry: "prob", "oracle", "oracle_prob"; "weights" for the
    loop under ``--live-weights``; "ensemble" for the vote of ``--ensemble`` / ``--ensemble-from``; a trailing "tta" for the loop with the
    refinement net under ``--refine-tta`` ("tta", "weights_tta", "prob_tta", ...)."""
    return "_".join(x for x in ("oracle" if oracle else "", "prob" if combine == "probabilistic" else "", "weights" if live_weights else "",
                                "ensemble" if ensemble else "", "tta" if tta else "") if x)


def mode_layout(root: str, combine: str = "argmax", oracle: bool = False, live_weights: bool = False, ensemble: bool = False,
                tta: bool = False) -> Dict[str, str]:
    """``_layout`` with the places of a mode's outputs: "out", "overlay", "viz", "eval" (the per-video count files) and "summary".  The modes
    never write output/final/, output/overlay/, output/eval/ or the live loop's summary."""
    lay, sfx = _layout(root), mode_suffix(combine, oracle, live_weights, ensemble, tta)
    tail = "_" + sfx if sfx else ""
    from .evaluate import SUMMARY
    lay.update({"out": os.path.join(root, "output", "final" + tail) + "/", "overlay": os.path.join(root, "output", "overlay" + tail) + "/",
                "viz": os.path.join(root, "output", "viz" + tail) + "/", "eval": os.path.join(root, "output", "eval" + tail),
                "summary": os.path.join(root, "output", f"premvos_amd_davis_eval{tail}.json") if sfx else os.path.join(root, SUMMARY)})
    return lay


def check_inputs(root: str) -> List[str]:
    """-> what ``main`` would miss under ``root`` (empty = ready)."""
    lay = _layout(root)
    problems = [f"{lay[k]} is missing ({why})" for k, why in
                (("images", "the frames"), ("props", "the ReID stage's proposals: run premvos_amd.stream --reid, or premvos_amd.stream and then premvos_amd.reid.driver, first"),
                 ("flows", "the flow stage's .flo files")) if not os.path.isdir(lay[k])]
    for rel in ("code/refinement_net/configs/live", "code/ReID_net/configs/live"):
        if not os.path.isfile(os.path.join(root, rel)):
            problems.append(f"{os.path.join(root, rel)} is missing (the engine configuration MergeTrack loads)")
    return problems


def tree_videos(lay: Dict[str, str], only: Optional[str] = None) -> List[str]:
    """The videos of the tree (the folders of ReID_proposals), sorted; ``only``: ``--videos``' comma-separated names."""
    videos = sorted(d for d in os.listdir(lay["props"]) if os.path.isdir(os.path.join(lay["props"], d)))
    return [v for v in videos if v in only.split(",")] if only else videos


@contextlib.contextmanager
def _in_code_dir(root: str):
    """The engines are built inside code/: the configs' 'load' paths are relative to it (the reference runs there)."""
    cwd = os.getcwd()
    os.chdir(os.path.join(root, "code"))
    try:
        yield
    finally:
        os.chdir(cwd)


def prewarp_stem(negatives) -> str:
    """what every output name of the pre-warp merge is built on: ``--negatives`` never writes the places of the run without it"""
    return "prewarp" if negatives is None else "prewarp_neg"


def _main_prewarp(ap, a, root: str, weights) -> int:
    """``--prewarp`` / ``--prewarp-search``: premvos_amd.prewarp on the tree; the ReID net only embeds the annotation objects."""
    from . import prewarp as pw
    lay = _layout(root)
    videos = tree_videos(lay, a.videos)
    for v in videos:                                              # (PIL reads the headers only)
        sizes = sorted({_image_size(fn) for fn in glob.glob(os.path.join(lay["images"], v) + "/*")})
        if len(sizes) > 1:
            ap.error(f"argument --prewarp: the frames of {v} differ in size ({sizes}): one pool of masks holds one size")
    _lib.require_gpu()
    from .reid.driver import ReID_net_init
    with _in_code_dir(root):
        ReID_net = ReID_net_init()
    negatives = getattr(a, "negatives", None)
    stem = prewarp_stem(negatives)
    tail = stem + "_ensemble" if a.ensemble_sets is not None else stem                          # (the vote never writes the single merge's places)
    eval_dir = os.path.join(root, "output", "eval_" + tail) if a.eval else None                 # (never the live loop's output/eval/)
    overlay_dir = os.path.join(root, "output", "overlay_" + tail) + "/" if a.overlay else None
    remove_stale(eval_dir, videos)
    if a.ensemble_sets is not None:
        out = os.path.join(root, "output", "final_" + tail) + "/"
        r = pw.run_tree(root, videos, late=a.late_annotations, ReID_net=ReID_net, eval_dir=eval_dir, overlay_dir=overlay_dir,
                        lay=dict(lay, out=out), ensemble_sets=a.ensemble_sets,
                        ensemble_source=f"--ensemble-from {a.ensemble_from}" if a.ensemble_from is not None else "--ensemble",
                        negatives=negatives)
        print(f"premvos_amd.track: videos: {len(videos)}  frames: {r['frames']}  weight sets: {len(a.ensemble_sets)}  ->  {out}"
              + (f"  {overlay_dir}" if overlay_dir else "") + f"  {os.path.join(root, 'output', stem + '_ensemble.json')}")
        if eval_dir is not None:
            summarise(eval_dir, videos, os.path.join(root, "output", f"premvos_amd_davis_eval_{tail}.json"),
                      "premvos_amd.track: pre-warp ensemble:")
        return 0
    r = pw.run_tree(root, videos, weights=weights, late=a.late_annotations, search_sets=a.prewarp_search, seed=a.seed, ReID_net=ReID_net,
                    eval_dir=eval_dir, overlay_dir=overlay_dir, negatives=negatives)
    if a.prewarp_search:
        print(f"premvos_amd.track: videos: {len(videos)}  frames: {r['frames']}  weight sets: {a.prewarp_search}  best mean: "
              f"{max((m for m in r['mean'] if m is not None), default=None)}  ->  {os.path.join(root, 'output', stem + '_search.json')}")
    else:
        print(f"premvos_amd.track: videos: {len(videos)}  frames: {r['frames']}  ->  {os.path.join(root, 'output/final_' + stem) + '/'}"
              + (f"  {overlay_dir}" if overlay_dir else ""))
    if eval_dir is not None:
        summarise(eval_dir, videos, os.path.join(root, "output", f"premvos_amd_davis_eval_{stem}.json"), "premvos_amd.track: pre-warp merge:")
    return 0


def _main_max_reid_distance(a, root: str) -> int:
    """``--max-reid-distance``: premvos_amd.viz.max_reid_distance_tree; only the ReID net is loaded, it embeds the annotation objects."""
    from . import viz
    videos = tree_videos(_layout(root), a.videos)
    _lib.require_gpu()
    from .reid.driver import ReID_net_init
    with _in_code_dir(root):
        ReID_net = ReID_net_init()
    viz.max_reid_distance_tree(root, videos, ReID_net)
    return 0


def _five_weights(ap, flag: str, text: str) -> List[float]:
    """``--weights`` / ``--live-weights``: five non-negative numbers a,b,c,d,e, not all zero"""
    try:
        weights = [float(x) for x in text.split(",")]
        assert len(weights) == 5 and all(np.isfinite(weights)) and min(weights) >= 0 and sum(weights) > 0
    except (ValueError, AssertionError):
        ap.error(f"argument {flag}: invalid value: {text!r} (five non-negative numbers a,b,c,d,e, not all zero)")
    return weights


def refine_tta(a):
    """The namespace's test-time augmentation spec (``--refine-tta``), None when the flag is absent or plain."""
    return getattr(a, "tta", None)


def parse_args(argv: Optional[List[str]] = None):
    """The command line and its refusals (no file is looked at) -> the namespace; ``merge_weights``: ``--weights`` as five floats or None,
    ``live``: ``--live-weights`` normalised (float64 [5]) or None, ``ensemble_sets``: ``--ensemble`` normalised (float64 [K,5]) or None
    (``--ensemble-from``'s file is read by ``main``), ``parser``: for errors that need the tree."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=".")
    ap.add_argument("--videos", default=None, help="comma-separated video names (default: every folder of ReID_proposals)")
    ap.add_argument("--check-only", action="store_true", help="name what is missing and stop")
    ap.add_argument("--eval", action="store_true",
                    help="also score every id map against data/DAVIS/Annotations/480p on the GPU (premvos_amd.evaluate): "
                         "output/eval/<video>.json and output/premvos_amd_davis_eval.json")
    ap.add_argument("--overlay", action="store_true",
                    help="also write every frame with its objects tinted (premvos_amd.overlay: blend + JPEG encode on the GPU, from the "
                         "id map the loop just painted): output/overlay/<video>/<frame>.jpg")
    ap.add_argument("--lockstep", type=int, default=1, choices=range(1, MAX_SEATS + 1), metavar="V",
                    help=f"videos in flight on the GPU (1 to {MAX_SEATS}; default 1: one video after another, the loop as it always ran).  "
                         "V > 1 steps V videos of one frame size together (TrackerGroup): one launch of each of the loop's kernels and of "
                         "each net per step.  It promises the loop of merge.py:69-115 on what the engines returned, not the bytes of the "
                         "sequential run: the nets see another batch size and may pick another k-split (posteriors agree to 1e-5; a mask "
                         "may differ where a posterior is within 1e-4 of 0.5)")
    ap.add_argument("--prewarp", action="store_true",
                    help="the paper's pre-warp merge instead of the live-warp loop (MergeTrack/oldmerge.py, premvos_amd.prewarp): every "
                         "proposal's mask is warped to the next frame once, no network runs in the merge, a video is a handful of launches.  "
                         "Writes output/final_prewarp/<video>/<frame>.png, never output/final/.  Its quality on DAVIS is not measured here")
    ap.add_argument("--weights", default=None, metavar="a,b,c,d,e",
                    help="--prewarp: the five merge weights (objectness, ReID, inverse ReID, mask propagation, inverse mask propagation; "
                         "normalised to sum 1).  Default: oldmerge.py:220-221")
    ap.add_argument("--late-annotations", action="store_true",
                    help="--prewarp: an annotation PNG of a later frame contributes the ids that have not appeared before (default off: "
                         "only 00000's objects, merge.py:78)")
    ap.add_argument("--negatives", nargs="?", const="all", default=argparse.SUPPRESS, metavar="K",      # (absent from the result unless given)
                    help="--prewarp / --prewarp-search: negative first-frame templates (oldmerge.py:43,63-85 use_ff_negative_props): frame "
                         "00000's proposals in descending score that overlap neither an annotated object nor one taken before become "
                         "templates of label 0 -- distractor tracks that take proposals and pixels away from the objects and are never "
                         "written.  K: at most K of them (default: all).  Writes output/final_prewarp_neg/ (and eval_prewarp_neg/, "
                         "overlay_prewarp_neg/, premvos_amd_davis_eval_prewarp_neg.json, prewarp_neg_search.json, final_prewarp_neg_ensemble/, "
                         "prewarp_neg_ensemble.json) and output/prewarp_negatives.json, never output/final_prewarp/.  Its quality on DAVIS "
                         "is not measured here")
    ap.add_argument("--prewarp-search", type=int, default=0, metavar="W",
                    help="score W weight sets with eval_video's objective (merge_functions.py:613-634) instead of writing PNGs: set 0 = the "
                         "default weights, sets 1 .. W-1 = default_rng(--seed).random(5), normalised; needs an annotation for every frame; "
                         "writes output/prewarp_search.json")
    ap.add_argument("--seed", type=int, default=0, help="--prewarp-search / --search: the seed of the random weight sets")
    ap.add_argument("--search", type=int, default=0, metavar="W",
                    help="score W weight sets of the LIVE-warp loop with eval_video's objective (merge_functions.py:613-634) instead of "
                         "writing PNGs -- the random search of oldmerge.py:225-227,253-255 with the W runs of a video in lockstep "
                         f"(SearchGroup, rounds of at most {MAX_SEATS} sets): set 0 = the default weights (merge.py:119), sets 1 .. W-1 = "
                         "default_rng(--seed).random(5), normalised.  The sets share the frame's proposals, flow, frame and annotation; "
                         "candidates, scores and selections are per set.  Needs an annotation for every frame and the ids 1 .. T in "
                         "frame 00000.  A set promises the loop of merge.py:69-115 on what the engines returned to it, not the bytes of "
                         "--live-weights with the same weights (W = 1: the bytes of the plain loop).  Writes output/live_search.json, no PNG")
    ap.add_argument("--live-weights", default=None, metavar="a,b,c,d,e",
                    help="run the live-warp loop with these five merge weights (objectness, ReID, inverse ReID, mask propagation, inverse "
                         "mask propagation; normalised to sum 1) instead of merge.py:119's -- e.g. a row of output/live_search.json.  Works "
                         "with --lockstep, --eval, --overlay and --viz.  Writes output/final_weights/ (and eval_weights/, overlay_weights/, "
                         "viz_weights/, premvos_amd_davis_eval_weights.json), never output/final/")
    ap.add_argument("--combine", default="argmax", choices=COMBINE_MODES,
                    help="probabilistic: the reference's soft merge (merge_functions.py:151-195 probabilitic_combination) instead of argmax + "
                         "overlap removal: a softmax over the candidates at temperature 0.1, a per-pixel weighted average of all candidate "
                         "masks, the argmax over background and objects.  Writes output/final_prob/<video>/<frame>.png, never output/final/")
    ap.add_argument("--oracle", action="store_true",
                    help="the reference's oracle merge (merge_functions.py:78-94 calculate_gt_scores): every score is the IoU of a candidate "
                         "with the annotation of the template's object, read from data/DAVIS/Annotations/480p/<video>/<frame>.png for EVERY "
                         "frame.  With --eval: the J&F the proposals and the warp/refine chain could reach under a perfect selection.  "
                         "Writes output/final_oracle/ (with --combine probabilistic: output/final_oracle_prob/), never output/final/")
    ap.add_argument("--viz", action="store_true",
                    help="also write the reference's score sheet of every frame (merge_functions.py:547-611 viz_scores, premvos_amd.viz): every "
                         "candidate's crop with its mask tinted, under it per template the five score planes, the weighted score and the IoU "
                         "with the annotation as colour cells, a mark on the candidate the weights chose and on the one the annotation would "
                         "choose.  Drawn and DCT-coded on the GPU right after the scores; needs data/DAVIS/Annotations/480p/<video>/<frame>.png "
                         "for EVERY frame.  Writes output/viz/<video>/<frame>.jpg (with a mode: output/viz_<mode>/); the PNGs are the same")
    ap.add_argument("--max-reid-distance", action="store_true",
                    help="instead of merging: MergeTrack/print_max_reid_distance.py on the GPU (premvos_amd.viz) -- per video and per object "
                         "of every annotated frame, the largest ReID distance to any proposal of the video; the number MAX_REID_DISTANCE = 25 "
                         "(merge_functions.py:12, compiled into the score kernels) was read from.  Prints one line per video and the "
                         "maximum, writes output/max_reid_distance.json, writes no PNG and changes no constant")
    ap.add_argument("--ensemble", default=None, metavar="a,b,c,d,e;a,b,c,d,e;...",
                    help=f"run the merge under {MIN_ENSEMBLE} to {MAX_SEATS} weight sets at once and write their per-pixel vote -- the combination "
                         "of the runs MergeTrack/oldmerge.py:129-131,220-224 writes under to_ensemble/<n>/ (EnsembleGroup: the sets of a video "
                         "in lockstep, premvos_idmap_vote_u8 over their id maps after every paint).  The label most sets painted wins a pixel; "
                         "on a tie the set listed FIRST wins, so list the best set first.  The members run independently: each propagates its "
                         "own selection, the vote feeds nothing back.  Each set is normalised to sum 1.  Works with --eval and --overlay.  "
                         "Writes output/final_ensemble/ (and eval_ensemble/, overlay_ensemble/, premvos_amd_davis_eval_ensemble.json) and "
                         "output/ensemble.json, never output/final/.  With --prewarp: the pre-warp merge's sets (one chain launch for all), "
                         "output/final_prewarp_ensemble/ and output/prewarp_ensemble.json, never output/final_prewarp/")
    ap.add_argument("--ensemble-from", default=None, metavar="FILE",
                    help="--ensemble with the --top K best weight sets of a search result: FILE is output/live_search.json or "
                         "output/prewarp_search.json (its keys 'weights' and 'mean'; the highest mean first, the lower index on a tie, rows "
                         "without a mean ignored)")
    ap.add_argument("--top", type=int, default=None, metavar="K",
                    help=f"--ensemble-from: how many sets ({MIN_ENSEMBLE} to {MAX_SEATS}; default {DEFAULT_TOP})")
    ap.add_argument("--refine-tta", default=argparse.SUPPRESS, metavar="SPEC",      # (absent from the namespace unless given: ``refine_tta``)
                    help="run the loop's refinement net with test-time augmentation, DeepLab's multi-scale / flipped inference "
                         "(refinement_net/network/deeplab/model.py:84-160 predict_labels_multi_scale; premvos_amd.refinement.tta): SPEC is a "
                         "list of scales from 0.5, 0.75, 1, 1.25, 1.5, 1.75, optionally followed by +flip, e.g. 0.75,1,1.25+flip -- every "
                         "candidate crop goes through the net once per scale (and once more mirrored) and the members' softmax "
                         "probabilities are averaged.  Costs about (1 + flip) x sum(scale^2) plain refinements.  Works with every flag of "
                         "the live-warp loop.  Writes output/final_tta/ (and eval_tta/, overlay_tta/, viz_tta/, "
                         "premvos_amd_davis_eval_tta.json; after another mode's name: final_weights_tta/, final_prob_tta/, ...; --search and "
                         "--ensemble write live_search_tta.json / ensemble_tta.json), never output/final/.  SPEC 1 is plain inference: the flag is then off.  Its quality on DAVIS is not measured here")
    a = ap.parse_args(argv)
    prewarp = a.prewarp or a.prewarp_search > 0
    suffix = mode_suffix(a.combine, a.oracle)
    a.ensemble_sets = None
    if hasattr(a, "refine_tta"):                                  # -> ``tta``: the spec, None when it stands for plain inference ("1")
        if prewarp:
            ap.error("argument --refine-tta: not with --prewarp / --prewarp-search (no refinement net runs in the pre-warp merge)")
        if a.max_reid_distance:
            ap.error("argument --refine-tta: not with --max-reid-distance (it runs no refinement net)")
        from .refinement import tta as tta_mod
        try:
            a.tta = tta_mod.resolve(a.refine_tta)
        except ValueError as e:
            ap.error(f"argument --refine-tta: invalid value: {e}")
    if a.top is not None and a.ensemble_from is None:
        ap.error("argument --top: only with --ensemble-from")
    if a.ensemble is not None or a.ensemble_from is not None:
        flag = "--ensemble" if a.ensemble is not None else "--ensemble-from"
        for on, why in ((a.ensemble is not None and a.ensemble_from is not None, "--ensemble-from (one source of weight sets: the list or the file)"),
                        (a.search != 0 or a.prewarp_search != 0, "--search / --prewarp-search (they score weight sets and write no id maps)"),
                        (a.live_weights is not None or a.weights is not None, "--live-weights / --weights (the ensemble brings its own sets)"),
                        (bool(suffix), "--combine / --oracle (the members run the argmax merge on the weighted scores)"),
                        (a.viz, "--viz (the members draw no score sheets)"),
                        (a.max_reid_distance, "--max-reid-distance (it runs no merge)"),
                        (a.lockstep > 1, "--lockstep above 1 (the seats hold the weight sets of one video)"),
                        (a.late_annotations and not a.prewarp, "--late-annotations without --prewarp (it belongs to the pre-warp merge)")):
            if on:
                ap.error(f"argument {flag}: not with {why}")
        if a.top is not None and not MIN_ENSEMBLE <= a.top <= MAX_SEATS:
            ap.error(f"argument --top: invalid choice: {a.top} ({MIN_ENSEMBLE} to {MAX_SEATS} weight sets)")
        if a.ensemble is not None:
            try:
                a.ensemble_sets = parse_ensemble_sets(a.ensemble)
            except ValueError as e:
                ap.error(f"argument --ensemble: invalid value: {e}")
    if a.max_reid_distance and (suffix or prewarp or a.lockstep > 1 or a.eval or a.overlay or a.viz or a.weights is not None or a.late_annotations
                                or a.search != 0 or a.live_weights is not None):
        ap.error("argument --max-reid-distance: not with a merge flag (--combine / --oracle / --prewarp / --prewarp-search / --lockstep / --eval / "
                 "--overlay / --viz / --weights / --late-annotations / --search / --live-weights): it runs no merge")
    if a.search < 0:
        ap.error(f"argument --search: invalid choice: {a.search} (a number of weight sets, 1 or more)")
    if a.search > 0:
        for on, why in ((prewarp, "--prewarp / --prewarp-search (it searches the live-warp loop; --prewarp-search is the pre-warp merge's)"),
                        (a.lockstep > 1, "--lockstep above 1 (the seats hold the weight sets of one video)"),
                        (bool(suffix), "--combine / --oracle (the seats run the argmax merge on the weighted scores)"),
                        (a.viz, "--viz (the search draws no score sheets)"),
                        (a.eval or a.overlay, "--eval / --overlay (the search writes no id maps)"),
                        (a.weights is not None or a.late_annotations, "--weights / --late-annotations (they belong to --prewarp)"),
                        (a.live_weights is not None, "--live-weights (set 0 is the default weights, the others are drawn from --seed)")):
            if on:
                ap.error(f"argument --search: not with {why}")
    if a.live_weights is not None:
        if prewarp:
            ap.error("argument --live-weights: not with --prewarp / --prewarp-search (--weights is the pre-warp merge's flag)")
        if suffix:
            ap.error("argument --live-weights: not with --combine / --oracle (the weights are the argmax loop's: what --search scores)")
    if suffix and a.lockstep > 1:
        ap.error("argument --combine / --oracle: not with --lockstep above 1 (the lockstep seats run the argmax merge only)")
    if suffix and prewarp:
        ap.error("argument --combine / --oracle: not with --prewarp / --prewarp-search (they are swaps inside the live-warp loop)")
    if prewarp and a.lockstep > 1:
        ap.error("argument --lockstep: not with --prewarp (the pre-warp merge takes one video at a time: it has no per-frame step to share)")
    if a.prewarp_search > 0 and (a.eval or a.overlay):
        ap.error("argument --prewarp-search: not with --eval / --overlay (the search writes no id maps)")
    if a.prewarp_search < 0:
        ap.error(f"argument --prewarp-search: invalid choice: {a.prewarp_search} (a number of weight sets, 1 or more)")
    if (a.weights is not None or a.late_annotations) and not prewarp:
        ap.error("argument --weights / --late-annotations: only with --prewarp or --prewarp-search")
    if hasattr(a, "negatives"):
        if not prewarp:
            ap.error("argument --negatives: only with --prewarp or --prewarp-search")
        if a.negatives != "all":
            if not a.negatives.isdigit():
                ap.error(f"argument --negatives: invalid choice: {a.negatives!r} (a number of templates, 0 or more; without a number: all)")
            a.negatives = int(a.negatives)
    if a.viz and a.lockstep > 1:
        ap.error("argument --viz: not with --lockstep above 1 (the lockstep seats draw no score sheets)")
    if a.viz and prewarp:
        ap.error("argument --viz: not with --prewarp / --prewarp-search (the sheets show the scores of the live-warp loop)")
    a.merge_weights = _five_weights(ap, "--weights", a.weights) if a.weights is not None else None
    a.live = None
    if a.live_weights is not None:
        live = np.array(_five_weights(ap, "--live-weights", a.live_weights), np.float64)
        a.live = live / live.sum()
    a.parser = ap
    return a


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    ap, weights, tta = a.parser, a.merge_weights, refine_tta(a)
    prewarp = a.prewarp or a.prewarp_search > 0
    if a.ensemble_from is not None:                               # (the first file this mode looks at)
        try:
            with open(a.ensemble_from) as f:
                a.ensemble_sets = select_ensemble(json.load(f), DEFAULT_TOP if a.top is None else a.top)
        except (OSError, ValueError) as e:
            ap.error(f"argument --ensemble-from: {a.ensemble_from}: {e}")
    ensemble = a.ensemble_sets is not None
    suffix = mode_suffix(a.combine, a.oracle, a.live is not None, ensemble, tta is not None)
    root = os.path.abspath(a.root)
    problems = check_inputs(root)
    if prewarp:                                                   # no refinement net in this merge
        problems = [p for p in problems if "refinement_net" not in p]
    lay = mode_layout(root, a.combine, a.oracle, a.live is not None, ensemble, tta is not None)
    if a.max_reid_distance:                                       # neither the refinement net nor the flow
        problems = [p for p in problems if "refinement_net" not in p and not p.startswith(lay["flows"])]
    if (a.oracle or a.viz or a.search) and os.path.isdir(lay["props"]) and os.path.isdir(lay["images"]):
        flag = "--oracle" if a.oracle else "--viz" if a.viz else "--search"
        for v in tree_videos(lay, a.videos):
            lacking = missing_annotations(sorted(glob.glob(os.path.join(lay["images"], v) + "/*")), lay["images"], lay["anns"])
            problems += [f"{fn} is missing ({flag} scores every frame of {v} against its annotation)" for fn in lacking]
    if problems:
        print("premvos_amd.track: inputs are not ready:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print("premvos_amd.track: inputs are in place")
        return 0
    if prewarp:
        return _main_prewarp(ap, a, root, weights)
    if a.max_reid_distance:
        return _main_max_reid_distance(a, root)
    _lib.require_gpu()
    from . import io_pipeline as iop
    from .refinement.driver import refinement_net_init
    from .reid.driver import ReID_net_init
    videos = tree_videos(lay, a.videos)
    with _in_code_dir(root):
        refinement_net, ReID_net = (refinement_net_init() if tta is None else refinement_net_init(tta=tta)), ReID_net_init()
    if tta is not None:
        print(f"premvos_amd.track: the refinement net runs with test-time augmentation {tta}: members {tta.describe()}")
    if a.search:
        search_json = "live_search_tta.json" if tta is not None else "live_search.json"
        r = search_tree(root, videos, a.search, a.seed, refinement_net, ReID_net, **({} if tta is None else {"json_name": search_json}))
        print(f"premvos_amd.track: videos: {len(r['videos'])}  skipped: {len(r['skipped'])}  frames: {r['frames']}  weight sets: {a.search}  "
              f"best: set {r['best']}" + (f" (mean {r['mean'][r['best']]:.6f}; the default weights: {r['mean'][0]:.6f})" if r["best"] is not None else "")
              + f"  ->  {os.path.join(root, 'output', search_json)}")
        return 0
    frames = 0
    eval_dir = lay["eval"] if a.eval else None
    remove_stale(eval_dir, videos)
    if ensemble:
        with iop.Writer() as writer:
            r = ensemble_tree(root, videos, a.ensemble_sets, refinement_net, ReID_net, lay=lay, writer=writer, eval_dir=eval_dir,
                              overlay_dir=lay["overlay"] if a.overlay else None,
                              source=f"--ensemble-from {a.ensemble_from}" if a.ensemble_from is not None else "--ensemble",
                              **({} if tta is None else {"json_name": "ensemble_tta.json"}))
        print(f"premvos_amd.track: videos: {len(videos)}  frames: {r['frames']}  weight sets: {r['sets']}  ->  {lay['out']}"
              + (f"  {lay['overlay']}" if a.overlay else "")
              + f"  {os.path.join(root, 'output', 'ensemble_tta.json' if tta is not None else 'ensemble.json')}")
        if eval_dir is not None:
            summarise(eval_dir, videos, lay["summary"], f"premvos_amd.track: {suffix}:")
        return 0
    with iop.Writer() as writer:
        if a.lockstep > 1:
            logs = do_videos_lockstep(videos, lay, a.lockstep, refinement_net, ReID_net, writer, eval_dir=eval_dir,
                                      overlay_dir=lay["overlay"] if a.overlay else None, weights=a.live)
            frames = sum(len(x) for x in logs.values())
        else:
            for v in videos:
                frames += len(do_video(os.path.join(lay["images"], v) + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"],
                                       refinement_net, ReID_net, writer=writer, eval_dir=eval_dir,
                                       overlay_dir=lay["overlay"] if a.overlay else None, combine=a.combine, oracle=a.oracle,
                                       viz_dir=lay["viz"] if a.viz else None,
                                       **({} if a.live is None else {"tracker": Tracker(refinement_net, ReID_net, weights=a.live, viz=a.viz)})))
    print(f"premvos_amd.track: videos: {len(videos)}  frames: {frames}  ->  {lay['out']}" + (f"  {lay['overlay']}" if a.overlay else "")
          + (f"  {lay['viz']}" if a.viz else ""))
    if eval_dir is not None:
        summarise(eval_dir, videos, lay["summary"], f"premvos_amd.track: {suffix}:" if suffix else "premvos_amd.track:")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
