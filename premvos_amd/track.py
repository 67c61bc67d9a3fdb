"""The merge stage: MergeTrack/merge.py ``do_video`` and the functions of MergeTrack/merge_functions.py it calls, with the pixel and
score work in libpremvos_hip.so (csrc/track_ops.hip + the mask helpers of ``mergetrack``).  The reference's MergeTrack keeps working
unchanged on the trees this package writes; with this module the package can also finish the job alone:

    python -m premvos_amd.track --root <PReMVOS root> [--videos a,b] [--check-only]      ->  output/final/<video>/<frame>.png
                                [--overlay]                                                ->  output/overlay/<video>/<frame>.jpg

Two forms of the same loop:

  * the reference's functions under their names and call shapes, on lists of proposal dicts -- ``read_ann``, ``read_props``,
    ``calculate_scores``, ``calculate_selected_props``, ``remove_mask_overlap``, ``update_templates``, ``save_pngs`` (and
    ``mergetrack.warp_proposals``); ``do_video(..., resident=False)`` is merge.py:69-115 written with them;
  * ``Tracker`` (``do_video``'s default): masks, embeddings and scores of the templates and of the warped candidates stay in HBM from
    frame to frame.  Per frame: decode the fresh proposals (premvos_rle_decode_u8), overlap counts (premvos_mask_overlap_u8), scores
    + selection (premvos_track_scores_f64), overlap removal + id map (premvos_track_paint_u8; the selection never visits the host),
    the id map to the PNG writer thread, warp (premvos_mask_warp_u8), run boundaries + boxes, refinement and ReID of the warped boxes.

The reference's oddities are kept: after refinement a candidate's 'segmentation' is the refined mask while its 'mask' and 'bbox' stay
the warped ones; templates keep the first-frame ReID and id; 'object_score' is the maximum over the template's whole row;
annotations are read only for a ``00000.jpg``; a video without templates gets all-zero PNGs; an unreadable proposal file is an
empty list.  One rule is this package's own: among selections with EQUAL final scores the higher index is painted last (the
reference leaves that to numpy's unstable argsort; in practice such objects both selected the empty proposal).

No CPU fallback for the device work (``_lib.require_gpu()``).  Host-side by design: JSON / PNG files, RLE strings <-> run
boundaries, and ``calculate_selected_props`` of the dict form, whose inputs are host arrays of T x (P + 1) numbers.
"""
from __future__ import annotations

import glob
import json
import os
from copy import deepcopy as copy
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, mergetrack, rle

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


class IdMapSlot:
    """One id map on its way to the host: a page-locked buffer and the event recorded behind its copy."""

    def __init__(self, buf: torch.Tensor, event, ring):
        self.buf, self.event, self._ring = buf, event, ring

    def wait(self) -> np.ndarray:
        self.event.synchronize()
        return self.buf.numpy()

    def release(self) -> None:
        self._ring.put(self)


class Tracker:
    """The resident form of one video's loop.  ``do_refinement(proposals, image_fn, refinement_net)`` and ``add_ReID(proposals,
    image_fn, ReID_net)`` have the reference's call shapes (MergeTrack/refinement_net_functions.py:38, ReID_net_functions.py:26) and
    default to this package's; with this package's engines the warped boxes go through the nets without their masks leaving HBM,
    any other pair (a test's stubs) is called on proposal dicts and its 'segmentation' / 'ReID' results are uploaded."""

    def __init__(self, refinement_net, ReID_net, do_refinement: Optional[Callable] = None, add_ReID: Optional[Callable] = None,
                 weights=None, score_thresh: float = SCORE_THRESH, device=None, record: bool = False):
        _lib.require_gpu()
        from .refinement.driver import RefinementEngine
        from .reid.driver import ReIDEngine
        self.refinement_net, self.ReID_net = refinement_net, ReID_net
        self._direct = (do_refinement is None and add_ReID is None and isinstance(refinement_net, RefinementEngine)
                        and isinstance(ReID_net, ReIDEngine))
        self.do_refinement, self.add_ReID = _default_engine_calls(do_refinement, add_ReID)
        self.weights = np.ascontiguousarray(NORMALISED_WEIGHTS if weights is None else weights, dtype=np.float64)
        self.score_thresh = score_thresh
        self.device = _lib.resolve_device(device)
        self.record = record
        self.engine_log: List[Dict] = []          # record=True: what the engines returned, call by call (replayed by tests)
        self.timer: Optional[Callable[[str], None]] = None     # tools/time_track_loop.py: called with a phase name when the phase ends
        self.T = 0
        self.ids: List = []
        self.ids_dev = self.templ_emb = self.cand_masks = self.cand_emb = self.cand_score = None
        self.ring_slots = 16                      # step_resident: page-locked id-map buffers in flight to the PNG writer
        self._ring = self._fos = None
        self.ring_alive: Optional[Callable[[], bool]] = None     # step_resident: is whoever releases the id-map buffers still at work?
        self.evaluator = None                     # --eval: a premvos_amd.evaluate.LoopEval, handed every id map right after the paint
        self.on_idmap: Optional[Callable] = None  # step_resident: called with the id map (CUDA tensor) right after the paint (--overlay)

    def _tick(self, phase: str) -> None:
        if self.timer is not None:
            self.timer(phase)

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

    # -- one frame -------------------------------------------------------------------------------------------------------------
    def step(self, fresh: List[Dict], flow=None, next_image_fn: Optional[str] = None) -> Dict[str, object]:
        """The frame's fresh proposals (``read_props``) against the templates: -> {"idmap": uint8 [h,w] CUDA tensor (what the PNG
        holds)} and, with ``record``, host copies of "selected", "weighted", "planes", "final_score", "object_score".  ``flow``
        ([h,w,2] array / CUDA tensor / .flo name, None on the last frame) carries the selection to ``next_image_fn``."""
        assert self.T > 0, "no templates: call add_templates first"
        dev, T = self.device, self.T
        _, h, w = self.cand_masks.shape
        F = len(fresh)
        P = T + F
        masks = torch.empty((P, h, w), dtype=torch.uint8, device=dev)
        masks[:T].copy_(self.cand_masks)
        pscore, emb_p = self.cand_score, self.cand_emb
        if F:
            decode_segmentations([p["segmentation"] for p in fresh], out=masks[T:])
            pscore = torch.cat([pscore, _f64([float(p["score"]) for p in fresh], dev)])
            emb_p = torch.cat([emb_p, _f64(np.array([np.asarray(p["ReID"], np.float64) for p in fresh]), dev)])
        self._tick("decode")
        # templates' masks and scores ARE the warped candidates' (update_templates copies them): the first T rows
        inter, area_p, area_t = mergetrack.mask_overlap(masks, masks[:T])
        self._tick("overlap")
        s = track_scores(inter, area_p, area_t, self.cand_score, pscore, emb_p, self.templ_emb, self.weights, self.score_thresh)
        self._tick("scores")
        labels, idmap, refined = track_paint(masks, s["selected"], s["final_score"], self.ids_dev)
        if self.evaluator is not None:
            self.evaluator.frame(idmap)
        self._tick("paint")
        out: Dict[str, object] = {"idmap": idmap}
        if self.record:
            out.update({k: s[k].cpu().numpy() for k in ("selected", "weighted", "planes", "final_score", "object_score")})
            out["labels"] = labels.cpu().numpy()
        if flow is not None:
            self._advance(refined, s["final_score"], flow, next_image_fn)
        return out

    # -- one frame, everything resident ---------------------------------------------------------------------------------------------
    def _idmap_slot(self, h: int, w: int) -> "IdMapSlot":
        """A page-locked [h,w] buffer + event from the ring (made on first use, reused once its reader released it)."""
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
                    return IdMapSlot(torch.empty((h, w), dtype=torch.uint8).pin_memory(), torch.cuda.Event(), self._ring)
            if tuple(slot.buf.shape) == (h, w):
                return slot
            self._ring_made -= 1                                              # another frame size: dropped, a new one is made

    def pin_idmap_ring(self, h: int, w: int) -> None:
        """Make the ring's page-locked buffers now (a page-locked allocation blocks the host): call it once per video, before the
        first ``step_resident``; without it the buffers are made as the first ``ring_slots`` frames need them."""
        slots = []
        while (self._ring_made if self._ring is not None else 0) < self.ring_slots:
            slots.append(self._idmap_slot(h, w))
        for s in slots:
            s.release()

    def step_resident(self, fresh_masks: Optional[torch.Tensor], reid_rows: Optional[torch.Tensor], scores: Optional[torch.Tensor],
                      flow: Optional[torch.Tensor] = None, next_frame: Optional[torch.Tensor] = None,
                      stack: Optional[torch.Tensor] = None, next_slots: Optional[torch.Tensor] = None) -> Dict[str, object]:
        """``step`` for a caller whose arrays are in HBM already (premvos_amd.stream --track): ``fresh_masks`` uint8 [F,h,w],
        ``reid_rows`` float32 [F,132] (``ReIDNet.embed_masks``: 128 embedding values + the mask's box as int32 bits; a box with
        w <= 0 or h <= 0 = no embedding), ``scores`` float64 [F], ``flow`` float32 [h,w,2] and ``next_frame`` uint8 [h,w,3] (both None
        on a video's last frame), all CUDA; F = 0: the three may be None.  Everything is queued on the current stream: no host
        synchronisation, no RLE, nothing copied to the host but the id map -- into a page-locked ring buffer, with an event.
        -> {"idmap": ``IdMapSlot`` (``wait()`` -> the [h,w] array once the event has passed; ``release()`` when done), "selected",
        "weighted", "planes", "final_score", "object_score", "labels": CUDA tensors}.
        ``stack``: uint8 [T + F,h,w] whose last F entries ARE ``fresh_masks`` and whose first T are free for the candidates (the feed
        lays its store out like this: no gather); ``next_slots``: uint8 [T,h,w], where the refined candidates of the next frame go (the
        first T entries of the next call's ``stack``).  Both optional: without them the tracker uses stores of its own."""
        assert self.T > 0, "no templates: call add_templates first"
        if not self._direct:
            raise _lib.PremvosError("step_resident needs this package's engines (RefinementEngine, ReIDEngine)")
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
        inter, area_p, area_t = mergetrack.mask_overlap(stack, stack[:T])
        self._tick("overlap")
        s = track_scores(inter, area_p, area_t, self.cand_score, pscore, emb_p, self.templ_emb, self.weights, self.score_thresh)
        self._tick("scores")
        labels, idmap, refined = track_paint(stack, s["selected"], s["final_score"], self.ids_dev)
        slot = self._idmap_slot(h, w)
        slot.buf.copy_(idmap, non_blocking=True)
        slot.event.record(torch.cuda.current_stream(dev))
        if self.evaluator is not None:                                        # (behind the id map's event: the PNG does not wait for it)
            self.evaluator.frame(idmap)
        if self.on_idmap is not None:
            self.on_idmap(idmap)
        self._tick("paint")
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
        cand_score = torch.empty((T,), dtype=torch.float64, device=dev)
        yx = torch.empty((T, 4), dtype=torch.float32, device=dev)
        assert bbox.is_contiguous() and bbox.dtype == torch.int32
        _lib.check(lib.premvos_track_next_f32(s["final_score"].data_ptr(), bbox.data_ptr(), T, cand_score.data_ptr(), yx.data_ptr(),
                                              _lib.current_stream()), "track_next")
        self._tick("boxes+reid")
        p = self.refinement_net.net.refine(next_frame, yx, max_boxes=_bucket(T))
        dest = next_slots if next_slots is not None else torch.empty((T, h, w), dtype=torch.uint8, device=dev)
        assert tuple(dest.shape) == (T, h, w) and dest.is_contiguous()
        dest.copy_(p.mask[:T])
        self.cand_masks, self.cand_emb, self.cand_score = dest, cand_emb, cand_score
        self._tick("refine")
        return out

    def _advance(self, refined: torch.Tensor, final_score: torch.Tensor, flow, next_image_fn) -> None:
        """merge.py:98-102: warp_proposals, do_refinement, add_ReID, update_templates.  With this package's engines ``next_image_fn``
        may also be the decoded frame (uint8 [h,w,3] array or CUDA tensor)."""
        flow = mergetrack.get_flow(flow) if isinstance(flow, str) else flow
        warped = mergetrack.warp_masks(refined, flow)
        segs = mergetrack.encode_masks(warped)                                        # run boundaries on the GPU; strings + boxes on the host
        boxes = [rle.to_bbox(sg) for sg in segs]
        self.cand_score = 0.5 * (final_score + 1)                                     # 'score' of a warped proposal (merge_functions.py:234)
        self._tick("warp+rle+bbox")
        if self._direct and self.T <= self.refinement_net.max_boxes:
            from PIL import Image
            from . import jpeg
            from .refinement.driver import _bucket
            image = np.asarray(Image.open(next_image_fn).convert("RGB")) if isinstance(next_image_fn, str) else next_image_fn
            frame = jpeg.to_device(image, self.refinement_net.net.device)
            yx = np.array([[b[1], b[0], b[1] + b[3], b[0] + b[2]] for b in boxes], np.float32)
            p = self.refinement_net.net.refine(frame, torch.from_numpy(yx).to(self.refinement_net.net.device), max_boxes=_bucket(self.T))
            self.cand_masks = p.mask[:self.T].to(self.device).clone()
            self._tick("refine")
            emb = self.ReID_net.embed(image, boxes, feed=True)
            self.cand_emb = _f64(emb.astype(np.float64), self.device)
            self._tick("reid")
            if self.record:
                self.engine_log.append({"call": "refine", "image_fn": next_image_fn, "bbox": np.array(boxes), "mask": self.cand_masks.cpu().numpy()})
                self.engine_log.append({"call": "reid", "image_fn": next_image_fn, "ReID": emb.astype(np.float64)})
            return
        fs = final_score.cpu().numpy()
        props = [{"segmentation": segs[i], "bbox": boxes[i], "score": 0.5 * (fs[i] + 1), "final_score": fs[i], "mask": warped[i],
                  "id": self.ids[i]} for i in range(self.T)]
        props = self.do_refinement(props, next_image_fn, self.refinement_net)
        props = self.add_ReID(props, next_image_fn, self.ReID_net)
        self.cand_masks = decode_segmentations([p["segmentation"] for p in props], device=self.device)
        self.cand_emb = _f64(np.array([np.asarray(p["ReID"], np.float64) for p in props]), self.device)
        if self.record:
            self.engine_log.append({"call": "refine", "image_fn": next_image_fn, "bbox": np.array(boxes), "mask": self.cand_masks.cpu().numpy()})
            self.engine_log.append({"call": "reid", "image_fn": next_image_fn, "ReID": self.cand_emb.cpu().numpy()})


def _frame_paths(image_fn: str, images: str, anns: str, props: str, flows: str, out: str):
    rel = os.path.relpath(image_fn, images)
    stem = os.path.splitext(rel)[0]
    return (os.path.join(anns, stem + ".png"), os.path.join(props, stem + ".json"), os.path.join(flows, stem + ".flo"),
            os.path.join(out, stem + ".png"))


def do_video(video_dir: str, images: str, anns: str, props: str, flows: str, out: str, refinement_net, ReID_net,
             do_refinement: Optional[Callable] = None, add_ReID: Optional[Callable] = None, resident: bool = True, writer=None,
             record: bool = False, tracker: Optional[Tracker] = None, eval_dir: Optional[str] = None,
             overlay_dir: Optional[str] = None) -> List[Dict]:
    """merge.py:69-115 for the frames ``video_dir``*.jpg: one PNG per frame under ``out``.  ``images`` / ``anns`` / ``props`` /
    ``flows`` / ``out`` are the five roots the reference keeps in module globals.  PNGs are written on ``writer`` (an
    ``io_pipeline.Writer``; None: one of its own, closed before returning).  -> one dict per frame ("image_fn", "png_fn" and, with
    ``record``, host copies of the selection, the scores and the id map).  ``eval_dir``: also score the id maps against the video's
    annotations while they are in HBM (premvos_amd.evaluate.LoopEval) and write ``eval_dir``/<video>.json; the PNGs are the same.
    ``overlay_dir``: also one JPEG per frame under it, the frame with the id map's objects tinted (premvos_amd.overlay: blended and
    DCT-coded on the GPU from the id map in HBM, Huffman-coded on ``writer``); the PNGs are the same."""
    from . import io_pipeline as iop
    if eval_dir is not None and not resident:
        raise _lib.PremvosError("eval_dir needs the resident tracker (the id maps are scored in device memory)")
    own = writer is None
    writer = iop.Writer() if own else writer
    log: List[Dict] = []
    try:
        image_fn_list = sorted(glob.glob(video_dir + "*"))
        if resident:
            tr = tracker or Tracker(refinement_net, ReID_net, do_refinement, add_ReID, record=record)
        else:
            _lib.require_gpu()
            do_ref, add_reid = _default_engine_calls(do_refinement, add_ReID)
            templates: List[Dict] = []
            next_props: List[Dict] = []
        for image_id, image_fn in enumerate(image_fn_list):
            ann_fn, prop_fn, flow_fn, png_fn = _frame_paths(image_fn, images, anns, props, flows, out)
            rec: Dict[str, object] = {"image_fn": image_fn, "png_fn": png_fn}
            idmap_dev = None
            has_flow = os.path.exists(flow_fn) and image_id + 1 < len(image_fn_list)
            new_templates = read_ann(ann_fn) if os.path.exists(ann_fn) and "00000.jpg" in image_fn else []
            if resident:
                tr.add_templates(new_templates, image_fn)
                if eval_dir is not None and image_id == 0:
                    from .evaluate import LoopEval
                    video = os.path.relpath(video_dir, images).strip("/")
                    tr.evaluator = LoopEval.open(video, os.path.join(anns, video), tr.device) if tr.T else None
                    if not tr.T:
                        print(f"premvos_amd.track: {video}: no templates, not evaluated")
                if tr.T:
                    if tr.evaluator is not None:
                        tr.evaluator.expect(os.path.splitext(os.path.basename(image_fn))[0])
                    r = tr.step(read_props(prop_fn), flow_fn if has_flow else None, image_fn_list[image_id + 1] if has_flow else None)
                    idmap_dev = r.pop("idmap")
                    idmap = idmap_dev.cpu().numpy()
                    rec.update(r)
                else:
                    idmap = np.zeros(_image_size(image_fn), np.uint8)
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
                else:
                    idmap = np.zeros(_image_size(image_fn), np.uint8)
            if record:
                rec["png"] = idmap
            writer.submit(write_png, png_fn, idmap)
            if overlay_dir is not None:
                from . import jpeg, overlay
                dev = tr.device if resident else _lib.resolve_device(None)
                if idmap_dev is None and idmap.any():
                    idmap_dev = torch.from_numpy(np.ascontiguousarray(idmap, dtype=np.uint8)).to(dev)
                jpg_fn = os.path.join(overlay_dir, os.path.splitext(os.path.relpath(image_fn, images))[0] + ".jpg")
                writer.submit(overlay.write_jpg, jpg_fn, overlay.forward(jpeg.imread(image_fn, dev), idmap_dev))
            log.append(rec)
        if resident and eval_dir is not None and tr.evaluator is not None:
            writer.submit(tr.evaluator.fetch().dump, eval_dir)               # the writer waits for the counts, once per video
            tr.evaluator = None
    finally:
        if own:
            writer.close()
    return log


# ---------------------------------------------------------------------------------------------------------------- command line
def _layout(root: str) -> Dict[str, str]:
    return {"images": os.path.join(root, "data/DAVIS/JPEGImages/480p") + "/", "anns": os.path.join(root, "data/DAVIS/Annotations/480p") + "/",
            "props": os.path.join(root, "output/intermediate/ReID_proposals") + "/", "flows": os.path.join(root, "output/intermediate/flow") + "/",
            "out": os.path.join(root, "output/final") + "/", "overlay": os.path.join(root, "output/overlay") + "/"}


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


def main(argv: Optional[List[str]] = None) -> int:
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
    a = ap.parse_args(argv)
    root = os.path.abspath(a.root)
    problems = check_inputs(root)
    if problems:
        print("premvos_amd.track: inputs are not ready:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print("premvos_amd.track: inputs are in place")
        return 0
    _lib.require_gpu()
    from . import io_pipeline as iop
    from .refinement.driver import refinement_net_init
    from .reid.driver import ReID_net_init
    lay = _layout(root)
    videos = sorted(d for d in os.listdir(lay["props"]) if os.path.isdir(os.path.join(lay["props"], d)))
    if a.videos:
        videos = [v for v in videos if v in a.videos.split(",")]
    cwd = os.getcwd()
    os.chdir(os.path.join(root, "code"))                      # the configs' 'load' paths are relative to code/ (the reference runs there)
    try:
        refinement_net, ReID_net = refinement_net_init(), ReID_net_init()
    finally:
        os.chdir(cwd)
    frames = 0
    eval_dir = os.path.join(root, "output", "eval") if a.eval else None
    with iop.Writer() as writer:
        for v in videos:
            if eval_dir is not None and os.path.isfile(os.path.join(eval_dir, v + ".json")):
                os.remove(os.path.join(eval_dir, v + ".json"))                 # (an earlier run's: the summary is of THIS run's videos)
            frames += len(do_video(os.path.join(lay["images"], v) + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"],
                                   refinement_net, ReID_net, writer=writer, eval_dir=eval_dir,
                                   overlay_dir=lay["overlay"] if a.overlay else None))
    print(f"premvos_amd.track: videos: {len(videos)}  frames: {frames}  ->  {lay['out']}" + (f"  {lay['overlay']}" if a.overlay else ""))
    if eval_dir is not None:
        from . import evaluate as ev
        scored = [v for v in videos if os.path.isfile(os.path.join(eval_dir, v + ".json"))]
        r = ev.summarise(eval_dir, scored) if scored else None
        if r is not None:
            print(f"premvos_amd.track: J {r['mean_J']}  F {r['mean_F']}  J&F {r['mean_JF_percent']}  ->  {ev.write_summary(root, r)}")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
