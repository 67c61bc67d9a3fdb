"""The paper's pre-warp merge (MergeTrack/oldmerge.py, "PREMVOS 1 uses pre-warp") of a whole video in a handful of launches, and
the random search that produced its weights (oldmerge.py:225-227,253-255 with merge_functions.py:613-634 eval_video) as W small
workgroups.  Every proposal carries its mask warped to the next frame (made here: premvos_rle_decode_u8, premvos_mask_warp_seats_u8,
premvos_mask_pack_bits_u8; only the bits are kept), so no network runs in the loop, objects may be annotated in any frame
(``late``), and between "the video's proposals are uploaded" and "the id maps are there" nothing returns to the host.
tests/prewarp_restated.py states the semantics in numpy; DESIGN.md 8.5 has the rules of our own and what is left out.

    python -m premvos_amd.track --prewarp [--weights a,b,c,d,e] [--late-annotations]      ->  output/final_prewarp/<video>/<frame>.png
    python -m premvos_amd.track --prewarp-search W [--seed S]                              ->  output/prewarp_search.json
    python -m premvos_amd.track --prewarp --ensemble "a,b,c,d,e;..." | --ensemble-from F   ->  output/final_prewarp_ensemble/<video>/<frame>.png
                                                                                               (``ensemble_video``: K sets, one chain launch, their vote)
    python -m premvos_amd.stream --track --prewarp [--weights a,b,c,d,e]                   ->  the same PNGs from JPEGs, in one process
                                                                                               (``VideoIngest``: the pool from arrays in HBM)
    ... --negatives [K] with any of them (oldmerge.py's use_ff_negative_props)             ->  ``_neg`` behind ``prewarp`` in every name:
                                                                                               output/final_prewarp_neg/, prewarp_neg_search.json, ...

The quality of this merge on DAVIS is NOT measured here (no weights, no dataset): it is the reference's older merge, not an
equal of the live-warp loop."""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, mergetrack, track

EMB = 128
WEIGHTS = np.array([0.1639026729185494, 0.3090363324359478, 0.11728252456485666, 0.18345061062541546, 0.2263278594552307])   # oldmerge.py:220-221
MAX_T, MAX_P, MAX_TP = 64, 256, 8000                                                # prewarp_ops.hip's caps (it refuses beyond them)
MAX_WARP_FLOWS = 8                                                                  # premvos_mask_warp_seats_u8's seats (merge_ops.hip)
CHUNK_BYTES = 256 << 20                                                             # byte masks alive at once while the bits are made


def normalised(weights=None) -> np.ndarray:
    w = np.asarray(WEIGHTS if weights is None else weights, np.float64).reshape(5)
    return w / np.sum(w)


def search_weights(W: int, seed: int = 0) -> np.ndarray:
    """set 0 = the default weights, sets 1 .. W-1 = ``default_rng(seed).random(5)``, all normalised -> float64 [W,5]"""
    rng = np.random.default_rng(seed)
    return np.array([normalised()] + [normalised(rng.random(5)) for _ in range(W - 1)])


# ------------------------------------------------------------------------------------------------------------ host helpers (no GPU)
def row_bytes(hw: int) -> int:
    """bytes of one mask's row in the pool: h*w bits rounded up to whole 64-bit words"""
    return (hw + 63) // 64 * 8


def pack_bits_host(masks: np.ndarray) -> np.ndarray:
    """uint8 [n,h,w] (non-zero = set) -> uint8 [n, row_bytes(h*w)] in premvos_mask_pack_bits_u8's layout (bit k of byte i = pixel
    8 i + k), zero beyond h*w: the host twin of ``pack_rows`` (tests, and the layout's definition)."""
    m = np.asarray(masks)
    n, hw = m.shape[0], int(np.prod(m.shape[1:]))
    out = np.zeros((n, row_bytes(hw)), np.uint8)
    b = np.packbits(m.reshape(n, hw) != 0, axis=1, bitorder="little")
    out[:, :b.shape[1]] = b
    return out


def unpack_bits_host(bits: np.ndarray, h: int, w: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bits, np.uint8), axis=1, bitorder="little")[:, :h * w].reshape(-1, h, w)


class Tables:
    """The host tables of a video (prewarp_ops.hip's block table, poff, first) from P_t and the number of objects annotated per frame.
    Pool slots: [current masks of the sumP proposals | their forward masks | the T annotation masks | their forward masks].
    ``n_neg`` > 0 (``--negatives``, oldmerge.py:137-138,147): that many templates more, behind the ``T_ann`` annotated ones and annotated
    in no frame (``first`` still ends at ``T_ann``); their own masks are ``n_neg`` slots behind the annotations' forward masks and
    block 0's ``c0, nc`` range.  With ``n_neg`` = 0 every array is what it always was."""

    def __init__(self, P: Sequence[int], A: Sequence[int], n_neg: int = 0):
        assert len(P) == len(A) and len(P) >= 1 and 0 <= n_neg <= int(P[0])
        self.N = len(P)
        self.poff = np.concatenate(([0], np.cumsum(np.asarray(P, np.int64)))).astype(np.int32)
        self.first = np.concatenate(([0], np.cumsum(np.asarray(A, np.int64)))).astype(np.int32)
        self.sumP, self.T_ann, self.n_neg = int(self.poff[-1]), int(self.first[-1]), int(n_neg)
        self.T = self.T_ann + self.n_neg
        self.S = 2 * self.sumP + 2 * self.T_ann + self.n_neg
        self.cur0, self.fwd0, self.ann0, self.annfwd0 = 0, self.sumP, 2 * self.sumP, 2 * self.sumP + self.T_ann
        self.neg0 = 2 * self.sumP + 2 * self.T_ann
        rows, io, ao = [], 0, 0
        for t in range(self.N):
            na = int(P[t])
            if t == 0:
                b0, nb, c0, nc = self.ann0, int(A[0]), (self.neg0 if self.n_neg else 0), self.n_neg
            else:
                b0, nb, c0, nc = self.fwd0 + int(self.poff[t - 1]), int(P[t - 1]), self.annfwd0 + int(self.first[t - 1]), int(A[t - 1])
            rows.append((self.cur0 + int(self.poff[t]), na, b0, nb, c0, nc, io, ao))
            io, ao = io + na * (nb + nc), ao + na + nb + nc
        assert io < 2 ** 31 and ao < 2 ** 31, "the video's overlap counts do not fit int32 offsets"
        self.blocks = np.ascontiguousarray(np.array(rows, np.int32).reshape(self.N, 8))
        self.n_inter, self.n_areas = io, ao

    def check_caps(self) -> None:
        P = np.diff(self.poff)
        if self.T > MAX_T or (len(P) and (P.max() > MAX_P or P.max() * self.T > MAX_TP)):
            raise _lib.PremvosError(f"prewarp: {self.T} templates, up to {int(P.max())} proposals per frame: at most {MAX_T} templates, {MAX_P} "
                                    f"proposals and {MAX_TP} scores per frame fit the chain kernel's LDS"
                                    + (f" ({self.n_neg} of the templates are negatives: pass --negatives K)" if self.n_neg else ""))


def _i32(a, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)


# ------------------------------------------------------------------------------------------------------------------ device wrappers
def pack_rows(masks: torch.Tensor, out_rows: torch.Tensor) -> None:
    """uint8 [n,h,w] in HBM -> the n rows ``out_rows`` [n, row_bytes] of a pool (one premvos_mask_pack_bits_u8 launch)."""
    n = masks.shape[0]
    if n == 0:
        return
    hw, rb = masks.shape[1] * masks.shape[2], out_rows.shape[1]
    assert out_rows.is_contiguous() and out_rows.shape[0] == n and rb == row_bytes(hw)
    flat = masks.reshape(n, hw)
    if rb * 8 != hw:
        padded = torch.zeros((n, rb * 8), dtype=torch.uint8, device=masks.device)
        padded[:, :hw] = flat
        flat = padded
    flat = flat.contiguous()
    _lib.check(_lib.load().premvos_mask_pack_bits_u8(flat.data_ptr(), n * rb * 8, out_rows.data_ptr(), _lib.current_stream()), "mask_pack_bits")


def bits_overlap(pool: torch.Tensor, hw: int, blocks: np.ndarray, n_inter: int, n_areas: int, blocks_dev: Optional[torch.Tensor] = None):
    """premvos_bits_overlap_i32 -> (inter int32 [n_inter], areas int32 [n_areas]) in HBM."""
    _lib.require_gpu()
    dev = pool.device
    blocks = np.ascontiguousarray(blocks, np.int32).reshape(-1, 8)
    bd = blocks_dev if blocks_dev is not None else _i32(blocks, dev)
    inter = torch.empty((max(n_inter, 1),), dtype=torch.int32, device=dev)
    areas = torch.empty((max(n_areas, 1),), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().premvos_bits_overlap_i32(pool.data_ptr(), pool.shape[0], pool.shape[1], hw, blocks.ctypes.data, bd.data_ptr(),
                                                    blocks.shape[0], inter.data_ptr(), n_inter, areas.data_ptr(), n_areas,
                                                    _lib.current_stream()), "bits_overlap")
    return inter[:n_inter], areas[:n_areas]


def negatives_cap(negatives) -> Optional[int]:
    """``negatives`` as the public functions take it -> None (off), -1 (all, as oldmerge.py:63-85) or the cap K >= 0"""
    if negatives is None:
        return None
    if isinstance(negatives, str):
        if negatives != "all":
            raise ValueError(f'negatives: None, "all" or a number of templates, 0 or more (got {negatives!r})')
        return -1
    if isinstance(negatives, bool) or int(negatives) != negatives or int(negatives) < 0:
        raise ValueError(f'negatives: None, "all" or a number of templates, 0 or more (got {negatives!r})')
    return int(negatives)


def negatives_room(negatives, P0: int, T_ann: int) -> int:
    """the pool slots and embedding rows to keep free for the negatives of a video: they are at most frame 0's proposals"""
    K = negatives_cap(negatives)
    return 0 if K is None or T_ann == 0 else int(P0) if K < 0 else min(int(P0), K)


class DeviceVideo:
    """A video in HBM: the bit pool, the tables (host and device), scores and embeddings.  ``neg_room``: slots and template rows kept
    free for ``add_negatives``."""

    def __init__(self, tab: Tables, h: int, w: int, ids: Sequence[int], device=None, neg_room: int = 0):
        _lib.require_gpu()
        self.dev = _lib.resolve_device(device)
        self.tab, self.h, self.w, self.hw = tab, int(h), int(w), int(h) * int(w)
        assert all(0 < int(i) <= 255 for i in ids) and len(ids) == tab.T_ann and tab.n_neg == 0, "object ids are palette indices 1 .. 255"
        self.ids = [int(i) for i in ids]
        self.negatives: List[int] = []
        self.pool = torch.zeros((max(tab.S + neg_room, 1), row_bytes(self.hw)), dtype=torch.uint8, device=self.dev)
        self.blocks_dev, self.poff_dev, self.first_dev = _i32(tab.blocks, self.dev), _i32(tab.poff, self.dev), _i32(tab.first, self.dev)
        self.ids_dev = _i32(np.asarray(self.ids, np.int32), self.dev)
        self.score = torch.zeros((max(tab.sumP, 1),), dtype=torch.float64, device=self.dev)
        self.emb_p = torch.zeros((max(tab.sumP, 1), EMB), dtype=torch.float64, device=self.dev)
        self.emb_t = torch.zeros((max(tab.T + neg_room, 1), EMB), dtype=torch.float64, device=self.dev)

    # -- the negative templates (oldmerge.py:63-85,137-138,147) -----------------------------------------------------------------------
    def add_negatives(self, negatives) -> List[int]:
        """Once the pool, the scores and the embeddings are in place and before ``prepare``: premvos_prewarp_negatives_i32 walks frame
        0's proposals, ONE readback (the indices and their count, 4 (P_0 + 1) bytes: the count sizes the tables), then the tables with
        ``n_neg`` templates more and premvos_prewarp_gather_neg_u8 for their mask rows and embeddings.  -> frame-0 proposal indices in
        acceptance order.  A video without annotated objects has no negatives."""
        K, tab, lib = negatives_cap(negatives), self.tab, _lib.load()
        P, A = np.diff(tab.poff), np.diff(tab.first)
        P0, A0 = int(P[0]), int(A[0])
        assert tab.n_neg == 0, "a video's negatives are chosen once"
        if K is None or K == 0 or P0 == 0 or tab.T_ann == 0:
            return self.negatives
        buf = torch.empty((P0 + 1,), dtype=torch.int32, device=self.dev)                         # taken [P0] | count
        conflict = torch.empty((P0 * (A0 + P0),), dtype=torch.uint8, device=self.dev)
        _lib.check(lib.premvos_prewarp_negatives_i32(self.pool.data_ptr(), self.pool.shape[0], self.pool.shape[1], self.hw, tab.cur0, P0, tab.ann0,
                                                     A0, self.score.data_ptr(), K, conflict.data_ptr(), buf.data_ptr(), buf.data_ptr() + 4 * P0,
                                                     _lib.current_stream()), "prewarp_negatives")
        host = buf.cpu().numpy()
        n = int(host[P0])
        self.negatives = [int(i) for i in host[:n]]
        if n == 0:
            return self.negatives
        new = Tables(P, A, n)
        new.check_caps()
        assert new.S <= self.pool.shape[0] and new.T <= self.emb_t.shape[0], "no room was kept for the negatives (neg_room)"
        _lib.check(lib.premvos_prewarp_gather_neg_u8(self.pool.data_ptr(), self.pool.shape[0], self.pool.shape[1], new.cur0, P0, new.neg0, n,
                                                     buf.data_ptr(), self.emb_p.data_ptr(), self.emb_t.data_ptr() + 8 * EMB * new.T_ann,
                                                     _lib.current_stream()), "prewarp_gather_neg")
        self.tab, self.blocks_dev = new, _i32(new.blocks, self.dev)
        return self.negatives

    # -- the weight-independent part ---------------------------------------------------------------------------------------------
    def prepare(self) -> None:
        tab, lib = self.tab, _lib.load()
        self.inter, self.areas = bits_overlap(self.pool, self.hw, tab.blocks, tab.n_inter, tab.n_areas, self.blocks_dev)
        n = max(tab.T * tab.sumP, 1)
        self.flat = torch.empty((n,), dtype=torch.float64, device=self.dev)
        self.maxd = torch.empty((tab.T,), dtype=torch.float64, device=self.dev)
        self.reid, self.oreid = torch.empty_like(self.flat), torch.empty_like(self.flat)
        _lib.check(lib.premvos_prewarp_reid_f64(self.emb_p.data_ptr(), self.emb_t.data_ptr(), tab.sumP, tab.T, tab.poff.ctypes.data,
                                                self.poff_dev.data_ptr(), tab.N, self.flat.data_ptr(), self.maxd.data_ptr(), self.reid.data_ptr(),
                                                self.oreid.data_ptr(), _lib.current_stream()), "prewarp_reid")

    def chain(self, weights: np.ndarray, want_weighted: bool = False) -> Dict[str, torch.Tensor]:
        """``weights`` [W,5] normalised -> chosen int32 [W,N,T], best float64 [W,N,T] (+ the weighted scores for W == 1)."""
        tab = self.tab
        wts = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1, 5))
        W = wts.shape[0]
        wd = torch.from_numpy(wts).to(self.dev)
        chosen = torch.empty((W, tab.N, tab.T), dtype=torch.int32, device=self.dev)
        best = torch.empty((W, tab.N, tab.T), dtype=torch.float64, device=self.dev)
        weighted = torch.empty_like(self.flat) if want_weighted else None
        head = (self.inter.data_ptr(), tab.n_inter, self.areas.data_ptr(), tab.n_areas, tab.blocks.ctypes.data, self.blocks_dev.data_ptr(),
                tab.poff.ctypes.data, self.poff_dev.data_ptr(), tab.first.ctypes.data, self.first_dev.data_ptr(), tab.N, tab.T)
        rest = (self.score.data_ptr(), self.reid.data_ptr(), self.oreid.data_ptr(), wd.data_ptr(), W, chosen.data_ptr(), best.data_ptr(),
                weighted.data_ptr() if weighted is not None else None, _lib.current_stream())
        if tab.n_neg:                                                 # (without negatives: the entry that was always called)
            _lib.check(_lib.load().premvos_prewarp_chain_neg_f64(*head, tab.n_neg, *rest), "prewarp_chain_neg")
        else:
            _lib.check(_lib.load().premvos_prewarp_chain_f64(*head, *rest), "prewarp_chain")
        out = {"chosen": chosen, "best": best}
        if weighted is not None:
            out["weighted"] = weighted
        return out

    def paint(self, chosen: torch.Tensor, best: torch.Tensor, idmap: bool = True, gt_bits: Optional[torch.Tensor] = None, T0: int = 0,
              out: Optional[torch.Tensor] = None):
        """-> (idmap uint8 [N,h,w] or None, counts int32 [W,N,T0,3] or None); ``out``: the id map's place (contiguous [N,h,w] in HBM)"""
        tab = self.tab
        W = chosen.shape[0]
        if out is not None:
            assert idmap and out.is_contiguous() and out.dtype == torch.uint8 and tuple(out.shape) == (tab.N, self.h, self.w), out.shape
        im = (torch.empty((tab.N, self.h, self.w), dtype=torch.uint8, device=self.dev) if out is None else out) if idmap else None
        counts = torch.empty((W, tab.N, T0, 3), dtype=torch.int32, device=self.dev) if gt_bits is not None else None
        if gt_bits is not None:
            assert gt_bits.is_contiguous() and tuple(gt_bits.shape) == (tab.N, T0, self.pool.shape[1]) and gt_bits.dtype == torch.uint8
        head = (self.pool.data_ptr(), self.pool.shape[0], self.pool.shape[1], self.hw, tab.blocks.ctypes.data, self.blocks_dev.data_ptr(),
                tab.first.ctypes.data, self.first_dev.data_ptr(), self.ids_dev.data_ptr(), tab.ann0, chosen.data_ptr(), best.data_ptr(), tab.N, tab.T)
        rest = (W, im.data_ptr() if im is not None else None, gt_bits.data_ptr() if gt_bits is not None else None, T0,
                counts.data_ptr() if counts is not None else None, _lib.current_stream())
        if tab.n_neg:
            _lib.check(_lib.load().premvos_prewarp_paint_neg_bits_u8(*head, tab.n_neg, *rest), "prewarp_paint_neg")
        else:
            _lib.check(_lib.load().premvos_prewarp_paint_bits_u8(*head, *rest), "prewarp_paint")
        return im, counts


def upload(frames: Sequence[Dict], h: int, w: int, device=None, negatives=None) -> DeviceVideo:
    """A video as a list of frames -> ``DeviceVideo`` with its pool filled.  A frame is a dict with
        "score" [P], "emb" [P,128] float64 (an all-inf row: no 'ReID'),
        the current masks: "mask" uint8 [P,h,w] (host or HBM), or "pool" / "offsets" (run boundaries: ``track.parse_fresh``),
        the forward masks: "fwd" uint8 [P,h,w], or "flow" float32 [h,w,2] to warp with (neither: empty forward masks),
        "ann": the objects annotated IN this frame, dicts of "id", "mask" [h,w], "reid" [128] and optionally "fwd" [h,w].
    The byte masks exist only chunk-wise while the bits are made (a decode per frame, a warp per 8 flows, four packs per chunk).
    ``negatives`` (None: off, "all" or a cap): ``DeviceVideo.add_negatives`` once the pool is filled."""
    dev = _lib.resolve_device(device)
    P = [len(f["score"]) for f in frames]
    tab = Tables(P, [len(f["ann"]) for f in frames])
    tab.check_caps()
    dv = DeviceVideo(tab, h, w, [o["id"] for f in frames for o in f["ann"]], dev, negatives_room(negatives, P[0], tab.T))
    hw = h * w
    if tab.sumP:
        dv.score[:tab.sumP] = track._f64(np.concatenate([np.asarray(f["score"], np.float64).reshape(-1) for f in frames]), dev)
        dv.emb_p[:tab.sumP] = track._f64(np.concatenate([np.asarray(f["emb"], np.float64).reshape(-1, EMB) for f in frames]), dev)
    if tab.T:
        dv.emb_t[:tab.T] = track._f64(np.array([np.asarray(o["reid"], np.float64) for f in frames for o in f["ann"]]).reshape(tab.T, EMB), dev)
    t0 = 0
    while t0 < tab.N:
        t1, n = t0, 0
        while t1 < tab.N and (t1 == t0 or (n + P[t1] + len(frames[t1]["ann"])) * hw * 2 <= CHUNK_BYTES):
            n += P[t1] + len(frames[t1]["ann"])
            t1 += 1
        cur_p, cur_a, fwd_given_p, fwd_given_a, flows, flow_of = [], [], [], [], [], []
        for t in range(t0, t1):
            f = frames[t]
            if P[t]:
                if "mask" in f:
                    cur_p.append(mergetrack._dev_masks(f["mask"], dev).reshape(P[t], h, w))
                else:
                    cur_p.append(track.decode_boundaries(f["pool"], f["offsets"], h, w, device=dev))
            for o in f["ann"]:
                cur_a.append(mergetrack._dev_masks(np.asarray(o["mask"])[None], dev))
            fl = f.get("flow")
            if fl is not None:
                flows.append(torch.from_numpy(np.ascontiguousarray(fl, np.float32)).to(dev) if not isinstance(fl, torch.Tensor) else fl.to(dev))
            flow_of.append(len(flows) - 1 if fl is not None else -1)
            fwd_given_p.append(mergetrack._dev_masks(f["fwd"], dev).reshape(P[t], h, w) if "fwd" in f and P[t] else None)
            fwd_given_a.append([mergetrack._dev_masks(np.asarray(o["fwd"])[None], dev) if "fwd" in o else None for o in f["ann"]])
        np_, na = int(tab.poff[t1] - tab.poff[t0]), int(tab.first[t1] - tab.first[t0])
        cur = torch.cat(cur_p + cur_a) if cur_p or cur_a else torch.zeros((0, h, w), dtype=torch.uint8, device=dev)
        fwd = torch.zeros_like(cur)
        if flows and cur.shape[0]:
            fom = np.concatenate([np.full(P[t], flow_of[t - t0], np.int32) for t in range(t0, t1)] +
                                 [np.full(len(frames[t]["ann"]), flow_of[t - t0], np.int32) for t in range(t0, t1)])
            for g0 in range(0, len(flows), MAX_WARP_FLOWS):       # premvos_mask_warp_seats_u8 takes at most 8 flows: a launch per group,
                grp = np.where((fom >= g0) & (fom < g0 + MAX_WARP_FLOWS), fom - g0, -1).astype(np.int32)      # the other masks are not written
                mergetrack.warp_masks_seats(cur, _i32(grp, dev), torch.stack(flows[g0:g0 + MAX_WARP_FLOWS]).contiguous(), out=fwd)
        for t in range(t0, t1):                                   # forward masks that came with the frame replace the warped ones
            if fwd_given_p[t - t0] is not None:
                fwd[int(tab.poff[t] - tab.poff[t0]):int(tab.poff[t + 1] - tab.poff[t0])] = fwd_given_p[t - t0]
            for j, g in enumerate(fwd_given_a[t - t0]):
                if g is not None:
                    fwd[np_ + int(tab.first[t] - tab.first[t0]) + j] = g[0]
        p0, k0 = int(tab.poff[t0]), int(tab.first[t0])
        pack_rows(cur[:np_], dv.pool[tab.cur0 + p0:tab.cur0 + p0 + np_])
        pack_rows(fwd[:np_], dv.pool[tab.fwd0 + p0:tab.fwd0 + p0 + np_])
        pack_rows(cur[np_:], dv.pool[tab.ann0 + k0:tab.ann0 + k0 + na])
        pack_rows(fwd[np_:], dv.pool[tab.annfwd0 + k0:tab.annfwd0 + k0 + na])
        t0 = t1
    if negatives is not None:
        dv.add_negatives(negatives)
    return dv


def ingest_bytes(frames: int, proposals: int, objects: int, h: int, w: int) -> int:
    """Upper bound of the device bytes ``VideoIngest`` holds for a video of ``frames`` frames with at most ``proposals`` masks each and
    ``objects`` annotated objects, at its peak: inside ``finish()`` the chunks' bit rows and the pool they are copied into exist side by
    side (twice the pool), beside the scores, the float64 embeddings and the tables.  What stays afterwards is half of the first term."""
    sumP, rb = int(frames) * int(proposals), row_bytes(int(h) * int(w))
    return 2 * (2 * sumP + 2 * int(objects)) * rb + sumP * (8 + EMB * 8) + int(objects) * EMB * 8 + (8 * frames + 2 * (frames + 1) + objects) * 4


def _dev_async(a: np.ndarray, dev) -> torch.Tensor:
    """a small host array -> HBM through page-locked memory, queued on the current stream (the caller's thread does not wait)"""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def warp_pack_rows(masks: torch.Tensor, counts: Sequence[int], flows: Optional[torch.Tensor], flow_of_frame: Optional[Sequence[int]] = None):
    """uint8 [n,h,w] in HBM, grouped by frame (``counts[k]`` masks of frame k, n = their sum), flows float32 [k,h,w,2] or None: frame k
    moves by flows[k], a frame beyond them by nothing (``flow_of_frame``: another assignment, -1 = by nothing) -> (cur_bits, fwd_bits)
    uint8 [n, row_bytes]: ONE premvos_mask_warp_pack_bits_u8 launch on the current stream."""
    n, h, w = masks.shape
    V = len(counts)
    assert n == sum(counts) and n > 0 and masks.is_contiguous() and masks.dtype == torch.uint8
    nfl = 0 if flows is None else int(flows.shape[0])
    if nfl:
        assert flows.is_contiguous() and flows.dtype == torch.float32 and tuple(flows.shape[1:]) == (h, w, 2)
    first = np.concatenate(([0], np.cumsum(np.asarray(counts, np.int64)))).astype(np.int32)
    fof = np.array([k if k < nfl else -1 for k in range(V)] if flow_of_frame is None else flow_of_frame, np.int32).reshape(V)
    dev, rb = masks.device, row_bytes(h * w)
    tables = _dev_async(np.concatenate((first, fof)), dev)
    cur = torch.empty((n, rb), dtype=torch.uint8, device=dev)
    fwd = torch.empty((n, rb), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().premvos_mask_warp_pack_bits_u8(
        masks.data_ptr(), n, h, w, first.ctypes.data, tables.data_ptr(), fof.ctypes.data, tables.data_ptr() + 4 * (V + 1),
        flows.data_ptr() if nfl else None, nfl, V, cur.data_ptr(), fwd.data_ptr(), rb, _lib.current_stream()), "mask_warp_pack_bits")
    return cur, fwd


class VideoIngest:
    """A ``DeviceVideo`` built chunk by chunk from arrays that are in HBM already (``stream --track --prewarp``: the refined masks,
    their [F,132] ReID rows, the scores and the flow block of a chunk), instead of ``upload()``'s frame dicts.  Per chunk ONE launch of
    premvos_mask_warp_pack_bits_u8 makes the chunk's current and forward bit rows -- the byte masks are not kept -- and one of
    premvos_track_inputs_f64 widens the embeddings (a row whose box has w <= 0 or h <= 0 becomes all +inf: ``read_props``' proposal
    without a "ReID" key).  ``finish()`` lays the pool out exactly as ``upload()`` does.  Only frame 0 carries annotations.

    The host side (``note_annotations`` / ``note_chunk`` / ``tables``) needs no GPU."""

    def __init__(self, h: int, w: int, device=None):
        self.h, self.w, self.hw = int(h), int(w), int(h) * int(w)
        self.device = device
        self.P: List[int] = []
        self.ids: List[int] = []
        self._chunks: List[tuple] = []               # (first proposal of the chunk, cur rows, fwd rows, scores, embeddings)
        self._ann = None                             # (cur rows, fwd rows, emb_t)

    # -- host ------------------------------------------------------------------------------------------------------------------------
    def note_annotations(self, ids: Sequence[int]) -> None:
        assert not self.P and not self.ids, "the annotated objects are frame 0's: they come first, once"
        self.ids = [int(i) for i in ids]

    def note_chunk(self, counts: Sequence[int]) -> int:
        """-> the index of the chunk's first proposal among the video's"""
        p0 = sum(self.P)
        self.P += [int(c) for c in counts]
        return p0

    def tables(self) -> Tables:
        return Tables(self.P, [len(self.ids)] + [0] * (len(self.P) - 1))

    # -- device ----------------------------------------------------------------------------------------------------------------------
    def add_annotations(self, objs: Sequence[Dict], flow: Optional[torch.Tensor]) -> None:
        """``objs``: frame 0's objects as ``upload()`` takes them ("id", "mask" [h,w], "reid" [128]); ``flow`` float32 [h,w,2] in HBM,
        frame 0's, or None (a one-frame video)."""
        self.note_annotations([o["id"] for o in objs])
        if not objs:
            return
        dev = _lib.resolve_device(self.device)
        masks = _dev_async(np.stack([np.asarray(o["mask"], np.uint8).reshape(self.h, self.w) for o in objs]), dev)
        cur, fwd = warp_pack_rows(masks, [len(objs)], None if flow is None else flow.reshape(1, self.h, self.w, 2))
        emb = _dev_async(np.array([np.asarray(o["reid"], np.float64) for o in objs]).reshape(len(objs), EMB), dev)
        self._ann = (cur, fwd, emb)

    def add_chunk(self, masks: torch.Tensor, counts: Sequence[int], flows: Optional[torch.Tensor], rows: torch.Tensor,
                  scores: torch.Tensor) -> None:
        """``masks`` uint8 [sumF,h,w] in HBM grouped by frame, ``counts`` per frame, ``flows`` float32 [k,h,w,2] (frame j < k of the chunk
        moves by flows[j]; a frame beyond them -- a video's last -- has empty forward masks) or None, ``rows`` float32 [sumF,132],
        ``scores`` float64 [sumF].  Everything is queued on the current stream."""
        n = int(sum(counts))
        p0 = self.note_chunk(counts)
        if n == 0:
            return
        assert tuple(masks.shape[1:]) == (self.h, self.w) and masks.shape[0] >= n
        assert rows.dtype == torch.float32 and rows.shape[0] >= n and rows.shape[1] == EMB + 4 and rows.is_contiguous()
        assert scores.dtype == torch.float64 and scores.shape[0] >= n and scores.is_contiguous()
        cur, fwd = warp_pack_rows(masks[:n], counts, flows)
        score = torch.empty((n,), dtype=torch.float64, device=masks.device)
        emb = torch.empty((n, EMB), dtype=torch.float64, device=masks.device)
        lib = _lib.load()
        for s in range(0, n, 65535):                 # (premvos_track_inputs_f64's bound per launch)
            k = min(65535, n - s)
            _lib.check(lib.premvos_track_inputs_f64(None, None, scores[s:].data_ptr(), rows[s:].data_ptr(), 0, k, score[s:].data_ptr(),
                                                    emb[s:].data_ptr(), _lib.current_stream()), "track_inputs")
        self._chunks.append((p0, cur, fwd, score, emb))

    def finish(self, negatives=None) -> DeviceVideo:
        """``Tables(P, A)`` of what was fed and the pool in ``upload()``'s layout; the chunks' rows are released.  ``negatives``: as
        ``upload``'s."""
        tab = self.tables()
        tab.check_caps()
        dv = DeviceVideo(tab, self.h, self.w, self.ids, self.device, negatives_room(negatives, self.P[0], tab.T))
        for p0, cur, fwd, score, emb in self._chunks:
            n = cur.shape[0]
            dv.pool[tab.cur0 + p0:tab.cur0 + p0 + n] = cur
            dv.pool[tab.fwd0 + p0:tab.fwd0 + p0 + n] = fwd
            dv.score[p0:p0 + n] = score
            dv.emb_p[p0:p0 + n] = emb
        if self._ann is not None:
            cur, fwd, emb = self._ann
            dv.pool[tab.ann0:tab.ann0 + tab.T] = cur
            dv.pool[tab.annfwd0:tab.annfwd0 + tab.T] = fwd
            dv.emb_t[:tab.T] = emb
        self._chunks, self._ann = [], None
        if negatives is not None:
            dv.add_negatives(negatives)
        return dv


def merge_video(frames: Sequence[Dict], h: int, w: int, weights=None, device=None, record: bool = False, negatives=None) -> Dict[str, object]:
    """oldmerge.py:129-218 for one video (``frames``: see ``upload``).  -> {"idmap": uint8 [N,h,w] in a page-locked host buffer,
    "ready": the event after which it holds the id maps, "idmap_dev": the same in HBM} and, with ``record``, chosen / best / weighted /
    reid / oreid / inter / areas (HBM) and the ``DeviceVideo``.  A video without annotated objects: all-zero id maps.  ``negatives``
    (None: off, "all", or a cap K): oldmerge.py's use_ff_negative_props -- frame 0's proposals that touch no annotated object and no
    proposal taken before become label-0 templates; "negatives": their frame-0 indices in acceptance order ([] when off)."""
    _lib.require_gpu()
    dev = _lib.resolve_device(device)
    N = len(frames)
    host = torch.empty((N, h, w), dtype=torch.uint8, pin_memory=True)
    if not any(len(f["ann"]) for f in frames):
        host.zero_()
        return {"idmap": host, "ready": None, "idmap_dev": None, "negatives": []}
    dv = upload(frames, h, w, dev, negatives)
    dv.prepare()
    c = dv.chain(normalised(weights)[None], want_weighted=record)
    idmap, _ = dv.paint(c["chosen"], c["best"])
    host.copy_(idmap, non_blocking=True)
    ready = torch.cuda.Event()
    ready.record()
    out: Dict[str, object] = {"idmap": host, "ready": ready, "idmap_dev": idmap, "negatives": dv.negatives}
    if record:
        out.update(c, reid=dv.reid, oreid=dv.oreid, inter=dv.inter, areas=dv.areas, video=dv)
    return out


def ensemble_video(frames: Sequence[Dict], h: int, w: int, weight_sets, device=None, record: bool = False, negatives=None) -> Dict[str, object]:
    """``merge_video`` under every row of ``weight_sets`` [K,5] (K = 2 .. 8; each row normalised as ``merge_video`` does) and the per-pixel
    vote of the K results -- the combination of oldmerge.py:129-131,220-224's runs under to_ensemble/<n>/: ONE chain launch resolves
    all sets, a paint launch per set fills a [K,N,h,w] stack (K * N * h * w bytes of HBM), one premvos_idmap_vote_u8 votes it; row 0
    breaks ties.  -> ``merge_video``'s keys (the voted maps) + "hist" int64 [K+1] in HBM (None for a video without annotated objects,
    whose maps are zero) and, with ``record``, "members" uint8 [K,N,h,w] in HBM."""
    _lib.require_gpu()
    dev = _lib.resolve_device(device)
    ws = np.array([normalised(x) for x in np.asarray(weight_sets, np.float64).reshape(-1, 5)])
    K, N = len(ws), len(frames)
    assert track.MIN_ENSEMBLE <= K <= track.MAX_SEATS, f"an ensemble has {track.MIN_ENSEMBLE} to {track.MAX_SEATS} weight sets (got {K})"
    if not any(len(f["ann"]) for f in frames):
        host = torch.zeros((N, h, w), dtype=torch.uint8).pin_memory()
        return {"idmap": host, "ready": None, "idmap_dev": None, "hist": None, "negatives": []}
    dv = upload(frames, h, w, dev, negatives)
    dv.prepare()
    c = dv.chain(ws)
    members = torch.empty((K, N, h, w), dtype=torch.uint8, device=dev)
    for k in range(K):                                            # (the paint entry writes an id map for W == 1 only)
        dv.paint(c["chosen"][k:k + 1], c["best"][k:k + 1], out=members[k])
    v = track.vote_idmaps(members)
    host, ready = track.stack_to_host(v["voted"])
    out: Dict[str, object] = {"idmap": host, "ready": ready, "idmap_dev": v["voted"], "hist": v["hist"], "negatives": dv.negatives}
    if record:
        out["members"] = members
    return out


def scores_from_counts(counts: np.ndarray) -> np.ndarray:
    """eval_video (merge_functions.py:613-634) from integer counts [W,N,T0,3] = |R and G|, |R or G|, |R|: float64 [W,T0], the mean
    over frames 1 .. N-2, summed in frame order -- host floats from integers, so they equal the reference's."""
    c = np.asarray(counts, np.int64)
    W, N, T0, _ = c.shape
    scores = np.zeros((W, T0))
    for t in range(1, N - 1):
        inter, union, area = c[:, t, :, 0], c[:, t, :, 1], c[:, t, :, 2]
        absent = (union - area + inter) == 0                          # |G| == 0: the id is not in this frame's annotation
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = np.where(inter != 0, inter / np.where(union == 0, 1, union), 0.0)
        scores += np.where(absent, np.where(area == 0, 1.0, 0.0), iou)
    with np.errstate(invalid="ignore", divide="ignore"):
        return scores / (N - 2)


def first_frame_ids(frames: Sequence[Dict]) -> int:
    ids = [int(o["id"]) for o in frames[0]["ann"]] if len(frames) else []
    if ids != list(range(1, len(ids) + 1)):
        raise _lib.PremvosError(f"prewarp search: object k is scored against annotation id k + 1 (merge_functions.py:623), so frame 0 must hold "
                                f"the ids 1 .. T0; it holds {ids}")
    return len(ids)


def gt_bit_planes(gt: np.ndarray, T0: int, dev) -> torch.Tensor:
    """annotation id maps uint8 [N,h,w] -> uint8 [N,T0,row_bytes]: plane k = (gt == k + 1), bit-packed"""
    N, h, w = gt.shape
    out = torch.zeros((N, T0, row_bytes(h * w)), dtype=torch.uint8, device=dev)
    ids = torch.arange(1, T0 + 1, dtype=torch.uint8, device=dev).view(1, T0, 1, 1)
    step = max(1, CHUNK_BYTES // max(1, T0 * h * w))
    for t0 in range(0, N, step):
        g = torch.from_numpy(np.ascontiguousarray(gt[t0:t0 + step])).to(dev)
        planes = (g[:, None] == ids).to(torch.uint8).reshape(-1, h, w)
        pack_rows(planes, out[t0:t0 + g.shape[0]].view(-1, out.shape[2]))
    return out


def search(frames: Sequence[Dict], h: int, w: int, gt: np.ndarray, weight_sets: np.ndarray, device=None, negatives=None) -> Dict[str, np.ndarray]:
    """The objective of oldmerge.py's random search for every row of ``weight_sets`` [W,5] at once: ``gt`` uint8 [N,h,w] = the
    annotation id map of EVERY frame.  -> {"scores": float64 [W,T0], "counts": int64 [W,N,T0,3]}."""
    _lib.require_gpu()
    dev = _lib.resolve_device(device)
    T0 = first_frame_ids(frames)
    assert gt.shape == (len(frames), h, w), (gt.shape, len(frames), h, w)
    ws = np.array([normalised(x) for x in np.asarray(weight_sets, np.float64).reshape(-1, 5)])
    if T0 == 0:                                                   # no object in frame 0: nothing is scored (eval_video's empty array)
        return {"scores": np.zeros((len(ws), 0)), "counts": np.zeros((len(ws), len(frames), 0, 3), np.int64), "weights": ws, "negatives": []}
    dv = upload(frames, h, w, dev, negatives)
    dv.prepare()
    c = dv.chain(ws)
    _, counts = dv.paint(c["chosen"], c["best"], idmap=False, gt_bits=gt_bit_planes(np.asarray(gt, np.uint8), T0, dev), T0=T0)
    counts = counts.cpu().numpy().astype(np.int64)
    return {"scores": scores_from_counts(counts), "counts": counts, "weights": ws, "negatives": dv.negatives}


# --------------------------------------------------------------------------------------------------------------------- a file tree
def read_video(name: str, lay: Dict[str, str], late: bool, add_ReID, ReID_net, need_gt: bool = False):
    """The tree ``track`` reads -> (frames for ``upload``, (h, w), image file names, gt id maps or None).  Proposal files are parsed as
    ``track --lockstep`` parses them (read_props + parse_fresh, ahead on the io pool); annotation objects get their embedding the
    host route, once per annotated frame (``Tracker.add_templates``'s).  ``late`` off: only 00000's annotation counts (merge.py:78)."""
    from PIL import Image
    from . import io_pipeline as iop
    fns = sorted(glob.glob(os.path.join(lay["images"], name) + "/*"))
    if not fns:
        return [], None, fns, None
    sizes = {track._image_size(fn) for fn in fns}
    if len(sizes) != 1:
        raise _lib.PremvosError(f"premvos_amd.track: --prewarp: the frames of {name} differ in size ({sorted(sizes)}): one pool holds one size")
    h, w = next(iter(sizes))

    def load(k):
        ann_fn, prop_fn, flow_fn, _ = track._frame_paths(fns[k], lay)
        fresh = track.parse_fresh(track.read_props(prop_fn))
        if k + 1 < len(fns) and not os.path.exists(flow_fn):
            raise _lib.PremvosError(f"premvos_amd.track: --prewarp: {flow_fn} is missing: only a video's last frame may lack a flow (its masks "
                                    "are warped to the next frame with it)")
        flow = mergetrack.get_flow(flow_fn) if k + 1 < len(fns) else None
        ann = np.array(Image.open(ann_fn)) if os.path.exists(ann_fn) and (need_gt or late or k == 0) else None
        return fresh, flow, ann, ann_fn
    frames, seen, gts = [], set(), []
    for k, (fresh, flow, ann, ann_fn) in enumerate(iop.prefetch(range(len(fns)), load)):
        if fresh["F"] and fresh["size"] != (h, w):
            raise _lib.PremvosError(f"premvos_amd.track: --prewarp: {name} frame {k}: proposals of {fresh['size']}, frames of {(h, w)}")
        objs = []
        if ann is not None and (k == 0 and "00000.jpg" in fns[0] or (late and k > 0)):
            new = [t for t in track.read_ann(ann_fn) if int(t["id"]) not in seen]
            if new:
                new = add_ReID(new, fns[k], ReID_net)
                for t in new:
                    seen.add(int(t["id"]))
                    objs.append({"id": int(t["id"]), "mask": (ann == t["id"]).astype(np.uint8), "reid": np.asarray(t["ReID"], np.float64)})
        if need_gt:
            if ann is None:
                raise _lib.PremvosError(f"premvos_amd.track: --prewarp-search needs an annotation for every frame; {ann_fn} is missing")
            gts.append(ann.astype(np.uint8))
        fr = {"score": fresh["score"], "emb": fresh["emb"], "pool": fresh["pool"], "offsets": fresh["offsets"], "ann": objs}
        if flow is not None:
            fr["flow"] = flow
        frames.append(fr)
    return frames, (h, w), fns, (np.array(gts) if need_gt else None)


def run_tree(root: str, videos: Sequence[str], weights=None, late: bool = False, search_sets: int = 0, seed: int = 0, add_ReID=None,
             ReID_net=None, writer=None, eval_dir: Optional[str] = None, overlay_dir: Optional[str] = None,
             lay: Optional[Dict[str, str]] = None, ensemble_sets=None, ensemble_source: str = "--ensemble", negatives=None) -> Dict[str, object]:
    """``track --prewarp`` / ``--prewarp-search`` under ``root``: PNGs under output/final_prewarp/ (never output/final/), or
    output/prewarp_search.json and no PNGs.  Videos are independent.  ``ensemble_sets`` [K,5] (``track --prewarp --ensemble``): every
    video through ``ensemble_video`` instead of ``merge_video``, the voted PNGs under output/final_prewarp_ensemble/ (never
    output/final_prewarp/) and output/prewarp_ensemble.json (``track.ensemble_result``).  ``eval_dir`` / ``overlay_dir``: as ``track.do_video``'s -- every
    frame's id map goes from HBM to the video's ``evaluate.LoopEval`` (as ``Tracker.evaluator`` gets it) and to ``overlay.forward`` (as
    ``Tracker.on_idmap`` does).  ``lay``: other roots than ``track._layout(root)``'s (images, anns, props, flows, out).
    ``negatives`` (``track --negatives [K]``: "all" or a cap): every video with its negative first-frame templates; ``_neg`` follows
    ``prewarp`` in every name (output/final_prewarp_neg/, final_prewarp_neg_ensemble/, prewarp_neg_search.json, prewarp_neg_ensemble.json
    -- never the places of the run without the flag) and output/prewarp_negatives.json lists what each video took."""
    from . import io_pipeline as iop
    from .merge_out import VideoOut
    assert not (search_sets and ensemble_sets is not None), "the search writes no id maps: nothing to vote"
    stem = "prewarp" if negatives is None else "prewarp_neg"
    final = f"output/final_{stem}" if ensemble_sets is None else f"output/final_{stem}_ensemble"
    lay = dict(track._layout(root), out=os.path.join(root, final) + "/") if lay is None else lay
    dev = _lib.resolve_device(None)
    if add_ReID is None:
        add_ReID = track._default_engine_calls(None, None)[1]
    own = writer is None
    writer = iop.Writer() if own else writer
    frames_done, result, taken = 0, {"videos": {}}, {}
    ws = search_weights(search_sets, seed) if search_sets else None
    try:
        for name in videos:
            frames, size, fns, gt = read_video(name, lay, late, add_ReID, ReID_net, need_gt=bool(search_sets))
            if not frames:
                continue
            if search_sets:
                r = res = search(frames, size[0], size[1], gt, ws, dev, negatives)
                result["videos"][name] = {"scores": r["scores"].tolist()}
            elif ensemble_sets is not None:
                res = ensemble_video(frames, size[0], size[1], ensemble_sets, dev, negatives=negatives)
                VideoOut(name, lay["out"], writer, dev, lay["anns"], eval_dir, overlay_dir).whole_video(fns, res)
                K = len(ensemble_sets)                            # (no annotated object: K blank members agree everywhere)
                hist = res["hist"].cpu().numpy() if res["hist"] is not None else np.array([0] * K + [len(frames) * size[0] * size[1]])
                result["videos"][name] = {"frames": len(frames), "hist": hist}
            else:
                res = merge_video(frames, size[0], size[1], weights, dev, negatives=negatives)
                VideoOut(name, lay["out"], writer, dev, lay["anns"], eval_dir, overlay_dir).whole_video(fns, res)
            if negatives is not None:
                score0 = np.asarray(frames[0]["score"], np.float64).reshape(-1)
                taken[name] = {"candidates": len(score0), "taken": list(res["negatives"]), "scores": [float(score0[i]) for i in res["negatives"]],
                               "templates": sum(len(f["ann"]) for f in frames) + len(res["negatives"])}
            frames_done += len(frames)
    finally:
        if own:
            writer.close()
    result["frames"] = frames_done
    if negatives is not None:
        os.makedirs(os.path.join(root, "output"), exist_ok=True)
        with open(os.path.join(root, "output", "prewarp_negatives.json"), "w") as f:
            json.dump({"negatives": "all" if negatives_cap(negatives) < 0 else negatives_cap(negatives), "videos": taken}, f, indent=1)
    if search_sets:
        per_set = [[s for v in result["videos"].values() for s in v["scores"][i]] for i in range(search_sets)]
        result.update(weights=ws.tolist(), seed=seed, mean=[float(np.mean(x)) if x else None for x in per_set])
        os.makedirs(os.path.join(root, "output"), exist_ok=True)
        with open(os.path.join(root, "output", f"{stem}_search.json"), "w") as f:
            json.dump(result, f, indent=1)
    if ensemble_sets is not None:
        ws = np.array([normalised(x) for x in np.asarray(ensemble_sets, np.float64).reshape(-1, 5)])
        result = track.ensemble_result(result["videos"], len(ws), ws, ensemble_source)
        track.write_ensemble_json(os.path.join(root, "output", f"{stem}_ensemble.json"), result)
    return result
