"""MergeTrack's two diagnostics next to its loop, on the GPU (csrc/viz_ops.hip):

    python -m premvos_amd.track --root <PReMVOS root> --viz [--combine ..] [--oracle]    ->  output/viz/<video>/<frame>.jpg
    python -m premvos_amd.track --root <PReMVOS root> --max-reid-distance                ->  output/max_reid_distance.json

``viz_scores`` (MergeTrack/merge_functions.py:547-611, imported by merge.py:51 and never called there) draws one SCORE SHEET per frame:
every candidate's crop with its mask tinted; under it, per template, the five score planes, the weighted score and the ground-truth
IoU as colour cells (red = 0, green = 1); a black mark on the candidate the weights chose and on the one the annotation would choose.
``sheet`` makes it in HBM from what the loop already holds there (``premvos_viz_scores_u8``: crop + cv2's fixed-point resize + tint,
the cells, the marks and scipy.misc.imsave's bytescale with the canvas' global extremes, found on the device); ``jpeg.encode(sheet, 75,
"4:2:0")`` is the file PIL writes for it, the Huffman pass on a writer thread.

``print_max_reid_distance.py`` (the program ``MAX_REID_DISTANCE = 25`` of merge_functions.py:12 was read from) is ``max_reid_distance``
(``premvos_reid_max_distance_f64``: one launch per video) and ``max_reid_distance_tree``.

Rules of this package's own (the reference has none or would raise): the tint is ``track.voc_palette()[2]`` (tensorpack's table is not
known here; a parameter); a crop is clipped to the frame and a crop that is empty then gives a black tile; a non-finite weighted score
counts as 0, a non-finite plane or gt value is drawn as 0 and does not enter the extremes; a negative box origin is clipped to 0.
"""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, jpeg

BOX = 100                                                                     # merge_functions.py:559
QUALITY, SUBSAMPLING = 75, "4:2:0"                                            # PIL's defaults: what scipy.misc.imsave's save() writes
COMPILED_IN = 25                                                              # merge_functions.py:12, csrc/track_ops.hip
EMB = 128


def default_tint() -> np.ndarray:
    """draw_mask's ``PALETTE_RGB[color + 1][::-1]`` for ``color=1``, with the DAVIS palette standing in for tensorpack's: uint8 [3]."""
    from .track import voc_palette
    return voc_palette()[2][::-1].copy()


def workspace_bytes(T: int, P: int) -> int:
    """premvos_viz_scores_u8's workspace (include/premvos_hip.h)."""
    return 16 * (int(P) + 1) + 8 * int(T)


def _f64(x, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    return t.to(device=dev, dtype=torch.float64)


def sheet(frame: torch.Tensor, masks: torch.Tensor, boxes, planes, weighted, gt, tint=None) -> torch.Tensor:
    """premvos_viz_scores_u8 on the current stream -> the score sheet, uint8 [100 (T + 1), 100 P, 3] in HBM (after bytescale).
    ``frame`` uint8 [h,w,3] and ``masks`` uint8 [P,h,w] (nonzero = foreground) in HBM; ``boxes`` [P,4] = x, y, w, h (truncated toward
    zero, as viz_scores' ``int()``), ``planes`` [5,T,P], ``weighted`` [T,P] or [T,P+1] (``track_scores``': the threshold column is not
    read), ``gt`` [T,P]: float64 arrays or CUDA tensors; ``tint``: three bytes (default ``default_tint()``)."""
    _lib.require_gpu()
    if not (isinstance(frame, torch.Tensor) and frame.is_cuda and frame.dtype == torch.uint8 and frame.dim() == 3 and frame.shape[2] == 3):
        raise ValueError("sheet() takes a uint8 [h,w,3] frame in HBM")
    dev = frame.device
    h, w = int(frame.shape[0]), int(frame.shape[1])
    if not (isinstance(masks, torch.Tensor) and masks.dtype == torch.uint8 and masks.dim() == 3 and tuple(masks.shape[1:]) == (h, w)
            and masks.device == dev):
        raise ValueError(f"masks: a uint8 [P,{h},{w}] tensor on the frame's device")
    P = int(masks.shape[0])
    pl, ws, g, bx = _f64(planes, dev).contiguous(), _f64(weighted, dev), _f64(gt, dev).contiguous(), _f64(boxes, dev).contiguous()
    if pl.dim() != 3 or pl.shape[0] != 5 or pl.shape[2] != P:
        raise ValueError(f"planes: [5,T,{P}] (got {tuple(pl.shape)})")
    T = int(pl.shape[1])
    if ws.dim() != 2 or ws.shape[0] != T or ws.shape[1] not in (P, P + 1) or tuple(g.shape) != (T, P) or tuple(bx.shape) != (P, 4):
        raise ValueError(f"weighted [{T},{P}] or [{T},{P + 1}], gt [{T},{P}], boxes [{P},4] (got {tuple(ws.shape)}, {tuple(g.shape)}, {tuple(bx.shape)})")
    ws = ws if ws.stride(1) == 1 else ws.contiguous()
    tint3 = np.ascontiguousarray(default_tint() if tint is None else np.asarray(tint), dtype=np.uint8)
    assert tint3.shape == (3,), tint3.shape
    frame, masks = frame.contiguous(), masks.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((BOX * (T + 1), BOX * P, 3), dtype=torch.uint8, device=dev)
        work = torch.empty((workspace_bytes(T, P) // 8,), dtype=torch.float64, device=dev)
        _lib.check(_lib.load().premvos_viz_scores_u8(frame.data_ptr(), h, w, masks.data_ptr(), bx.data_ptr(), P, pl.data_ptr(), ws.data_ptr(),
                                                     ws.stride(0), g.data_ptr(), T, tint3.ctypes.data, work.data_ptr(), work.numel() * 8,
                                                     out.data_ptr(), _lib.current_stream()), "viz_scores")
    return out


def forward(sheet_u8: torch.Tensor) -> jpeg.Encoded:
    """The device half of a sheet's file (current stream): DCT + quantisation at PIL's default quality, coefficients on their way to a
    pinned buffer; ``overlay.write_jpg`` is the host half."""
    return jpeg.forward(sheet_u8, QUALITY, SUBSAMPLING)


def write_sheet(filename: str, sheet_u8: torch.Tensor, writer=None) -> None:
    """``filename`` = the bytes of ``PIL.Image.fromarray(sheet).save(filename)`` (quality 75, 4:2:0); with ``writer`` (an
    ``io_pipeline.Writer``) the Huffman pass and the write run there."""
    from . import overlay
    enc = forward(sheet_u8)
    if writer is None:
        overlay.write_jpg(filename, enc)
    else:
        writer.submit(overlay.write_jpg, filename, enc)


def viz_scores(all_scores, weighted_scores, proposals: Sequence[Dict], image_fn: str, input_images: str, gt_scores, out_dir: str,
               writer=None, tint=None, device=None) -> str:
    """merge_functions.py:553-611 with its call shape (``out_dir`` instead of the hard-coded "DAVIS/viz2/"): ``proposals`` are dicts with
    'bbox' and 'segmentation', the frame is read from ``image_fn``; writes ``image_fn`` with ``input_images`` replaced by ``out_dir``
    (``out_dir``/<video>/<frame>.jpg) and returns that name."""
    from PIL import Image
    from .track import decode_segmentations
    _lib.require_gpu()
    dev = _lib.resolve_device(device)
    out_fn = image_fn.replace(input_images, out_dir)
    frame = jpeg.to_device(np.asarray(Image.open(image_fn).convert("RGB")), dev)
    masks = decode_segmentations([p["segmentation"] for p in proposals], device=dev)
    boxes = np.array([np.asarray(p["bbox"], np.float64) for p in proposals], np.float64).reshape(len(proposals), 4)
    gt = np.asarray(gt_scores, np.float64)
    write_sheet(out_fn, sheet(frame, masks, boxes, all_scores, weighted_scores, gt[0] if gt.ndim == 3 else gt, tint), writer)
    return out_fn


# ----------------------------------------------------------------------------------------------------- print_max_reid_distance.py
def max_reid_distance(templates, proposals, device=None):
    """premvos_reid_max_distance_f64 -> (max_distance float64 [T], over int64 [T]) CUDA tensors: per template the largest
    ``norm(c - t)`` over ``proposals`` [N,128] (an infinite distance counts as 0; N = 0 gives zeros) and how many exceed 25."""
    _lib.require_gpu()
    dev = templates.device if isinstance(templates, torch.Tensor) and templates.is_cuda else _lib.resolve_device(device)
    t = _f64(np.asarray(templates, np.float64).reshape(-1, EMB) if not isinstance(templates, torch.Tensor) else templates, dev).contiguous()
    p = _f64(np.asarray(proposals, np.float64).reshape(-1, EMB) if not isinstance(proposals, torch.Tensor) else proposals, dev).contiguous()
    assert t.dim() == 2 and t.shape[1] == EMB and t.shape[0] >= 1 and p.dim() == 2 and p.shape[1] == EMB, (t.shape, p.shape)
    T, N = int(t.shape[0]), int(p.shape[0])
    with torch.cuda.device(dev):
        out = torch.empty((T,), dtype=torch.float64, device=dev)
        over = torch.empty((T,), dtype=torch.int64, device=dev)
        _lib.check(_lib.load().premvos_reid_max_distance_f64(t.data_ptr(), T, p.data_ptr() if N else None, N, out.data_ptr(), over.data_ptr(),
                                                             _lib.current_stream()), "reid_max_distance")
    return out, over


def _frame_embeddings(prop_fn: str) -> np.ndarray:
    """One frame's proposal embeddings, float64 [F,128] (``read_props``: a proposal without 'ReID' is all inf, an unreadable file is
    no proposal).  Pure host work: runs on the io pool."""
    from .track import read_props
    props = read_props(prop_fn)
    return np.array([np.asarray(p["ReID"], np.float64) for p in props], np.float64).reshape(len(props), EMB)


def max_reid_distance_video(video: str, images: str, anns: str, props: str, ReID_net, add_ReID: Optional[Callable] = None, pool=None,
                            device=None) -> Optional[Dict[str, object]]:
    """print_max_reid_distance.py:18-50 for one video (``images`` / ``anns`` / ``props``: the roots, with a trailing slash): the templates
    are the objects of EVERY frame with an annotation PNG, embedded on their own frame; the proposals of all frames are pooled.
    -> {"per_template", "max", "pairs", "over"}, or None for a video without annotation or frames."""
    import glob
    from .track import _frame_paths, read_ann
    if add_ReID is None:
        from .reid.driver import add_ReID
    fns = sorted(glob.glob(os.path.join(images, video) + "/*"))
    lay = {"images": images, "anns": anns, "props": props, "flows": "", "out": ""}
    prop_fns = [_frame_paths(fn, lay)[1] for fn in fns]
    pending = [pool.submit(_frame_embeddings, fn) for fn in prop_fns] if pool is not None else None       # read while the net embeds
    templates: List[Dict] = []
    for fn in fns:
        ann_fn = _frame_paths(fn, lay)[0]
        if os.path.isfile(ann_fn):
            templates = templates + add_ReID(read_ann(ann_fn), fn, ReID_net)
    embs = [f.result() for f in pending] if pending is not None else [_frame_embeddings(fn) for fn in prop_fns]
    if not templates or not fns:
        return None
    pooled = np.concatenate(embs) if embs else np.zeros((0, EMB), np.float64)
    t = np.array([np.asarray(x["ReID"], np.float64) for x in templates], np.float64).reshape(len(templates), EMB)
    best, over = max_reid_distance(t, pooled, device)
    best, over = best.cpu().numpy(), over.cpu().numpy()
    return {"per_template": [float(x) for x in best], "max": float(best.max()), "pairs": int(len(templates) * pooled.shape[0]),
            "over": int(over.sum())}


def max_reid_distance_tree(root: str, videos: Sequence[str], ReID_net, add_ReID: Optional[Callable] = None) -> Dict[str, object]:
    """The whole program on a tree: one line per video and the data set's maximum on stdout, and ``root``/output/max_reid_distance.json:
    per video the per-template maxima, the maximum over everything, ``compiled_in`` = 25 and how many (template, proposal) pairs
    exceeded it.  The JSONs are read on the io pool."""
    from . import io_pipeline as iop
    from .track import _layout
    lay = _layout(root)
    res: Dict[str, object] = {"videos": {}, "max": None, "compiled_in": COMPILED_IN, "pairs": 0, "pairs_over_compiled_in": 0}
    with iop.thread_pool(max(1, iop.io_threads()), "premvos-max-reid") as pool:
        for v in videos:
            r = max_reid_distance_video(v, lay["images"], lay["anns"], lay["props"], ReID_net, add_ReID, pool)
            if r is None:
                print(f"premvos_amd.track: {v}: no annotation, no distances")
                continue
            res["videos"][v] = r
            res["pairs"] += r["pairs"]
            res["pairs_over_compiled_in"] += r["over"]
            print(f"premvos_amd.track: {v}: max ReID distance per template {r['per_template']}")
    vals = [r["max"] for r in res["videos"].values()]
    if vals:                                                                  # (np.max's rule: a NaN wins)
        res["max"] = float(np.max(vals))
    fn = os.path.join(root, "output", "max_reid_distance.json")
    os.makedirs(os.path.dirname(fn), exist_ok=True)
    with open(fn, "w") as f:
        json.dump(res, f, indent=1)
    print(f"premvos_amd.track: max ReID distance {res['max']}  (compiled in: {COMPILED_IN}; {res['pairs_over_compiled_in']} of {res['pairs']} "
          f"pairs beyond it)  ->  {fn}")
    return res
