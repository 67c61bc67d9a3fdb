"""Per-object largest-component clean-up of id maps that already exist: the rule of ReID_net/scripts/postproc/postproc.py:41-63
(``postproc_posteriors_connected_components``: dilate the mask with a 100 x 100 box, label the connected components of the DILATED
mask, count the original pixels in each, keep the largest) over any tree of palette PNGs this package wrote, on the GPU
(csrc/components_ops.hip, declared in include/premvos_post_hip.h):

    python -m premvos_amd.components --root <PReMVOS root> --input final [--out final_cc] [--dilate 100] [--videos a,b] [--eval] [--overlay]
                                     [--check-only]
        output/<input>/<video>/<frame>.png  ->  output/<out>/<video>/<frame>.png, output/<out>.json
                                   [--eval]      output/eval_<out>/<video>.json, output/premvos_amd_davis_eval_<out>.json
                                   [--overlay]   output/overlay_<out>/<video>/<frame>.jpg   (needs data/DAVIS/JPEGImages/480p/<video>/<frame>.jpg)

The reference works on a two-class posterior; here the rule runs per object id k >= 1 on ``(M == k)``, independently of the other ids:
parts of an object that an occluder separates stay (they sit within the box of one another), distant blobs go.  Freed pixels become
background, never another object.  A tie between components goes to the one whose dilated blob comes first in raster order
(postproc.py:48-54's strict ``>``).  Integers only: the result is exact, a frame's result does not depend on the frames it is stacked with.
It chains behind the CRF: ``crf --input final``, then ``components --input final_crf``.  Per video the PNGs are decoded on the io pool,
L = 1 + the largest id of the video (a video of background alone is copied without a launch), ``keep_largest`` runs the frames in
chunks and ``merge_out.VideoOut.whole_video`` writes the files, as for every other merge.  ``--check-only`` names a missing tree, a video
without PNGs and PNGs of different sizes (with ``--overlay`` also what ``premvos_amd.crf`` names about the frames), and needs no GPU.

As a library: ``label(masks)`` labels any binary planes (8-connected, a pixel's label = the smallest linear index of its component, -1 on
background), ``dilate(idmaps, L, D)`` gives the dilated planes, ``keep_largest(idmaps, L, dilate=100)`` applies the rule."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

DILATE = 100                                                                  # postproc.py:43
MIN_L, MAX_L, MIN_DILATE, MAX_DILATE = 2, 256, 1, 255                         # (csrc/components_ops.hip refuses the same)
PLANE_PIXEL_BYTES = 9                                                         # keep_largest: dilated mask 1, labels 4, counts 4
CHUNK_BYTES = 1 << 30


def _idmaps3(idmaps):
    import torch
    assert idmaps.is_cuda and idmaps.dtype == torch.uint8 and idmaps.dim() in (2, 3), (idmaps.dtype, idmaps.shape)
    return (idmaps if idmaps.dim() == 3 else idmaps[None]).contiguous()


def label(masks):
    """uint8 [P,H,W] (or [H,W]), CUDA, non-zero = set -> int32 of the same shape: the smallest linear index y * W + x of the pixel's
    8-connected component inside its plane, -1 on background.  Four launches on the current stream."""
    import torch
    from . import _lib
    _lib.require_gpu()
    m = _idmaps3(masks)
    P, H, W = m.shape
    labels = torch.empty((P, H, W), dtype=torch.int32, device=m.device)
    _lib.check(_lib.load().premvos_cc_label_i32(m.data_ptr(), P, H, W, labels.data_ptr(), _lib.current_stream()), "cc_label")
    return labels if masks.dim() == 3 else labels[0]


def dilate(idmaps, L: int, D: int = DILATE):
    """uint8 [N,H,W] (or [H,W]), CUDA -> uint8 [N,L-1,H,W] (or [L-1,H,W]): ``grey_dilation(M == k, size=(D, D))`` for k = 1 .. L-1."""
    import torch
    from . import _lib
    _lib.require_gpu()
    m = _idmaps3(idmaps)
    N, H, W = m.shape
    dil = torch.empty((N, max(L - 1, 0), H, W), dtype=torch.uint8, device=m.device)
    _lib.check(_lib.load().premvos_cc_dilate_u8(m.data_ptr(), N, H, W, L, D, dil.data_ptr(), _lib.current_stream()), "cc_dilate")
    return dil if idmaps.dim() == 3 else dil[0]


def keep_largest(idmaps, L: int, dilate: int = DILATE, chunk_bytes: int = CHUNK_BYTES):
    """idmaps uint8 [N,H,W] (CUDA), object ids below L -> {"idmap": uint8 [N,H,W], "removed": int32 [N,L-1] (the pixels of id k set to 0, at
    [:, k-1]), "components": int32 [N,L-1] (the components of id k's dilated mask; 0: the id is absent)}, all CUDA.  The frames run in chunks
    whose dilated planes, labels and counts (9 bytes per plane pixel) stay below ``chunk_bytes``; a frame's result does not depend on
    its chunk.  Eight launches and three memsets per chunk on the current stream; nothing waits."""
    import torch
    from . import _lib
    _lib.require_gpu()
    assert idmaps.dim() == 3, idmaps.shape
    m = _idmaps3(idmaps)
    N, H, W = m.shape
    lib, planes = _lib.load(), max(L - 1, 0)
    out = torch.empty_like(m)
    removed, ncomp = (torch.empty((N, planes), dtype=torch.int32, device=m.device) for _ in range(2))
    chunk = min(N, 65535, max(1, int(chunk_bytes) // max(1, PLANE_PIXEL_BYTES * planes * H * W)))
    dil = torch.empty((chunk, planes, H, W), dtype=torch.uint8, device=m.device)
    labels, counts = (torch.empty((chunk, planes, H, W), dtype=torch.int32, device=m.device) for _ in range(2))
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        s = _lib.current_stream()
        _lib.check(lib.premvos_cc_dilate_u8(m[a:b].data_ptr(), b - a, H, W, L, dilate, dil.data_ptr(), s), "cc_dilate")
        _lib.check(lib.premvos_cc_label_i32(dil.data_ptr(), (b - a) * planes, H, W, labels.data_ptr(), s), "cc_label")
        _lib.check(lib.premvos_cc_keep_largest_u8(m[a:b].data_ptr(), labels.data_ptr(), b - a, H, W, L, counts.data_ptr(), out[a:b].data_ptr(),
                                                  removed[a:b].data_ptr(), ncomp[a:b].data_ptr(), s), "cc_keep_largest")
    return {"idmap": out, "removed": removed, "components": ncomp}


# ------------------------------------------------------------------------------------------------------------------- the command
def check_tree(root: str, name: str, videos, images: Optional[str] = None) -> List[str]:
    """Pure host -> a missing output/<name>, every video without PNGs and every video whose PNGs differ in size (empty = the tree can be
    cleaned).  ``images`` (``--overlay``): also every PNG without its frame there, frame without its PNG and size that differs, as
    ``crf.check_tree`` names them.  Only headers are read."""
    from PIL import Image
    from .ensemble import tree_dir, tree_frames
    if images is not None:
        from .crf import check_tree as with_frames
        return with_frames(root, name, videos, images)
    if not os.path.isdir(tree_dir(root, name)):
        return [f"{tree_dir(root, name)} is missing"]
    problems = []
    for video in videos:
        stems = tree_frames(root, name, video)
        if not stems:
            problems.append(f"{video}: no PNGs under {os.path.join(tree_dir(root, name), video)}")
            continue
        sizes = set()
        for s in stems:
            with Image.open(os.path.join(tree_dir(root, name), video, s + ".png")) as im:
                sizes.add((im.size[1], im.size[0]))
        if len(sizes) > 1:
            problems.append(f"{video}: its PNGs differ in size ({sorted(sizes)}): one stack holds one size")
    return problems


def clean_video(root: str, name: str, video: str, lay: Dict[str, str], D: int, writer, eval_dir: Optional[str] = None,
                overlay_dir: Optional[str] = None) -> Dict[str, object]:
    """One video of the tree: decode, ``keep_largest``, ``VideoOut.whole_video`` under ``lay["out"]`` -> {"frames", "L", "removed" [N][L-1],
    "components" [N][L-1]}.  A video of background alone (L = 1) is written as it is, without a launch."""
    import torch
    from . import _lib, track
    from .ensemble import read_stack, tree_frames
    from .merge_out import VideoOut
    dev = _lib.resolve_device(None)
    stems = tree_frames(root, name, video)
    maps = read_stack(root, [name], video, stems)[0]
    L = 1 + int(maps.max())
    fns = [os.path.join(lay["images"], video, stem + ".jpg") for stem in stems]
    sink = VideoOut(video, lay["out"], writer, dev, lay["anns"], eval_dir, overlay_dir, program="premvos_amd.components")
    if L < MIN_L:
        sink.whole_video(fns, {"idmap": torch.from_numpy(maps), "ready": None, "idmap_dev": None})
        return {"frames": len(stems), "L": L, "removed": [[] for _ in stems], "components": [[] for _ in stems]}
    r = keep_largest(torch.from_numpy(maps).to(dev), L, D)
    host, ready = track.stack_to_host(r["idmap"])
    sink.whole_video(fns, {"idmap": host, "ready": ready, "idmap_dev": r["idmap"]})
    return {"frames": len(stems), "L": L, "removed": r["removed"].cpu().tolist(), "components": r["components"].cpu().tolist()}


def parse_args(argv: Optional[List[str]] = None):
    """The command line and its refusals (no file is looked at) -> the namespace."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=".")
    ap.add_argument("--input", required=True, help="the tree's name under output/ (final, final_crf, final_prewarp, final_vote, ...)")
    ap.add_argument("--out", default=None, help="the cleaned tree's name under output/ (default <input>_cc)")
    ap.add_argument("--dilate", type=int, default=DILATE, metavar="D",
                    help=f"the side of the dilation box, {MIN_DILATE} to {MAX_DILATE} (default {DILATE}, postproc.py:43; 1 = the object's own components)")
    ap.add_argument("--eval", action="store_true", help="also score the cleaned maps against data/DAVIS/Annotations/480p on the GPU")
    ap.add_argument("--overlay", action="store_true", help="also write every frame with the cleaned objects tinted (needs the frames)")
    ap.add_argument("--videos", default=None, help="comma-separated video names (default: every folder of the input)")
    ap.add_argument("--check-only", action="store_true", help="name what is missing or differs in size and stop (no GPU)")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = a.input + "_cc"
    for n in (a.input, a.out):
        if not n or n in (".", "..") or "/" in n or os.sep in n:
            ap.error(f"argument --input / --out: invalid value: {n!r} (a folder name under output/)")
    if a.out == a.input:
        ap.error(f"argument --out: {a.out} is the input (the clean-up would overwrite what it reads)")
    if a.out == "final":
        ap.error("argument --out: not final (output/final/ is the live loop's own place)")
    if not MIN_DILATE <= a.dilate <= MAX_DILATE:
        ap.error(f"argument --dilate: {a.dilate}: the box's side is {MIN_DILATE} to {MAX_DILATE}")
    a.parser = ap
    return a


def main(argv: Optional[List[str]] = None) -> int:
    import json
    a = parse_args(argv)
    root = os.path.abspath(a.root)
    from .ensemble import tree_dir, tree_videos
    images = os.path.join(root, "data/DAVIS/JPEGImages/480p")
    videos = tree_videos(root, [a.input], a.videos)
    problems = check_tree(root, a.input, videos, images if a.overlay else None)
    if not problems and not videos:
        problems = [f"no video folders under {tree_dir(root, a.input)}"]
    if problems:
        print("premvos_amd.components: the tree cannot be cleaned:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print(f"premvos_amd.components: {len(videos)} videos of output/{a.input} have their PNGs, in one size each"
              + (", and their frames" if a.overlay else ""))
        return 0
    from . import _lib, io_pipeline as iop, track
    from .merge_out import remove_stale, summarise
    _lib.require_gpu()
    lay = dict(track._layout(root), out=tree_dir(root, a.out) + "/")
    eval_dir = os.path.join(root, "output", "eval_" + a.out) if a.eval else None
    overlay_dir = os.path.join(root, "output", "overlay_" + a.out) + "/" if a.overlay else None
    remove_stale(eval_dir, videos)
    per_video = {}
    with iop.Writer() as writer:
        for video in videos:
            per_video[video] = clean_video(root, a.input, video, lay, a.dilate, writer, eval_dir, overlay_dir)
    result = {"videos": per_video, "frames": sum(v["frames"] for v in per_video.values()), "dilate": a.dilate, "source": "output/" + a.input}
    fn = os.path.join(root, "output", a.out + ".json")
    with open(fn, "w") as f:
        json.dump(result, f, indent=1)
    gone = sum(sum(sum(row) for row in v["removed"]) for v in per_video.values())
    print(f"premvos_amd.components: videos: {len(videos)}  frames: {result['frames']}  pixels removed: {gone}  ->  {lay['out']}"
          + (f"  {overlay_dir}" if overlay_dir else "") + f"  {fn}")
    if eval_dir is not None:
        summarise(eval_dir, videos, os.path.join(root, "output", f"premvos_amd_davis_eval_{a.out}.json"), f"premvos_amd.components: {a.out}:")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
