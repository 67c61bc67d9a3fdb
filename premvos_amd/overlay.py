"""Overlay pictures: every frame with its objects' masks tinted, as a JPEG next to the palette PNG -- the reference's
``draw_mask`` + ``save_jpg`` (MergeTrack/merge_functions.py:527-545).

    python -m premvos_amd.overlay --root <PReMVOS root> [--videos a,b] [--check-only]     ->  output/overlay/<video>/<frame>.jpg

reads data/DAVIS/JPEGImages/480p and output/final; ``premvos_amd.track --overlay`` and ``premvos_amd.stream --track --overlay`` write
the same files from inside the merge loop, where the frame and the id map it just painted are both in HBM.

Per frame: ``premvos_jpeg_forward_u8`` blends (``(frame + palette[id]) >> 1`` where id > 0: draw_mask's ``im * (1 - 0.5) + color * 0.5``
and its ``astype(uint8)``, for all objects at once -- the masks of a final id map do not overlap) while it loads the pixels and leaves
quantised DCT coefficients; they go to a pinned buffer, and a writer thread runs the Huffman pass
(``premvos_jpeg_entropy_encode_host``, plain C, no interpreter lock) and writes the file.  The blended picture never exists as pixels.

Two differences from the reference, both on purpose.  The colours are the DAVIS palette of the PNGs (``track.voc_palette``), so an
object has one colour in both files; the reference's draw_mask takes tensorpack's ``PALETTE_RGB``.  The file is what PIL writes for
the blended picture (quality 95, 4:2:0, libjpeg-turbo's defaults); save_jpg goes through cv2, which is not installed here -- the same
library behind a header of its own.
"""
from __future__ import annotations

import glob
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, jpeg

QUALITY, SUBSAMPLING = 95, "4:2:0"
_PALETTES: Dict[object, torch.Tensor] = {}


def palette(device=None) -> torch.Tensor:
    """``track.voc_palette()`` as a uint8 [256,3] tensor on ``device`` (uploaded once per device)."""
    from .track import voc_palette
    device = _lib.resolve_device(device)
    if device not in _PALETTES:
        _PALETTES[device] = torch.from_numpy(voc_palette()).to(device)
    return _PALETTES[device]


def blend(frame: torch.Tensor, idmap: torch.Tensor, pal: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``premvos_overlay_blend_u8`` on the current stream: frame uint8 [H,W,3], idmap uint8 [H,W], both in HBM -> uint8 [H,W,3]."""
    _lib.require_gpu()
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_cuda:
        raise ValueError("blend() takes a uint8 [H,W,3] frame in HBM")
    if idmap.dtype != torch.uint8 or tuple(idmap.shape) != tuple(frame.shape[:2]) or idmap.device != frame.device:
        raise ValueError("idmap: a uint8 [H,W] tensor on the frame's device")
    pal = palette(frame.device) if pal is None else pal
    frame, idmap = frame.contiguous(), idmap.contiguous()
    with torch.cuda.device(frame.device):
        out = torch.empty_like(frame)
        _lib.check(_lib.load().premvos_overlay_blend_u8(frame.data_ptr(), idmap.data_ptr(), pal.data_ptr(), int(frame.shape[0]),
                                                       int(frame.shape[1]), out.data_ptr(), _lib.current_stream()), "premvos_overlay_blend_u8")
    return out


def forward(frame: torch.Tensor, idmap: Optional[torch.Tensor]) -> jpeg.Encoded:
    """The device half of one overlay picture (current stream): blend fused into the encoder's load.  ``idmap`` None: no object."""
    if idmap is None:
        return jpeg.forward(frame, QUALITY, SUBSAMPLING)
    return jpeg.forward(frame, QUALITY, SUBSAMPLING, idmap=idmap, palette=palette(frame.device))


def write_jpg(filename: str, encoded: jpeg.Encoded) -> None:
    """The host half, for a writer thread: wait for the coefficients, Huffman pass, write the file."""
    data = jpeg.entropy_encode(encoded)
    os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
    with open(filename, "wb") as f:
        f.write(data)


def jpg_path(overlay_root: str, video: str, stem: str) -> str:
    return os.path.join(overlay_root, video, stem + ".jpg")


# ---------------------------------------------------------------------------------------------------------------- command line
def _layout(root: str) -> Dict[str, str]:
    return {"images": os.path.join(root, "data/DAVIS/JPEGImages/480p"), "final": os.path.join(root, "output/final"),
            "overlay": os.path.join(root, "output/overlay")}


def check_inputs(root: str, videos: Optional[List[str]] = None) -> List[str]:
    """-> what ``main`` would miss under ``root`` (empty = ready)."""
    lay = _layout(root)
    problems = [f"{lay[k]} is missing ({why})" for k, why in
                (("images", "the frames"), ("final", "the merge stage's PNGs: run premvos_amd.track, or premvos_amd.stream --track, first"))
                if not os.path.isdir(lay[k])]
    if problems:
        return problems
    for v in (_videos(lay) if videos is None else videos):
        if not os.path.isdir(os.path.join(lay["final"], v)):
            problems.append(f"{os.path.join(lay['final'], v)} is missing (no such video among the merge stage's results)")
            continue
        for png in sorted(glob.glob(os.path.join(lay["final"], v, "*.png"))):
            stem = os.path.splitext(os.path.basename(png))[0]
            if not os.path.isfile(os.path.join(lay["images"], v, stem + ".jpg")):
                problems.append(f"{os.path.join(lay['images'], v, stem + '.jpg')} is missing (the frame of {png})")
    return problems


def _videos(lay: Dict[str, str]) -> List[str]:
    return sorted(d for d in os.listdir(lay["final"]) if os.path.isdir(os.path.join(lay["final"], d)))


def do_video(video: str, images: str, final: str, out: str, writer, device=None) -> int:
    """One JPEG under ``out``/``video`` per PNG of ``final``/``video``; the Huffman pass and the file writes run on ``writer``."""
    from PIL import Image
    device = _lib.resolve_device(device)
    n = 0
    for png in sorted(glob.glob(os.path.join(final, video, "*.png"))):
        stem = os.path.splitext(os.path.basename(png))[0]
        frame = jpeg.imread(os.path.join(images, video, stem + ".jpg"), device)
        ids = np.array(Image.open(png))
        if ids.shape != tuple(frame.shape[:2]):
            raise _lib.PremvosError(f"{png} is {ids.shape[1]} x {ids.shape[0]}, its frame {frame.shape[1]} x {frame.shape[0]}")
        writer.submit(write_jpg, jpg_path(out, video, stem), forward(frame, torch.from_numpy(ids.astype(np.uint8)).to(device)))
        n += 1
    return n


def main(argv: Optional[List[str]] = None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=".")
    ap.add_argument("--videos", default=None, help="comma-separated video names (default: every folder of output/final)")
    ap.add_argument("--check-only", action="store_true", help="name what is missing and stop")
    a = ap.parse_args(argv)
    root = os.path.abspath(a.root)
    problems = check_inputs(root, a.videos.split(",") if a.videos else None)
    if problems:
        print("premvos_amd.overlay: inputs are not ready:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print("premvos_amd.overlay: inputs are in place")
        return 0
    _lib.require_gpu()
    from . import io_pipeline as iop
    lay = _layout(root)
    videos = a.videos.split(",") if a.videos else _videos(lay)
    frames = 0
    with iop.Writer() as writer:
        for v in videos:
            frames += do_video(v, lay["images"], lay["final"], lay["overlay"], writer)
    print(f"premvos_amd.overlay: videos: {len(videos)}  frames: {frames}  ->  {lay['overlay']}/")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
