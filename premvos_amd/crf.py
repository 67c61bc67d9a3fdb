"""Boundary refinement of id maps that already exist: the fully connected CRF of ReID_net/scripts/postproc/crf/crf_davis.py:43-60
(``apply_crf``: a Gaussian and a bilateral kernel, 12 mean-field rounds, argmax) over any tree of palette PNGs this package wrote, with
both filters computed exactly over a truncated window on the GPU (csrc/crf_ops.hip) instead of on pydensecrf's lattice:

    python -m premvos_amd.crf --root <PReMVOS root> --input final [--out final_crf] [--params TEXT] [--eval] [--overlay] [--videos a,b]
                              [--check-only]
        output/<input>/<video>/<frame>.png + data/DAVIS/JPEGImages/480p/<video>/<frame>.jpg
                                   ->  output/<out>/<video>/<frame>.png, output/<out>.json
                                   [--eval]      output/eval_<out>/<video>.json, output/premvos_amd_davis_eval_<out>.json
                                   [--overlay]   output/overlay_<out>/<video>/<frame>.jpg

``--params``: any of ``sxy=22.4,srgb=7.7,compat=1.4,gsxy=0.22,gcompat=1.25,r=56,gr=1,iters=12,gt_prob=0.7`` (the bilateral kernel's
sigmas and weight, the Gaussian kernel's, the two window radii, the rounds, the probability the unary gives a pixel's own label); what
is not given keeps crf_davis.py's value, a radius that is not given is ceil(2.5 sigma).  Per video the PNGs are decoded on the io pool,
the frames come through ``jpeg.imread``, L = 1 + the largest id of the video (at most 16 labels; a video of background alone is copied),
``refine_idmaps`` runs the frames in chunks and ``merge_out.VideoOut.whole_video`` writes the files, as for every other merge.
``--check-only`` names every PNG without a frame, frame without a PNG and size that differs, and needs no GPU.

As a library: ``meanfield(frames, unary, params)`` for any unary (a caller with soft probabilities passes ``-log(clamp(p))``) and
``refine_idmaps(frames, idmaps, L, params)`` for id maps."""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Dict, List, Optional

MIN_LABELS, MAX_LABELS, MAX_RADIUS, MAX_ITERS = 2, 16, 64, 1000               # (csrc/crf_ops.hip refuses the same)
CHUNK_BYTES = 1 << 30                                                         # refine_idmaps: U and two Q of a chunk stay below this


@dataclasses.dataclass(frozen=True)
class Params:
    """The CRF's numbers; the defaults are crf_davis.py:43-60's, ``r`` / ``gr`` = None: ceil(2.5 sigma) (``gr`` at least 1)."""
    sxy: float = 22.3761305044
    srgb: float = 7.70254062277
    compat: float = 1.40326787165
    gsxy: float = 0.220880737269
    gcompat: float = 1.24845093352
    r: Optional[int] = None
    gr: Optional[int] = None
    iters: int = 12
    gt_prob: float = 0.7

    def __post_init__(self):
        def bad(key, why):
            raise ValueError(f"crf parameter {key}={getattr(self, key)!r}: {why}")
        for key in ("sxy", "srgb", "gsxy"):
            if not (isinstance(getattr(self, key), (int, float)) and math.isfinite(getattr(self, key)) and getattr(self, key) > 0):
                bad(key, "a sigma is a positive number")
        for key in ("compat", "gcompat"):
            if not (isinstance(getattr(self, key), (int, float)) and math.isfinite(getattr(self, key)) and getattr(self, key) >= 0):
                bad(key, "a weight is a number >= 0")
        if self.r is None:
            object.__setattr__(self, "r", math.ceil(2.5 * self.sxy))
        if self.gr is None:
            object.__setattr__(self, "gr", max(1, math.ceil(2.5 * self.gsxy)))
        for key in ("r", "gr"):
            if not (isinstance(getattr(self, key), int) and 0 <= getattr(self, key) <= MAX_RADIUS):
                bad(key, f"a window radius is an integer from 0 to {MAX_RADIUS}")
        if not (isinstance(self.iters, int) and 0 <= self.iters <= MAX_ITERS):
            bad("iters", f"an integer from 0 to {MAX_ITERS}")
        if not (isinstance(self.gt_prob, (int, float)) and 0.0 < self.gt_prob < 1.0):
            bad("gt_prob", "inside (0, 1)")

    @classmethod
    def parse(cls, text: Optional[str]) -> "Params":
        """``"key=value,..."`` with any subset of the keys (None or "": the defaults); an unknown key, a value that is no number or one out
        of range raises ValueError naming the key."""
        kinds = {f.name: (int if f.name in ("r", "gr", "iters") else float) for f in dataclasses.fields(cls)}
        given: Dict[str, object] = {}
        for item in (text or "").split(","):
            if not item.strip():
                if (text or "").strip():
                    raise ValueError(f"crf parameters {text!r}: an empty item (key=value, comma-separated)")
                continue
            key, eq, value = (s.strip() for s in item.partition("="))
            if key not in kinds:
                raise ValueError(f"crf parameter {key!r}: unknown (one of {', '.join(kinds)})")
            if key in given:
                raise ValueError(f"crf parameter {key}: given twice")
            try:
                given[key] = kinds[key](value) if eq else kinds[key]("")
            except ValueError:
                raise ValueError(f"crf parameter {key}={value!r}: not " + ("an integer" if kinds[key] is int else "a number")) from None
        return cls(**given)

    def as_dict(self) -> Dict[str, object]:
        return dataclasses.asdict(self)

    def __str__(self) -> str:
        return ",".join(f"{k}={v!r}" for k, v in self.as_dict().items())


def _frames4(frames):
    import torch
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4) and frames.shape[-1] == 3, (frames.dtype, frames.shape)
    return (frames if frames.dim() == 4 else frames[None]).contiguous()


def normalisers(frames, params: Params):
    """uint8 [N,H,W,3] (CUDA) -> (n_g, n_b) float32 [N,H,W]: the Gaussian and the bilateral kernel's n(i), one launch each."""
    import torch
    from . import _lib
    N, H, W = frames.shape[:3]
    n_g, n_b = (torch.empty((N, H, W), dtype=torch.float32, device=frames.device) for _ in range(2))
    lib, s = _lib.load(), _lib.current_stream()
    _lib.check(lib.premvos_crf_norm_f32(frames.data_ptr(), N, H, W, params.gsxy, 0.0, params.gr, n_g.data_ptr(), s), "crf_norm")
    _lib.check(lib.premvos_crf_norm_f32(frames.data_ptr(), N, H, W, params.sxy, params.srgb, params.r, n_b.data_ptr(), s), "crf_norm")
    return n_g, n_b


def _step(frames, unary, q_in, n_g, n_b, params: Params, q_out) -> None:
    from . import _lib
    N, L, H, W = unary.shape
    _lib.check(_lib.load().premvos_crf_step_f32(frames.data_ptr(), unary.data_ptr(), None if q_in is None else q_in.data_ptr(), n_g.data_ptr(),
                                                n_b.data_ptr(), N, H, W, L, params.gsxy, params.gr, params.gcompat, params.sxy, params.srgb,
                                                params.r, params.compat, q_out.data_ptr(), _lib.current_stream()), "crf_step")


def _rounds(frames, unary, q, spare, n_g, n_b, params: Params):
    """``params.iters`` rounds from ``q``, ping-pong between ``q`` and ``spare`` -> the buffer that holds the last round."""
    for _ in range(params.iters):
        _step(frames, unary, q, n_g, n_b, params, spare)
        q, spare = spare, q
    return q


def meanfield(frames, unary, params: Optional[Params] = None):
    """frames uint8 [N,H,W,3] (or [H,W,3]), unary float32 [N,L,H,W] (or [L,H,W]), both CUDA -> Q float32 of ``unary``'s shape after
    ``params.iters`` rounds from Q^0 = softmax(-unary): 2 + 1 + iters launches on the current stream, two Q buffers."""
    import torch
    from . import _lib
    _lib.require_gpu()
    params = Params() if params is None else params
    f = _frames4(frames)
    assert unary.is_cuda and unary.dtype == torch.float32 and unary.dim() == frames.dim(), (unary.dtype, unary.shape, frames.shape)
    u = (unary if unary.dim() == 4 else unary[None]).contiguous()
    assert u.shape[0] == f.shape[0] and tuple(u.shape[2:]) == tuple(f.shape[1:3]), (u.shape, f.shape)
    n_g, n_b = normalisers(f, params)
    q, spare = torch.empty_like(u), torch.empty_like(u)
    _step(f, u, None, n_g, n_b, params, q)
    q = _rounds(f, u, q, spare, n_g, n_b, params)
    return q if unary.dim() == 4 else q[0]


def unary_from_labels(idmaps, L: int, gt_prob: float):
    """uint8 [N,H,W] (CUDA) -> (U, Q^0) float32 [N,L,H,W]; a label >= L raises and writes nothing.  Waits for the stream (the check)."""
    import torch
    from . import _lib
    N, H, W = idmaps.shape
    u, q0 = (torch.empty((N, L, H, W), dtype=torch.float32, device=idmaps.device) for _ in range(2))
    flag = torch.empty((1,), dtype=torch.int32, device=idmaps.device)
    _lib.check(_lib.load().premvos_crf_unary_labels_f32(idmaps.data_ptr(), N, H, W, L, gt_prob, u.data_ptr(), q0.data_ptr(), flag.data_ptr(),
                                                        _lib.current_stream()), "crf_unary_labels")
    return u, q0


def refine_idmaps(frames, idmaps, L: int, params: Optional[Params] = None, chunk_bytes: int = CHUNK_BYTES):
    """frames uint8 [N,H,W,3], idmaps uint8 [N,H,W] with labels < L (both CUDA) -> {"idmap": uint8 [N,H,W], "changed": int32 [N], the
    pixels per frame whose label changed} (CUDA).  The frames run in chunks whose U and two Q buffers (3 L 4 bytes per pixel) stay below
    ``chunk_bytes``; a frame's result does not depend on its chunk."""
    import torch
    from . import _lib
    _lib.require_gpu()
    params = Params() if params is None else params
    f = _frames4(frames)
    assert idmaps.is_cuda and idmaps.dtype == torch.uint8 and tuple(idmaps.shape) == tuple(f.shape[:3]), (idmaps.dtype, idmaps.shape, f.shape)
    idmaps = idmaps.contiguous()
    N, H, W = idmaps.shape
    out = torch.empty_like(idmaps)
    changed = torch.empty((N,), dtype=torch.int32, device=idmaps.device)
    chunk = max(1, int(chunk_bytes) // (3 * L * 4 * H * W))
    for a in range(0, N, chunk):
        b = min(a + chunk, N)
        u, q = unary_from_labels(idmaps[a:b], L, params.gt_prob)
        n_g, n_b = normalisers(f[a:b], params)
        q = _rounds(f[a:b], u, q, torch.empty_like(q), n_g, n_b, params)
        _lib.check(_lib.load().premvos_crf_argmax_u8(q.data_ptr(), b - a, H, W, L, idmaps[a:b].data_ptr(), out[a:b].data_ptr(),
                                                     changed[a:b].data_ptr(), _lib.current_stream()), "crf_argmax")
    return {"idmap": out, "changed": changed}


# ------------------------------------------------------------------------------------------------------------------- the command
def check_tree(root: str, name: str, videos, images: str) -> List[str]:
    """Pure host -> every PNG of output/<name> without its frame under ``images``, frame without its PNG and size that differs (empty =
    the tree can be refined).  Only headers are read."""
    from PIL import Image
    from .ensemble import tree_dir, tree_frames
    if not os.path.isdir(tree_dir(root, name)):
        return [f"{tree_dir(root, name)} is missing"]
    problems = []
    for video in videos:
        stems = tree_frames(root, name, video)
        if not stems:
            problems.append(f"{video}: no PNGs under {os.path.join(tree_dir(root, name), video)}")
            continue
        d = os.path.join(images, video)
        jpgs = sorted(os.path.splitext(f)[0] for f in os.listdir(d) if f.endswith(".jpg")) if os.path.isdir(d) else []
        problems += [f"{video}/{s}.png: no frame {os.path.join(d, s + '.jpg')}" for s in stems if s not in jpgs]
        problems += [f"{video}/{s}.jpg: no PNG under {os.path.join(tree_dir(root, name), video)}" for s in jpgs if s not in stems]
        sizes = set()
        for s in stems:
            with Image.open(os.path.join(tree_dir(root, name), video, s + ".png")) as im:
                png = (im.size[1], im.size[0])
            sizes.add(png)
            if s in jpgs:
                with Image.open(os.path.join(d, s + ".jpg")) as im:
                    jpg = (im.size[1], im.size[0])
                if jpg != png:
                    problems.append(f"{video}/{s}.png: its size {png} is not the frame's {jpg}")
        if len(sizes) > 1:
            problems.append(f"{video}: its PNGs differ in size ({sorted(sizes)}): one stack holds one size")
    return problems


def refine_video(root: str, name: str, video: str, lay: Dict[str, str], params: Params, writer, eval_dir: Optional[str] = None,
                 overlay_dir: Optional[str] = None) -> Dict[str, object]:
    """One video of the tree: decode, read the frames, ``refine_idmaps``, ``VideoOut.whole_video`` under ``lay["out"]`` -> {"frames", "L",
    "changed" [N]}.  A video of background alone (L = 1) is written as it is, without a launch."""
    import numpy as np
    import torch
    from . import _lib, io_pipeline as iop, jpeg, track
    from .ensemble import read_stack, tree_frames
    from .merge_out import VideoOut
    dev = _lib.resolve_device(None)
    stems = tree_frames(root, name, video)
    maps = read_stack(root, [name], video, stems)[0]
    L = 1 + int(maps.max())
    if L > MAX_LABELS:
        raise _lib.PremvosError(f"{video}: id {L - 1} in output/{name}: the CRF takes ids below {MAX_LABELS}")
    fns = [os.path.join(lay["images"], video, stem + ".jpg") for stem in stems]
    sink = VideoOut(video, lay["out"], writer, dev, lay["anns"], eval_dir, overlay_dir, program="premvos_amd.crf")
    if L < MIN_LABELS:
        sink.whole_video(fns, {"idmap": torch.from_numpy(maps), "ready": None, "idmap_dev": None})
        return {"frames": len(stems), "L": L, "changed": [0] * len(stems)}
    frames = jpeg.stack_frames(iop.prefetch(fns, jpeg.host_stage), dev)
    r = refine_idmaps(frames, torch.from_numpy(maps).to(dev), L, params)
    host, ready = track.stack_to_host(r["idmap"])
    sink.whole_video(fns, {"idmap": host, "ready": ready, "idmap_dev": r["idmap"]})
    return {"frames": len(stems), "L": L, "changed": [int(c) for c in r["changed"].cpu().numpy().astype(np.int64)]}


def parse_args(argv: Optional[List[str]] = None):
    """The command line and its refusals (no file is looked at) -> the namespace; ``crf``: ``--params`` as a ``Params``."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=".")
    ap.add_argument("--input", required=True, help="the tree's name under output/ (final, final_prewarp, final_vote, ...)")
    ap.add_argument("--out", default=None, help="the refined tree's name under output/ (default <input>_crf)")
    ap.add_argument("--params", default=None, metavar="TEXT", help="key=value,... over crf_davis.py's numbers (see above)")
    ap.add_argument("--eval", action="store_true", help="also score the refined maps against data/DAVIS/Annotations/480p on the GPU")
    ap.add_argument("--overlay", action="store_true", help="also write every frame with the refined objects tinted")
    ap.add_argument("--videos", default=None, help="comma-separated video names (default: every folder of the input)")
    ap.add_argument("--check-only", action="store_true", help="name what is missing or differs in size and stop (no GPU)")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = a.input + "_crf"
    for n in (a.input, a.out):
        if not n or n in (".", "..") or "/" in n or os.sep in n:
            ap.error(f"argument --input / --out: invalid value: {n!r} (a folder name under output/)")
    if a.out == a.input:
        ap.error(f"argument --out: {a.out} is the input (the refinement would overwrite what it reads)")
    if a.out == "final":
        ap.error("argument --out: not final (output/final/ is the live loop's own place)")
    try:
        a.crf = Params.parse(a.params)
    except ValueError as e:
        ap.error(f"argument --params: {e}")
    a.parser = ap
    return a


def main(argv: Optional[List[str]] = None) -> int:
    import json
    a = parse_args(argv)
    root = os.path.abspath(a.root)
    from .ensemble import tree_dir, tree_videos
    images = os.path.join(root, "data/DAVIS/JPEGImages/480p")
    videos = tree_videos(root, [a.input], a.videos)
    problems = check_tree(root, a.input, videos, images)
    if not problems and not videos:
        problems = [f"no video folders under {tree_dir(root, a.input)}"]
    if problems:
        print("premvos_amd.crf: the tree cannot be refined:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print(f"premvos_amd.crf: {len(videos)} videos of output/{a.input} have their frames, in their sizes")
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
            per_video[video] = refine_video(root, a.input, video, lay, a.crf, writer, eval_dir, overlay_dir)
    result = {"videos": per_video, "frames": sum(v["frames"] for v in per_video.values()), "params": a.crf.as_dict(), "source": "output/" + a.input}
    fn = os.path.join(root, "output", a.out + ".json")
    with open(fn, "w") as f:
        json.dump(result, f, indent=1)
    moved = sum(sum(v["changed"]) for v in per_video.values())
    print(f"premvos_amd.crf: videos: {len(videos)}  frames: {result['frames']}  pixels relabelled: {moved}  ->  {lay['out']}"
          + (f"  {overlay_dir}" if overlay_dir else "") + f"  {fn}")
    if eval_dir is not None:
        summarise(eval_dir, videos, os.path.join(root, "output", f"premvos_amd_davis_eval_{a.out}.json"), f"premvos_amd.crf: {a.out}:")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
