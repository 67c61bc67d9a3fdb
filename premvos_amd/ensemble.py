"""The per-pixel vote over PNG trees that already exist: the combination step behind MergeTrack/oldmerge.py:129-131,220-224, whose runs
write one tree per weight set under to_ensemble/<n>/.  Any trees of palette PNGs vote -- for example the different merges this package
writes (output/final, final_prewarp, final_prob, final_weights, final_oracle):

    python -m premvos_amd.ensemble --root <PReMVOS root> --inputs final,final_prewarp,final_prob [--out final_vote] [--eval] [--overlay]
                                   [--videos a,b] [--check-only]
        output/<input>/<video>/<frame>.png  ->  output/<out>/<video>/<frame>.png, output/<out>.json
                                   [--eval]      output/eval_<out>/<video>.json, output/premvos_amd_davis_eval_<out>.json
                                   [--overlay]   output/overlay_<out>/<video>/<frame>.jpg

The list order is the vote's priority: the label most inputs painted wins a pixel, on a tie the input listed first.  Per video the PNGs
are decoded on the host and uploaded as one [K,N,h,w] stack (K * N * h * w bytes of HBM), ONE premvos_idmap_vote_u8 launch votes it
(``track.vote_idmaps``), and ``merge_out.VideoOut.whole_video`` writes the files, as for every other merge.  ``--check-only`` names every
video, frame or size that is not the same in all inputs and needs no GPU.  The tracking modes' own votes are ``track --ensemble``."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import numpy as np

MIN_INPUTS, MAX_INPUTS = 2, 8                                                 # (premvos_idmap_vote_u8 takes 1 .. 8 sets)


def tree_dir(root: str, name: str) -> str:
    return os.path.join(root, "output", name)


def tree_frames(root: str, name: str, video: str) -> List[str]:
    """The stems of output/<name>/<video>/*.png, sorted."""
    d = os.path.join(tree_dir(root, name), video)
    return sorted(os.path.splitext(f)[0] for f in os.listdir(d) if f.endswith(".png")) if os.path.isdir(d) else []


def tree_videos(root: str, inputs: Sequence[str], only: Optional[str] = None) -> List[str]:
    """The videos of ANY input, sorted (one that an input lacks is a difference ``check_trees`` names); ``only``: comma-separated names."""
    seen = set()
    for name in inputs:
        d = tree_dir(root, name)
        if os.path.isdir(d):
            seen.update(v for v in os.listdir(d) if os.path.isdir(os.path.join(d, v)))
    return sorted(v for v in seen if not only or v in only.split(","))


def check_trees(root: str, inputs: Sequence[str], videos: Sequence[str]) -> List[str]:
    """Pure host -> every video, frame or frame size that is not the same in all ``inputs`` (empty = the trees can vote).  Only the PNG
    headers are read."""
    from PIL import Image
    problems = [f"{tree_dir(root, name)} is missing" for name in inputs if not os.path.isdir(tree_dir(root, name))]
    if problems:
        return problems
    for video in videos:
        frames = {name: tree_frames(root, name, video) for name in inputs}
        lacking = [name for name in inputs if not frames[name]]
        if lacking:
            problems += [f"{video}: no PNGs under {os.path.join(tree_dir(root, name), video)}" for name in lacking]
            continue
        every, video_sizes = sorted(set().union(*frames.values())), set()
        for stem in every:
            have = [name for name in inputs if stem in frames[name]]
            if len(have) != len(inputs):
                problems.append(f"{video}/{stem}.png: missing in " + ", ".join(n for n in inputs if n not in have))
                continue
            sizes = {}
            for name in inputs:
                with Image.open(os.path.join(tree_dir(root, name), video, stem + ".png")) as im:
                    sizes[name] = (im.size[1], im.size[0])
            video_sizes.add(sizes[inputs[0]])
            if len(set(sizes.values())) > 1:
                problems.append(f"{video}/{stem}.png: sizes differ: " + ", ".join(f"{n} {sizes[n]}" for n in inputs))
        if len(video_sizes) > 1:
            problems.append(f"{video}: its frames differ in size ({sorted(video_sizes)}): one stack holds one size")
    return problems


def read_stack(root: str, inputs: Sequence[str], video: str, stems: Sequence[str]) -> np.ndarray:
    """The id maps of ``video`` in every input -> uint8 [K,N,h,w] (host), decoded ahead on the io pool."""
    from . import io_pipeline as iop
    from .evaluate import _read_ids
    jobs = [os.path.join(tree_dir(root, name), video, stem + ".png") for name in inputs for stem in stems]
    maps = list(iop.prefetch(jobs, _read_ids))
    return np.ascontiguousarray(np.array(maps, np.uint8).reshape((len(inputs), len(stems)) + maps[0].shape))


def vote_video(root: str, inputs: Sequence[str], video: str, lay: Dict[str, str], writer, eval_dir: Optional[str] = None,
               overlay_dir: Optional[str] = None, record: bool = False) -> Dict[str, object]:
    """One video of the trees: decode, upload, ONE vote, ``VideoOut.whole_video`` under ``lay["out"]`` -> {"frames", "hist"} and, with
    ``record``, "voted" uint8 [N,h,w] (host)."""
    import torch
    from . import _lib, track
    from .merge_out import VideoOut
    dev = _lib.resolve_device(None)
    stems = tree_frames(root, inputs[0], video)
    members = torch.from_numpy(read_stack(root, inputs, video, stems)).to(dev)
    v = track.vote_idmaps(members)
    host, ready = track.stack_to_host(v["voted"])
    fns = [os.path.join(lay["images"], video, stem + ".jpg") for stem in stems]
    VideoOut(video, lay["out"], writer, dev, lay["anns"], eval_dir, overlay_dir, program="premvos_amd.ensemble").whole_video(
        fns, {"idmap": host, "ready": ready, "idmap_dev": v["voted"]})
    out: Dict[str, object] = {"frames": len(stems), "hist": v["hist"].cpu().numpy()}
    if record:
        out["voted"] = v["voted"].cpu().numpy()
    return out


def parse_args(argv: Optional[List[str]] = None):
    """The command line and its refusals (no file is looked at) -> the namespace; ``names``: ``--inputs`` as a list."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=".")
    ap.add_argument("--inputs", required=True, metavar="a,b,c",
                    help=f"{MIN_INPUTS} to {MAX_INPUTS} tree names under output/, comma-separated; the order is the vote's priority")
    ap.add_argument("--out", default="final_vote", help="the voted tree's name under output/ (default final_vote)")
    ap.add_argument("--eval", action="store_true", help="also score the voted maps against data/DAVIS/Annotations/480p on the GPU")
    ap.add_argument("--overlay", action="store_true", help="also write every frame of data/DAVIS/JPEGImages/480p with the voted objects tinted")
    ap.add_argument("--videos", default=None, help="comma-separated video names (default: every folder of the inputs)")
    ap.add_argument("--check-only", action="store_true", help="name what differs between the inputs and stop (no GPU)")
    a = ap.parse_args(argv)
    a.names = a.inputs.split(",")
    if not MIN_INPUTS <= len(a.names) <= MAX_INPUTS:
        ap.error(f"argument --inputs: {len(a.names)} trees ({MIN_INPUTS} to {MAX_INPUTS} names, comma-separated)")
    for n in a.names + [a.out]:
        if not n or n in (".", "..") or "/" in n or os.sep in n:
            ap.error(f"argument --inputs / --out: invalid value: {n!r} (a folder name under output/)")
    if len(set(a.names)) != len(a.names):
        ap.error("argument --inputs: a tree is listed twice (it would vote twice)")
    if a.out in a.names:
        ap.error(f"argument --out: {a.out} is an input (the vote would overwrite what it reads)")
    if a.out == "final":
        ap.error("argument --out: not final (output/final/ is the live loop's own place)")
    a.parser = ap
    return a


def main(argv: Optional[List[str]] = None) -> int:
    a = parse_args(argv)
    root = os.path.abspath(a.root)
    videos = tree_videos(root, a.names, a.videos)
    problems = check_trees(root, a.names, videos)
    if not problems and not videos:
        problems = [f"no video folders under {', '.join(tree_dir(root, n) for n in a.names)}"]
    if problems:
        print("premvos_amd.ensemble: the inputs differ:\n  " + "\n  ".join(problems))
        return 2
    if a.check_only:
        print(f"premvos_amd.ensemble: {len(a.names)} trees of {len(videos)} videos agree in videos, frames and sizes")
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
            per_video[video] = vote_video(root, a.names, video, lay, writer, eval_dir, overlay_dir)
    result = track.ensemble_result(per_video, len(a.names), None, ["output/" + n for n in a.names])
    track.write_ensemble_json(os.path.join(root, "output", a.out + ".json"), result)
    print(f"premvos_amd.ensemble: videos: {len(videos)}  frames: {result['frames']}  trees: {len(a.names)}  ->  {lay['out']}"
          + (f"  {overlay_dir}" if overlay_dir else "") + f"  {os.path.join(root, 'output', a.out + '.json')}")
    if eval_dir is not None:
        summarise(eval_dir, videos, os.path.join(root, "output", f"premvos_amd_davis_eval_{a.out}.json"), f"premvos_amd.ensemble: {a.out}:")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
