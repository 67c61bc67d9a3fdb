"""What the merge loops write per video, in one place: the palette PNGs, the overlay JPEGs (``--overlay``, premvos_amd.overlay) and the
DAVIS count file (``--eval``, premvos_amd.evaluate.LoopEval).  ``track.do_video``, ``track.do_videos_lockstep``,
``stream_track.run_tracker``, ``stream_track.run_prewarp`` and ``prewarp.run_tree`` each make one ``VideoOut`` per video and keep their
own order of jobs; the device work (``overlay.forward``, ``LoopEval.frame`` / ``fetch``) is queued on the caller's current stream, the
files are written on the caller's ``writer``.  Host code: nothing here launches a kernel of its own."""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence


def write_pngs(src, jobs: Sequence, event=None) -> None:
    """On the writer: wait for the id maps' copy, write one PNG per (index, file name) of ``jobs``, give the buffer back.  ``src``: a
    ``track.IdMapSlot`` ([h,w]: index None; a group's [seats,h,w]) or a host uint8 [N,h,w] tensor that is complete after ``event``."""
    from .track import write_png
    try:
        if event is not None:
            event.synchronize()
        maps = src.wait() if hasattr(src, "wait") else src.numpy()
        for i, fn in jobs:
            write_png(fn, maps if i is None else maps[i])
    finally:
        if hasattr(src, "release"):
            src.release()


class VideoOut:
    """One video's output files.  ``png_root`` / ``overlay_dir``: <root>/<video>/<stem>.png / .jpg; ``eval_dir``: <eval_dir>/<video>.json
    from the annotations under ``anns``/<video>; ``evaluated``: receives the video's name when its count file is queued; ``program``:
    who speaks in the log.  ``evaluator`` (after ``open``) is what goes into ``Tracker.evaluator`` / ``Seat.evaluator``."""

    def __init__(self, video: str, png_root: str, writer, device, anns: Optional[str] = None, eval_dir: Optional[str] = None,
                 overlay_dir: Optional[str] = None, evaluated: Optional[List[str]] = None, program: str = "premvos_amd.track"):
        self.video, self.png_root, self.writer, self.device = video, png_root, writer, device
        self.anns, self.eval_dir, self.overlay_dir, self.evaluated, self.program = anns, eval_dir, overlay_dir, evaluated, program
        self.evaluator = None

    def png_path(self, stem: str) -> str:
        return os.path.join(self.png_root, self.video, stem + ".png")

    def jpg_path(self, stem: str, root: Optional[str] = None) -> str:
        from .overlay import jpg_path
        return jpg_path(self.overlay_dir if root is None else root, self.video, stem)

    def open(self, templates) -> Optional[object]:
        """Once per video, when it is known whether it has templates -> the evaluator or None."""
        if self.eval_dir is not None and templates:
            from .evaluate import LoopEval
            self.evaluator = LoopEval.open(self.video, os.path.join(self.anns, self.video), self.device)
        elif self.eval_dir is not None:
            print(f"{self.program}: {self.video}: no templates, not evaluated")
        return self.evaluator

    def expect(self, stem: str) -> None:
        if self.evaluator is not None:
            self.evaluator.expect(stem)

    def close(self) -> None:
        """After the video's last frame, on the stream that painted it: the writer waits for the counts, once per video."""
        if self.evaluator is not None:
            self.writer.submit(self.evaluator.fetch().dump, self.eval_dir)
            if self.evaluated is not None:
                self.evaluated.append(self.video)
            self.evaluator = None

    def overlay(self, stem: str, frame, idmap) -> None:
        """``--overlay``: ``frame`` (a file name, a host array, a CUDA tensor) tinted by ``idmap`` (uint8 [h,w] in HBM; None: no object)."""
        if self.overlay_dir is None:
            return
        from . import _lib, jpeg, overlay
        dev = _lib.resolve_device(self.device)
        frame = jpeg.imread(frame, dev) if isinstance(frame, str) else jpeg.to_device(frame, dev)
        self.writer.submit(overlay.write_jpg, self.jpg_path(stem), overlay.forward(frame, idmap))

    def png(self, stem: str, idmap) -> None:
        from .track import write_png
        self.writer.submit(write_png, self.png_path(stem), idmap)

    def pngs(self, src, pairs: Sequence, event=None) -> None:
        """``write_pngs`` for frames of this video: ``pairs`` = (index into ``src``, stem); one ``IdMapSlot`` of one frame: [(None, stem)]."""
        self.writer.submit(write_pngs, src, [(i, self.png_path(stem)) for i, stem in pairs], event)

    def blank(self, stem: str, frame, size=None):
        """A frame of a video without templates: an all-zero PNG of the frame's size, the plain frame as its overlay -> the zero map."""
        import numpy as np
        if size is None:
            from .track import _image_size
            size = _image_size(frame) if isinstance(frame, str) else tuple(frame.shape[:2])
        zeros = np.zeros(size, np.uint8)
        self.png(stem, zeros)
        self.overlay(stem, frame, None)
        return zeros

    def whole_video(self, image_fns: Sequence[str], res) -> None:
        """A video that was merged at once (``prewarp.merge_video``'s result: "idmap" page-locked [N,h,w], "ready" its event or None,
        "idmap_dev" the same in HBM or None = no templates): frame by frame what the live loop does after each paint."""
        maps, stems = res["idmap_dev"], [os.path.splitext(os.path.basename(fn))[0] for fn in image_fns]
        self.pngs(res["idmap"], list(enumerate(stems)), res["ready"])
        ev = self.open(maps is not None)
        if ev is not None:
            for k, stem in enumerate(stems):
                ev.expect(stem)
                ev.frame(maps[k])
        self.close()
        for k, stem in enumerate(stems):
            self.overlay(stem, image_fns[k], maps[k] if maps is not None else None)


def remove_stale(eval_dir: Optional[str], videos: Sequence[str]) -> None:
    """An earlier run's count files of ``videos``: the summary is of THIS run's videos."""
    for v in videos if eval_dir is not None else ():
        fn = os.path.join(eval_dir, v + ".json")
        if os.path.isfile(fn):
            os.remove(fn)


def summarise(eval_dir: str, videos: Sequence[str], summary_fn: str, prefix: str, indent: Optional[int] = 1) -> None:
    """``evaluate.summarise`` of the ``videos`` that have a count file -> ``summary_fn``, and the J / F / J&F line behind ``prefix``."""
    from . import evaluate as ev
    scored = [v for v in videos if os.path.isfile(os.path.join(eval_dir, v + ".json"))]
    if not scored:
        return
    r = ev.summarise(eval_dir, scored)
    os.makedirs(os.path.dirname(summary_fn) or ".", exist_ok=True)
    with open(summary_fn, "w") as f:
        json.dump(r, f, indent=indent)
    print(f"{prefix} J {r['mean_J']}  F {r['mean_F']}  J&F {r['mean_JF_percent']}  ->  {summary_fn}")
