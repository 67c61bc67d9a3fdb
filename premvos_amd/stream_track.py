"""``python -m premvos_amd.stream --track``: the merge loop of premvos_amd.track inside the streaming driver, on the arrays the
stage threads have in HBM -- the refined masks, their ReID rows, the flow fields, the decoded frames -- instead of the files the
two-program path (``stream --reid``, then ``track``) writes and reads back.

Two parts:

  * ``TrackFeed`` -- host logic only (tests/test_cpu_stream_track.py drives it with fake payloads).  The producer thread opens a
    chunk per ``iter_chunks`` item, in frame order (``open_chunk``: blocks while ``capacity`` chunks are open -- the feed's bound);
    the flow thread and the refinement lanes attach their parts whenever they finish (``put_masks`` per launch, ``part_done``
    per chunk: out of order across chunks, two lanes); the tracker thread takes the chunks back in the order they were opened, each
    once BOTH parts are there (``chunks`` / ``frames``), and thereby closes them.  ``fail`` (any thread) wakes everybody: a waiting
    producer gets ``FeedClosed``, the consumer's iteration ends with it.
  * ``ChunkStore`` / ``run_tracker`` -- the device side: per chunk ONE uint8 store [sum over its frames of (T + F_k), H, W] in
    which frame k's F_k fresh masks sit behind T free slots (T = the video's objects), so that the tracker's mask stack of frame
    k -- candidates, then fresh proposals -- is a contiguous slice and ``Tracker.step_resident`` of frame k - 1 writes the refined
    candidates straight into it; the [F,132] ReID rows and the float64 scores of the chunk beside it; the flow block.  Each part
    is copied on its producer's stream and carries an event the tracker's stream waits on.

``run_prewarp`` is the tracker thread's other body (``--track --prewarp``): the same feed and stores (laid out without free slots), but
the chunks go to a ``prewarp.VideoIngest`` and a video is merged at its end by the pre-warp merge -- no network runs per frame.

What stays on the host, and why: the first-frame annotation (``read_ann``: a PNG, once per video) and its templates' embedding
through the file (``add_ReID``, as ``do_video``); the proposals' scores, which are taken from the dicts that are dumped into
ReID_proposals/ (Python floats: what ``read_props`` would parse) and uploaded once per chunk; PNG encoding, on the writer thread,
which waits for the id map's event -- the tracker thread does not.
"""
from __future__ import annotations

import collections
import os
import threading
from typing import Dict, Iterator, List, Optional, Tuple


class FeedClosed(RuntimeError):
    """The feed was failed (``TrackFeed.fail``) while this thread was waiting on it."""


class Chunk:
    """One ``iter_chunks`` item on its way to the tracker.  ``payload``: whatever the producer attached (the driver: video name,
    image files, decoded frames, next frame, templates); ``pieces[k]``: (first slot, count) per ``put_masks`` call of
    frame k; ``parts``: what ``part_done`` attached."""

    def __init__(self, index: int, video: str, names: List[str], first: bool, payload: Dict[str, object]):
        self.index, self.video, self.names, self.first, self.payload = index, video, list(names), first, payload
        self.pieces: List[List[tuple]] = [[] for _ in names]
        self.parts: Dict[str, object] = {}
        self.left = {"flow", "refine"}


Frame = collections.namedtuple("Frame", "chunk k name pieces")


class TrackFeed:
    def __init__(self, capacity: int = 4, poll: float = 0.2):
        assert capacity >= 1
        self.capacity, self.poll = capacity, poll
        self._cv = threading.Condition()
        self._open: "collections.deque[Chunk]" = collections.deque()
        self._by_key: Dict[int, Chunk] = {}
        self._n = 0
        self._ended = False
        self._error: Optional[BaseException] = None
        self._video: Optional[str] = None
        self.waited_s = 0.0                        # how long the producer stood in front of a full feed

    # ---- producer --------------------------------------------------------------------------------------------------------------
    def open_chunk(self, video: str, names: List[str], key: object = None, **payload) -> Chunk:
        """In frame order.  ``key``: an object the stage threads hold too (the chunk's frame list): ``lookup(key)`` finds the chunk."""
        import time
        with self._cv:
            t0 = time.perf_counter()
            while len(self._open) >= self.capacity and self._error is None:
                self._cv.wait(self.poll)
            self.waited_s += time.perf_counter() - t0
            if self._error is not None:
                raise FeedClosed("the tracker stopped") from self._error
            ch = Chunk(self._n, video, names, video != self._video, payload)
            self._n += 1
            self._video = video
            self._open.append(ch)
            if key is not None:
                ch.key = key                       # (kept alive: ids are unique only among live objects)
                self._by_key[id(key)] = ch
            self._cv.notify_all()
            return ch

    def end(self) -> None:
        """No more chunks: the consumer's iteration ends after the open ones."""
        with self._cv:
            self._ended = True
            self._cv.notify_all()

    # ---- stage threads ---------------------------------------------------------------------------------------------------------
    def lookup(self, key: object) -> Chunk:
        with self._cv:
            return self._by_key[id(key)]

    def put_masks(self, chunk: Chunk, k: int, first_slot: int, count: int) -> None:
        """One launch's share of frame ``k``: ``count`` proposals from slot ``first_slot`` on (a frame with more proposals than a
        launch holds arrives in several calls; a frame without proposals in none)."""
        with self._cv:
            chunk.pieces[k].append((first_slot, count))

    def part_done(self, chunk: Chunk, part: str, value: object = None) -> None:
        with self._cv:
            chunk.parts[part] = value
            chunk.left.discard(part)
            self._cv.notify_all()

    def fail(self, error: BaseException) -> None:
        with self._cv:
            if self._error is None:
                self._error = error
            self._cv.notify_all()

    # ---- consumer --------------------------------------------------------------------------------------------------------------
    def chunks(self) -> Iterator[Chunk]:
        """The chunks in the order they were opened, each when its flow and refinement parts are there; a chunk is closed (its
        place in the feed free again) when the consumer asks for the next one."""
        while True:
            with self._cv:
                while self._error is None and not (self._open and not self._open[0].left) and not (self._ended and not self._open):
                    self._cv.wait(self.poll)
                if self._error is not None:
                    raise FeedClosed("the feed was stopped") from self._error
                if not self._open:
                    return
                ch = self._open[0]
            yield ch
            with self._cv:
                self._open.popleft()
                self._by_key.pop(id(getattr(ch, "key", None)), None)
                self._cv.notify_all()

    def frames(self) -> Iterator[Frame]:
        """One frame at a time, in frame order; ``pieces`` sorted by slot."""
        for ch in self.chunks():
            for k, name in enumerate(ch.names):
                yield Frame(ch, k, name, sorted(ch.pieces[k], key=lambda p: p[0]))


def store_bytes(chunk: int, proposals: int, objects: int, h: int, w: int) -> int:
    """Device bytes one open chunk holds for the tracker: masks (objects + proposals per frame), ReID rows, scores, flow."""
    return chunk * ((objects + proposals) * h * w + proposals * (132 * 4 + 8) + h * w * 2 * 4)


# ------------------------------------------------------------------------------------------------------------------ device side
class ChunkStore:
    """The tracker-owned copy of one chunk's refinement results (see the module text).  Made on a refinement lane's thread and
    stream; ``counts[k]`` = proposals of frame k, ``T`` = free slots in front of each frame's block."""

    def __init__(self, counts: List[int], T: int, h: int, w: int, device, reader_stream):
        import torch
        self.counts, self.T = list(counts), T
        self.offs, self.roffs = [], []
        o = r = 0
        for c in self.counts:
            self.offs.append(o)
            self.roffs.append(r)
            o += T + c
            r += c
        self.masks = torch.empty((max(o, 1), h, w), dtype=torch.uint8, device=device)
        self.rows = torch.empty((max(r, 1), 132), dtype=torch.float32, device=device)
        self.scores = None
        self.event = None
        for t in (self.masks, self.rows):           # allocated on the lane's stream, read (and, the free slots, written) on the tracker's
            t.record_stream(reader_stream)
        self._reader = reader_stream

    def put(self, k: int, i0: int, masks, rows) -> None:
        n = masks.shape[0]
        assert i0 + n <= self.counts[k]
        self.masks[self.offs[k] + self.T + i0: self.offs[k] + self.T + i0 + n].copy_(masks)
        self.rows[self.roffs[k] + i0: self.roffs[k] + i0 + n].copy_(rows)

    def close(self, scores: List[List[float]], stream) -> None:
        """``scores``: per frame the Python floats of its proposals' "score"; records the event behind every copy."""
        import torch
        flat = [float(s) for fr in scores for s in fr]
        assert [len(fr) for fr in scores] == self.counts
        self.scores = torch.tensor(flat or [0.0], dtype=torch.float64).to(self.masks.device, non_blocking=True)
        self.scores.record_stream(self._reader)
        self.event = torch.cuda.Event()
        self.event.record(stream)

    def frame(self, k: int) -> Tuple[object, object, object, object, object]:
        """-> (stack [T + F], fresh [F] or None, rows, scores, the NEXT frame's free slots [T] or None at the chunk's end)."""
        T, F, o, r = self.T, self.counts[k], self.offs[k], self.roffs[k]
        stack = self.masks[o:o + T + F]
        nxt = self.masks[self.offs[k + 1]:self.offs[k + 1] + T] if k + 1 < len(self.counts) else None
        if F == 0:
            return stack, None, None, None, nxt
        return stack, stack[T:], self.rows[r:r + F], self.scores[r:r + F], nxt


def run_prewarp(feed: TrackFeed, ReID_net, final_dir: str, writer, stream, device, weights=None, anns: Optional[str] = None,
                eval_dir: Optional[str] = None, overlay_dir: Optional[str] = None, evaluated: Optional[List[str]] = None,
                stats: Optional[Dict[str, float]] = None, negatives=None) -> int:
    """``--track --prewarp``: the tracker thread's body for the pre-warp merge (premvos_amd.prewarp) instead of the live-warp loop.  No
    network runs per frame: every chunk of the feed is handed to its video's ``prewarp.VideoIngest`` on ``stream`` (one fused warp +
    bit-pack launch, one that widens the embeddings; the chunk's byte masks are not kept), and at a video's end -- the next chunk is
    another video's, or the feed ends -- the whole video is merged: ``finish()``, ``prepare()``, ``chain()``, ``paint()``, ONE copy of
    its id maps into page-locked memory with an event, and the PNG job on the writer, which waits for the event; this
    thread does not.  Only the annotated objects' embedding takes the host route (``add_ReID`` on ``ReID_net``, once per video, as
    ``prewarp.read_video``).  A video without templates gets all-zero PNGs and copies nothing.  ``eval_dir`` / ``overlay_dir`` /
    ``evaluated``: as ``run_tracker``'s (``merge_out.VideoOut.whole_video``, as ``track --prewarp``).  ``stats``: receives "waited_s"
    (this thread in front of an empty feed) and "videos".  ``negatives`` (``--negatives [K]``: "all" or a cap): ``finish(negatives)``
    adds the video's negative first-frame templates, as ``track --prewarp --negatives``; ``stats`` then also receives "negatives"
    (``run_tree``'s entry of output/prewarp_negatives.json per video).  Returns the number of frames."""
    import time
    import numpy as np
    import torch
    from . import prewarp as pw
    from .merge_out import VideoOut
    from .reid.driver import add_ReID
    wts = pw.normalised(weights)
    n_frames, waited, videos, taken = 0, 0.0, 0, {}
    cur: Optional[Dict[str, object]] = None          # the video being ingested

    def close_video():
        nonlocal videos
        if cur is None:
            return
        videos += 1
        name, fns, ing = cur["video"], cur["image_fns"], cur["ingest"]
        h, w = cur["size"]
        if ing is None:
            res = {"idmap": torch.zeros((len(fns), h, w), dtype=torch.uint8), "ready": None, "idmap_dev": None}
        else:
            dv = ing.finish(negatives)
            assert dv.tab.N == len(fns)
            if negatives is not None:
                score0 = dv.score[:int(dv.tab.poff[1])].cpu().numpy()
                taken[name] = {"candidates": len(score0), "taken": list(dv.negatives), "scores": [float(score0[i]) for i in dv.negatives],
                               "templates": dv.tab.T}
            dv.prepare()
            c = dv.chain(wts[None])
            idmap, _ = dv.paint(c["chosen"], c["best"])
            host = torch.empty((len(fns), h, w), dtype=torch.uint8, pin_memory=True)
            host.copy_(idmap, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(stream)
            res = {"idmap": host, "ready": ready, "idmap_dev": idmap}
        VideoOut(name, final_dir, writer, device, anns, eval_dir, overlay_dir, evaluated).whole_video(fns, res)

    with torch.cuda.stream(stream):
        it = feed.chunks()
        while True:
            t0 = time.perf_counter()
            ch = next(it, None)                                   # (asking for the next chunk frees the last one's place in the feed)
            waited += time.perf_counter() - t0
            if ch is None:
                break
            pl = ch.payload
            store: Optional[ChunkStore] = ch.parts.get("refine")
            flow = ch.parts.get("flow")
            if ch.first:
                close_video()
                h, w = pl["frames"][0].shape[:2]
                cur = {"video": ch.video, "image_fns": [], "size": (h, w), "ingest": pw.VideoIngest(h, w, device) if pl["T"] else None}
            cur["image_fns"] += list(pl["image_fns"])
            n_frames += len(ch.names)
            ing = cur["ingest"]
            if ing is None:
                continue
            assert store is not None and store.T == 0, "the chunk's store was laid out for the live loop"
            assert tuple(pl["frames"][0].shape[:2]) == cur["size"], f"{ch.video}: the frames differ in size"
            stream.wait_event(store.event)
            if flow is not None:
                stream.wait_event(flow[1])
            if ch.first:                                          # frame 0's objects: masks from the annotation, embedding the host route
                from PIL import Image
                first_fn = pl["image_fns"][0]
                ann = np.array(Image.open(os.path.join(anns, ch.video, os.path.splitext(os.path.basename(first_fn))[0] + ".png")))
                templates = add_ReID(list(pl["templates"]), first_fn, ReID_net)
                ing.add_annotations([{"id": int(t["id"]), "mask": (ann == t["id"]).astype(np.uint8), "reid": np.asarray(t["ReID"], np.float64)}
                                     for t in templates], flow[0][0] if flow is not None and flow[0].shape[0] else None)
            for k, name in enumerate(ch.names):
                got = sum(c for _, c in ch.pieces[k])
                assert got == store.counts[k], f"{ch.video}/{name}: {got} of {store.counts[k]} refined masks reached the tracker"
            ing.add_chunk(store.masks, store.counts, flow[0] if flow is not None else None, store.rows, store.scores)
        close_video()
    if stats is not None:
        stats.update(waited_s=waited, videos=videos, **({"negatives": taken} if negatives is not None else {}))
    return n_frames


def run_tracker(feed: TrackFeed, engines, final_dir: str, writer, stream, device, timer=None, eval_dir: Optional[str] = None,
                anns: Optional[str] = None, evaluated: Optional[List[str]] = None, overlay_dir: Optional[str] = None) -> int:
    """The tracker thread's body: every frame of the feed through ``Tracker.step_resident`` on ``stream``; PNGs go to ``writer``.
    Returns the number of frames.  ``eval_dir`` (with ``anns``, the annotation root): every id map is also scored against the
    video's annotations on ``stream`` (premvos_amd.evaluate.LoopEval: the annotations are read and uploaded once per video, the
    counts come back once per video and the WRITER waits for them); the names of the scored videos are appended to ``evaluated``.
    ``overlay_dir``: every frame also goes out as ``overlay_dir``/<video>/<frame>.jpg with its objects tinted (premvos_amd.overlay):
    the decoded frame and the id map are blended and DCT-coded on ``stream`` right behind the paint, the WRITER runs the Huffman pass."""
    import torch
    from . import jpeg
    from .merge_out import VideoOut
    from .track import Tracker
    n_frames = 0
    tr = sink = None
    with torch.cuda.stream(stream):
        for fr in feed.frames():                                  # one frame at a time, in frame order
            ch, k, name = fr.chunk, fr.k, fr.name
            pl = ch.payload
            frames, n = pl["frames"], len(ch.names)
            if k == 0:                                            # a new chunk: its parts were made on other streams
                if ch.first:
                    if sink is not None:
                        sink.close()
                    tr = Tracker(engines[0], engines[1], device=device)
                    tr.timer = timer
                    tr.ring_alive = lambda: not getattr(writer, "failed", False)
                    if pl.get("templates"):
                        tr.add_templates(pl["templates"], pl["image_fns"][0])
                        tr.pin_idmap_ring(*frames[0].shape[:2])   # page-locked once per video, not in the middle of it
                    sink = VideoOut(ch.video, final_dir, writer, device, anns, eval_dir, overlay_dir, evaluated, "premvos_amd.stream --track")
                    tr.evaluator = sink.open(tr.T)
                store: Optional[ChunkStore] = ch.parts.get("refine")
                flow = ch.parts.get("flow")
                if tr.T:
                    assert store is not None and store.T == tr.T, "the chunk's store was laid out for another number of objects"
                    stream.wait_event(store.event)
                    if flow is not None:
                        stream.wait_event(flow[1])
            n_frames += 1
            if not tr.T:                                          # do_video: a video without templates gets all-zero PNGs
                sink.blank(name, frames[k])
                continue
            nxt = frames[k + 1] if k + 1 < n else pl["nxt"]
            has_flow = nxt is not None and flow is not None and k < flow[0].shape[0]
            stack, fresh, rows, scores, next_slots = store.frame(k)
            got = sum(c for _, c in fr.pieces)
            assert got == store.counts[k], f"{ch.video}/{name}: {got} of {store.counts[k]} refined masks reached the tracker"
            sink.expect(name)
            if overlay_dir is not None:                           # (called inside step_resident, right behind the paint)
                tr.on_idmap = lambda idmap, name=name, frame=frames[k]: sink.overlay(name, frame, idmap)
            r = tr.step_resident(fresh, rows, scores, flow[0][k] if has_flow else None,
                                 jpeg.to_device(nxt, device) if has_flow else None, stack=stack,
                                 next_slots=next_slots if has_flow else None)
            sink.pngs(r["idmap"], [(None, name)])
        if sink is not None:
            sink.close()
    return n_frames
