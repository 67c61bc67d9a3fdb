"""Host side of `premvos_amd.stream --track` (no GPU): the command line and its refusals, the pre-flight, the track feed between the
stage threads and the tracker thread driven with fake payloads (order, bound, shutdown), and the two C-ABI entries of the resident
step: declared, bound, counted in the documents, built for gfx950 and refusing bad arguments before any HIP call."""
import itertools
import json
import os
import re
import threading
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- command line
def test_track_implies_reid_and_has_the_live_configs_as_defaults(monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    a = stream.parse_args([])
    assert a.track is False and a.reid is False
    a = stream.parse_args(["--track"])
    assert a.track is True and a.reid is True and a.reid_config == "code/ReID_net/configs/run"
    assert a.track_refinement_config == "code/refinement_net/configs/live" and a.track_reid_config == "code/ReID_net/configs/live"
    a = stream.parse_args(["--track", "--track_reid_config", "x/y/z", "--gpus", "2"])
    assert a.track_reid_config == "x/y/z" and a.gpus == 2
    assert stream.parse_args(["--reid"]).track is False                     # the other way round nothing is implied


def _tree(root, videos):
    for name, n in videos.items():
        d = root / "data" / "DAVIS" / "JPEGImages" / "480p" / name
        d.mkdir(parents=True)
        for t in range(n):
            (d / f"{t:05d}.jpg").write_bytes(b"")
    (root / "seq_to_run.txt").write_text("".join(f"data/DAVIS/JPEGImages/480p/{name}/\n" for name in videos))


def _snapshot(root):
    return sorted(str(p.relative_to(root)) for p in root.rglob("*"))


def test_the_three_refusals_each_with_its_own_message_write_nothing(tmp_path, monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _tree(tmp_path, {"bear": 3})
    before = _snapshot(tmp_path)
    cwd = os.getcwd()
    with pytest.raises(SystemExit) as e:
        stream.main(["--root", str(tmp_path), "--track", "--gather"])
    assert str(e.value) == stream.REFUSE_TRACK_GATHER and "--track" in str(e.value) and "--gather" in str(e.value)
    monkeypatch.setenv("PREMVOS_SIDECAR", "1")
    with pytest.raises(SystemExit) as e:
        stream.main(["--root", str(tmp_path), "--track"])
    assert str(e.value) == stream.REFUSE_TRACK_SIDECAR and "PREMVOS_SIDECAR=1" in str(e.value)
    monkeypatch.setenv("PREMVOS_SIDECAR", "0")
    with pytest.raises(SystemExit) as e:                                    # one video, two ranks: frame ranges
        stream.main(["--root", str(tmp_path), "--track", "--gpus", "2"])
    assert str(e.value) == stream.REFUSE_TRACK_RANGES and "whole videos" in str(e.value)
    assert len({stream.REFUSE_TRACK_GATHER, stream.REFUSE_TRACK_SIDECAR, stream.REFUSE_TRACK_RANGES, stream.REFUSE_REID_GATHER,
                stream.REFUSE_REID_SIDECAR}) == 5
    with pytest.raises(SystemExit) as e:                                    # the library entry refuses the pair as well
        stream.run(str(tmp_path), "seq_to_run.txt", "a", "b", "c", "d", gather=True, reid_config="code/ReID_net/configs/run",
                   track={"refinement_config": "r", "reid_config": "q"})
    assert str(e.value) == stream.REFUSE_TRACK_GATHER
    assert os.getcwd() == cwd and _snapshot(tmp_path) == before


def test_the_plan_check_wants_whole_videos():
    from premvos_amd import stream
    from premvos_amd.parallel import plan_shards
    for counts, world, ok in (([5, 3], 1, True), ([5, 3], 2, True), ([5, 3, 4], 2, True), ([5], 2, False), ([9, 8], 3, False)):
        plans = [plan_shards(counts, world, r, 2, "balanced") for r in range(world)]
        assert stream.whole_videos(plans, counts) is ok, (counts, world, plans)


def test_the_preflight_names_the_missing_live_configs_and_nothing_else(tmp_path, monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    _tree(tmp_path, {"bear": 2})
    ref, reid = "code/refinement_net/configs/live", "code/ReID_net/configs/live"
    assert len(stream.check_track_inputs(str(tmp_path), ref, reid)) == 2
    (tmp_path / "code" / "refinement_net" / "configs").mkdir(parents=True)
    (tmp_path / ref).write_text("{}")
    problems = stream.check_track_inputs(str(tmp_path), ref, reid)
    assert len(problems) == 1 and reid in problems[0]
    before, cwd = _snapshot(tmp_path), os.getcwd()
    with pytest.raises(SystemExit) as e:                                    # before any GPU work, before anything is written
        stream.run(str(tmp_path), "seq_to_run.txt", "a", "b", "c", "d", reid_config="code/ReID_net/configs/run",
                   track={"refinement_config": ref, "reid_config": reid})
    assert "inputs are not ready" in str(e.value) and reid in str(e.value) and ref + " is missing" not in str(e.value)
    assert os.getcwd() == cwd and _snapshot(tmp_path) == before
    (tmp_path / "code" / "ReID_net" / "configs").mkdir(parents=True)
    (tmp_path / reid).write_text("{}")
    assert stream.check_track_inputs(str(tmp_path), ref, reid) == []        # no ReID_proposals/, no flow/, no annotation: not errors


# --------------------------------------------------------------------------------------------------------------------- the feed
def _no_test_threads_left():
    deadline = time.time() + 5
    while time.time() < deadline:
        if not [t for t in threading.enumerate() if t.name.startswith("feedtest-")]:
            return True
        time.sleep(0.05)
    return False


def _start(fn, name):
    t = threading.Thread(target=fn, name="feedtest-" + name, daemon=True)
    t.start()
    return t


# per chunk: frames -> proposals per frame (0 = a frame that never reaches on_masks; 5 with launches of 2 = three calls)
CHUNKS = [("a", [3, 0]), ("a", [5, 1]), ("a", [0]), ("b", [2, 2]), ("b", [0, 0]), ("b", [4])]


def _complete(feed, ch, counts, launch=2):
    """What a refinement lane does with one chunk: its frames' slots in launches of ``launch`` slots that may span frames."""
    slots = [(k, i) for k, c in enumerate(counts) for i in range(c)]
    for s0 in range(0, len(slots), launch):
        group = slots[s0:s0 + launch]
        a = 0
        while a < len(group):
            b = a + 1
            while b < len(group) and group[b] == (group[a][0], group[a][1] + b - a):
                b += 1
            feed.put_masks(ch, group[a][0], group[a][1], b - a)
            a = b
    feed.part_done(ch, "refine", ("store", ch.index))


@pytest.mark.parametrize("order", list(itertools.permutations(range(4))) + [(5, 4, 3, 2, 1, 0), (1, 0, 3, 2, 5, 4)])
def test_chunks_completed_in_any_order_come_out_in_frame_order(order):
    """Six chunks of two videos; the refinement parts arrive in ``order`` (two lanes finish out of order), the flow parts ahead of
    all of them.  The consumer sees every frame once, in frame order, with all its pieces -- zero-proposal frames included."""
    from premvos_amd.stream_track import TrackFeed
    feed = TrackFeed(capacity=len(CHUNKS))
    opened = []
    for i, (video, counts) in enumerate(CHUNKS):
        opened.append(feed.open_chunk(video, [f"{i}_{k}" for k in range(len(counts))], key=counts, tag=i))
    assert [c.first for c in opened] == [True, False, False, True, False, False]
    assert all(feed.lookup(counts) is ch for (_, counts), ch in zip(CHUNKS, opened))
    got = []

    def consume():
        for fr in feed.frames():
            got.append((fr.chunk.index, fr.k, fr.name, fr.pieces, fr.chunk.parts["flow"], fr.chunk.parts["refine"]))
    t = _start(consume, "consumer")
    for ch in opened:                                                         # the flow thread runs ahead of both lanes
        feed.part_done(ch, "flow", ("flow", ch.index))
    todo = list(order) + [i for i in range(len(CHUNKS)) if i not in order]
    for i in todo:
        time.sleep(0.005)
        _complete(feed, opened[i], CHUNKS[i][1])
    feed.end()
    t.join(10)
    assert not t.is_alive() and _no_test_threads_left()
    want = [(i, k) for i, (_, counts) in enumerate(CHUNKS) for k in range(len(counts))]
    assert [(g[0], g[1]) for g in got] == want
    for i, k, name, pieces, flow, store in got:
        assert name == f"{i}_{k}" and flow == ("flow", i) and store == ("store", i)
        assert sum(c for _, c in pieces) == CHUNKS[i][1][k]                   # every slot arrived, once
        assert [p[0] for p in pieces] == sorted(p[0] for p in pieces)
        cover = [s for i0, c in pieces for s in range(i0, i0 + c)]
        assert cover == list(range(CHUNKS[i][1][k]))
    assert got[0][3] and len(got[2][3]) == 3 and got[1][3] == []             # 3 slots in 2 calls; 5 slots in 3 calls; none


def test_the_bound_blocks_the_producer_until_the_consumer_closes_a_chunk():
    from premvos_amd.stream_track import TrackFeed
    feed = TrackFeed(capacity=2, poll=0.02)
    opened, released = [], threading.Event()

    def produce():
        for i in range(4):
            opened.append(feed.open_chunk("v", [str(i)]))
        feed.end()
    t = _start(produce, "producer")
    time.sleep(0.3)
    assert len(opened) == 2 and t.is_alive()                                  # full: the third open waits
    it = feed.chunks()
    for ch in list(opened):
        feed.part_done(ch, "flow")
        feed.part_done(ch, "refine")
    assert next(it).index == 0
    time.sleep(0.2)
    assert len(opened) == 2                                                   # taken, not yet closed
    assert next(it).index == 1                                                # asking for the next one closes chunk 0
    deadline = time.time() + 5
    while len(opened) < 3 and time.time() < deadline:
        time.sleep(0.01)
    assert len(opened) == 3
    for i in (2, 3):
        while len(opened) <= i:
            time.sleep(0.01)
        feed.part_done(opened[i], "flow")
        feed.part_done(opened[i], "refine")
        assert next(it).index == i
    with pytest.raises(StopIteration):
        next(it)
    t.join(5)
    assert not t.is_alive() and feed.waited_s > 0.2 and _no_test_threads_left()


def test_a_consumer_that_raises_releases_every_producer():
    """The tracker fails on its second chunk: the producer that waits on the full feed and the one that would open a chunk later
    both get FeedClosed, at once; nothing is left waiting."""
    from premvos_amd.stream_track import FeedClosed, TrackFeed
    feed = TrackFeed(capacity=1)
    errors, results = [], []

    def consume():
        try:
            for n, ch in enumerate(feed.chunks()):
                if n == 1:
                    raise RuntimeError("tracker failure at chunk 1")
        except BaseException as e:      # noqa: BLE001
            errors.append(e)
            feed.fail(e)

    def produce():
        try:
            for i in range(10):
                ch = feed.open_chunk("v", [str(i)])
                feed.part_done(ch, "flow")
                feed.part_done(ch, "refine")
            results.append("all opened")
        except FeedClosed as e:
            results.append(e)
    t0 = time.time()
    threads = [_start(consume, "consumer"), _start(produce, "producer")]
    for t in threads:
        t.join(20)
    assert time.time() - t0 < 20 and _no_test_threads_left()
    assert len(errors) == 1 and "tracker failure at chunk 1" in str(errors[0])
    assert len(results) == 1 and isinstance(results[0], FeedClosed) and results[0].__cause__ is errors[0]
    with pytest.raises(FeedClosed):
        feed.open_chunk("v", ["late"])
    # and the other direction: a stage failure ends a consumer that waits for a part that will never come
    feed2 = TrackFeed(capacity=2)
    feed2.open_chunk("v", ["0"])
    seen = []

    def consume2():
        try:
            for ch in feed2.chunks():
                seen.append(ch)
        except FeedClosed as e:
            seen.append(e)
    t = _start(consume2, "consumer2")
    time.sleep(0.1)
    feed2.fail(RuntimeError("stage failure"))
    t.join(5)
    assert not t.is_alive() and len(seen) == 1 and isinstance(seen[0], FeedClosed)


def test_run_sequences_with_a_failing_tracker_ends_every_thread(tmp_path, monkeypatch):
    """The thread skeleton of StreamPipeline.run_sequences with fake stage bodies (as tests/test_cpu_stream_host.py) and a tracker
    whose body raises: the first error is re-raised, no premvos- thread is left."""
    from PIL import Image
    from premvos_amd import stream, stream_track
    monkeypatch.setenv("PREMVOS_GPU_JPEG", "0")
    monkeypatch.setenv("PREMVOS_TRACK_FEED_CHUNKS", "2")
    d = tmp_path / "seq"
    d.mkdir()
    for t in range(40):
        Image.fromarray(np.full((6, 8, 3), t, np.uint8)).save(d / f"{t:05d}.png")
    p = object.__new__(stream.StreamPipeline)
    p.batch, p.out, p.dev, p.refine_lanes, p.streams = 2, "out", "cpu", 2, {"track": None}
    p.track, p.track_engines, p.track_timer, p._feed = {"final": str(tmp_path / "final"), "anns": str(tmp_path / "anns")}, None, None, None
    seen = []

    def flow(chunk, writer):
        p._feed.part_done(p._feed.lookup(chunk[2]), "flow", None)

    def proposals(which, chunk, writer):
        return chunk, [[] for _ in chunk[2]]

    def refine(item, writer, lane=0):
        p._feed.part_done(p._feed.lookup(item[0][2]), "refine", None)

    def tracker(feed, engines, final, writer, st, dev, timer=None):
        for n, ch in enumerate(feed.chunks()):
            seen.append(ch.index)
            if n == 3:
                raise RuntimeError("tracker failure at chunk 3")
    p._flow, p._proposals, p._refine = flow, proposals, refine
    monkeypatch.setattr(stream_track, "run_tracker", tracker)
    p.streams = {"track": type("S", (), {"synchronize": lambda self: None})()}
    t0 = time.time()
    with pytest.raises(RuntimeError, match="tracker failure at chunk 3"):
        p.run_sequences([str(d) + "/"])
    assert time.time() - t0 < 20 and seen == [0, 1, 2, 3]
    deadline = time.time() + 5
    while time.time() < deadline and [t for t in threading.enumerate() if t.name.startswith("premvos-")]:
        time.sleep(0.05)
    assert not [t for t in threading.enumerate() if t.name.startswith("premvos-")]
    # and a run in which nothing fails hands every chunk over, in order
    seen.clear()
    monkeypatch.setattr(stream_track, "run_tracker", lambda feed, *a, **k: seen.extend(ch.index for ch in feed.chunks()))
    assert p.run_sequences([str(d) + "/"]) == 40 and seen == list(range(20))


def test_a_video_with_more_objects_than_the_engines_hold_stops_the_run_before_any_work(tmp_path, monkeypatch):
    """41 annotated objects against max_boxes = 40: refused when the annotations are read, before a thread is started or a file
    written, with a message that names the video and the two-program path."""
    from PIL import Image
    from premvos_amd import _lib, stream
    from premvos_amd.track import write_png
    monkeypatch.setenv("PREMVOS_GPU_JPEG", "0")
    for name in ("few", "many"):
        d = tmp_path / "images" / name
        d.mkdir(parents=True)
        for t in range(2):
            Image.fromarray(np.zeros((8, 64, 3), np.uint8)).save(d / f"{t:05d}.jpg")
        ann = np.zeros((8, 64), np.uint8)
        n = 3 if name == "few" else 41
        ann[0, :n] = np.arange(1, n + 1)
        write_png(str(tmp_path / "anns" / name / "00000.png"), ann)
    assert len(stream._video_templates(str(tmp_path / "images" / "few") + "/", str(tmp_path / "anns"))) == 3
    assert stream._video_templates(str(tmp_path / "images" / "few") + "/", str(tmp_path / "nowhere")) == []
    p = object.__new__(stream.StreamPipeline)
    p.batch, p.out, p.dev, p.refine_lanes, p.streams = 2, "out", "cpu", 2, {}
    p.track, p.track_timer, p._feed = {"final": str(tmp_path / "final"), "anns": str(tmp_path / "anns")}, None, None
    eng = type("E", (), {"max_boxes": 40})()
    p.track_engines = (eng, eng)
    before = sorted(str(q) for q in tmp_path.rglob("*"))
    with pytest.raises(_lib.PremvosError, match="41 annotated objects") as e:
        p.run_sequences([str(tmp_path / "images" / "few") + "/", str(tmp_path / "images" / "many") + "/"])
    assert "many" in str(e.value) and "premvos_amd.track" in str(e.value)
    assert sorted(str(q) for q in tmp_path.rglob("*")) == before
    assert not [t for t in threading.enumerate() if t.name.startswith("premvos-")]


def test_the_timing_tool_builds_its_job_and_reads_its_arguments(tmp_path, monkeypatch):
    """tools/time_stream_track.py on the host: its job (the two `live` configs, an annotation of N objects on top of the --reid
    tool's job, which is replaced by a stub here: full-depth weights are not needed to check the plumbing) and its command line."""
    import sys
    sys.path.insert(0, ROOT)
    from PIL import Image
    from tools import time_stream_reid, time_stream_track as TT
    made = []

    def base_job(root, n_frames):
        made.append((root, n_frames))
        os.makedirs(os.path.join(root, "code", "ReID_net", "configs"))
        os.makedirs(os.path.join(root, "data", "DAVIS", "JPEGImages", "480p", "clip0"))
    monkeypatch.setattr(time_stream_reid, "build_job", base_job)
    TT.build_job(str(tmp_path), 5, objects=10)
    assert made == [(str(tmp_path), 5)]
    for key, load in (("refinement_config", "../weights/refine.pt"), ("reid_config", "../weights/reid.pt")):
        assert json.load(open(tmp_path / TT.LIVE[key]))["load"] == load
    assert TT.LIVE == {"refinement_config": "code/refinement_net/configs/live", "reid_config": "code/ReID_net/configs/live"}
    ann = np.array(Image.open(tmp_path / "data" / "DAVIS" / "Annotations" / "480p" / "clip0" / "00000.png"))
    assert ann.shape == (480, 854) and sorted(np.unique(ann).tolist()) == list(range(11))
    assert min(int((ann == i).sum()) for i in range(1, 11)) > 3000                  # ten objects, none painted over
    a = TT.parse_args([])
    assert a.frames == 128 and a.objects == 10 and a.alternations == 2 and a.child is None and a.out.endswith("profiles/stream_track.json")
    a = TT.parse_args(["--child", "track_program", "--root", "R", "--inter", "I", "--frames", "16"])
    assert (a.child, a.root, a.inter, a.frames) == ("track_program", "R", "I", 16)
    with pytest.raises(SystemExit):
        TT.parse_args(["--child", "nonsense"])
    assert set(TT.PHASES) == {"inputs", "overlap", "scores", "paint", "warp", "boxes+reid", "refine"}
    src = open(os.path.join(ROOT, "premvos_amd", "track.py")).read()
    for ph in TT.PHASES:                                                            # the phases the tool sums are the ones the step ticks
        assert f'self._tick("{ph}")' in src, ph


def test_store_bytes_is_the_formula_of_the_design_text():
    from premvos_amd.stream_track import store_bytes
    assert store_bytes(8, 40, 10, 480, 854) == 8 * (50 * 480 * 854 + 40 * 536 + 480 * 854 * 8)
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "chunk x ((T + P) x H x W + P x 536 + 8 x H x W)" in text


# ----------------------------------------------------------------------------------------------------------------- the C-ABI
def test_header_signatures_and_documents_name_the_two_new_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    for name in ("premvos_track_inputs_f64", "premvos_track_next_f32"):
        assert name in declared and name in _lib.SIGNATURES
        for doc in ("DESIGN.md", "INTEGRATION.md", "profiles/track_README.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    assert len(_lib.SIGNATURES["premvos_track_inputs_f64"]) == 9 and len(_lib.SIGNATURES["premvos_track_next_f32"]) == 6
    assert _lib.ABI_VERSION == 21                                             # additive: nothing an older caller binds has changed
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v{_lib.ABI_VERSION}" in open(os.path.join(ROOT, doc)).read(), doc
    for cite in ("merge_functions.py:234", "merge_functions.py:27-36"):
        assert cite in hdr
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "track_ops.hip")).read()
    assert src.startswith("// hipcc-flags: -ffp-contract=off")               # 0.5 * (s + 1) must stay an add and a multiply
    for kernel, block in (("track_inputs_kernel", 256), ("track_next_kernel", 64)):
        assert re.search(r"__launch_bounds__\(%d\) void %s" % (block, kernel), src) and block % 64 == 0


def test_library_built_for_gfx950_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21
    one = np.zeros(1024, np.float64).ctypes.data
    assert lib.premvos_track_inputs_f64(None, None, None, None, 1, 1, None, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert lib.premvos_track_inputs_f64(one, one, None, one, 1, 1, one, one, None) == -1 and b"null" in lib.premvos_last_error()
    assert lib.premvos_track_inputs_f64(one, None, one, one, 1, 1, one, one, None) == -1
    assert lib.premvos_track_inputs_f64(one, one, one, one, 1, 1, None, one, None) == -1
    assert lib.premvos_track_inputs_f64(one, one, one, one, -1, 1, one, one, None) == -1 and b"negative" in lib.premvos_last_error()
    assert lib.premvos_track_inputs_f64(one, one, one, one, 1, -2, one, one, None) == -1 and b"negative" in lib.premvos_last_error()
    assert lib.premvos_track_inputs_f64(one, one, one, one, 256, 1, one, one, None) == -1 and b"255" in lib.premvos_last_error()
    assert lib.premvos_track_inputs_f64(one, one, None, None, 0, 0, one, one, None) == 0      # nothing to do: no launch
    assert lib.premvos_track_next_f32(None, None, 1, None, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert lib.premvos_track_next_f32(one, one, 1, one, None, None) == -1
    assert lib.premvos_track_next_f32(one, None, 1, one, one, None) == -1
    assert lib.premvos_track_next_f32(one, one, -1, one, one, None) == -1 and b"negative" in lib.premvos_last_error()
    assert lib.premvos_track_next_f32(one, one, 0, one, one, None) == 0
