"""premvos_amd.merge_out (no GPU): the one per-video output object of the five merge loops -- its paths, which jobs reach the writer, the
video without templates, the evaluator that does not open, the slot writers' release, the stale-file and summary helpers.  The writer
is a stub that runs every job at once; ``overlay.forward`` and ``LoopEval`` are replaced where a device would be needed."""
import json
import os

import numpy as np
import pytest
import torch


class InlineWriter:
    def __init__(self):
        self.jobs = []

    def submit(self, fn, *args):
        self.jobs.append((fn, args))
        fn(*args)


class FakeSlot:
    def __init__(self, maps):
        self.maps, self.waited, self.released = maps, 0, 0

    def wait(self):
        self.waited += 1
        return self.maps

    def release(self):
        self.released += 1


def _sink(tmp_path, video="v", **kw):
    from premvos_amd.merge_out import VideoOut
    w = InlineWriter()
    return VideoOut(video, str(tmp_path / "out") + "/", w, "cpu", **kw), w


def _fake_overlay(monkeypatch):
    """overlay.forward / write_jpg and jpeg.to_device / imread without a device: -> the list of (file name, frame, idmap) written"""
    from premvos_amd import jpeg, overlay
    written = []
    monkeypatch.setattr(jpeg, "to_device", lambda item, device=None, bgr=False: ("dev", item))
    monkeypatch.setattr(jpeg, "imread", lambda src, device=None, bgr=False: ("read", src))
    monkeypatch.setattr(overlay, "forward", lambda frame, idmap: (frame, idmap))
    monkeypatch.setattr(overlay, "write_jpg", lambda fn, enc: written.append((fn,) + enc))
    return written


@pytest.mark.parametrize("video,png,jpg,evf", [("v", "/t/out/v/00003.png", "/t/overlay/v/00003.jpg", "/t/eval/v.json"),
                                               ("a/b", "/t/out/a/b/00003.png", "/t/overlay/a/b/00003.jpg", "/t/eval/a/b.json")])
def test_paths_are_the_strings_the_loops_always_built(video, png, jpg, evf):
    from premvos_amd import track
    from premvos_amd.merge_out import VideoOut
    images, out, overlay, eval_dir = "/t/images/", "/t/out/", "/t/overlay/", "/t/eval"
    image_fn = os.path.join(images, video, "00003.jpg")
    rel = os.path.splitext(os.path.relpath(image_fn, images))[0]                                  # do_video's formulas before the sink
    assert (os.path.join(out, rel + ".png"), os.path.join(overlay, rel + ".jpg"), os.path.join(eval_dir, video + ".json")) == (png, jpg, evf)
    s = VideoOut(os.path.relpath(os.path.join(images, video) + "/", images).strip("/"), out, None, "cpu", eval_dir=eval_dir, overlay_dir=overlay)
    assert s.video == video
    assert (s.png_path("00003"), s.jpg_path("00003")) == (png, jpg)          # (the eval file's name is LoopEval.dump's: the first formula)
    assert s.jpg_path("00003", "/t/viz/") == "/t/viz/" + video + "/00003.jpg"                     # the score sheets' root
    lay = {"images": images, "anns": "/t/anns/", "props": "/t/props/", "flows": "/t/flows/", "out": out}
    assert track._frame_paths(image_fn, lay) == ("/t/anns/" + video + "/00003.png", "/t/props/" + video + "/00003.json",
                                                 "/t/flows/" + video + "/00003.flo", png)
    assert VideoOut(video, "/t/out", None, "cpu").png_path("00003") == png                        # a root without the trailing slash


def test_without_eval_and_overlay_only_the_png_job_reaches_the_writer(tmp_path):
    from premvos_amd import merge_out, track
    s, w = _sink(tmp_path)
    assert s.open(3) is None
    for k in range(3):
        stem = f"{k:05d}"
        s.expect(stem)
        s.overlay(stem, np.zeros((8, 12, 3), np.uint8), None)
        if k == 0:
            s.png(stem, np.full((8, 12), 2, np.uint8))
        elif k == 1:
            s.pngs(FakeSlot(np.full((8, 12), 2, np.uint8)), [(None, stem)])
        else:
            s.blank(stem, np.zeros((8, 12, 3), np.uint8))
        assert len(w.jobs) == k + 1
    s.close()
    assert [fn for fn, _ in w.jobs] == [track.write_png, merge_out.write_pngs, track.write_png]
    assert sorted(os.listdir(tmp_path / "out" / "v")) == ["00000.png", "00001.png", "00002.png"] and os.listdir(tmp_path) == ["out"]


def test_a_video_without_templates(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from premvos_amd import track
    written = _fake_overlay(monkeypatch)
    evaluated = []
    s, w = _sink(tmp_path, anns=str(tmp_path / "anns"), eval_dir=str(tmp_path / "eval"), overlay_dir=str(tmp_path / "overlay"),
                 evaluated=evaluated, program="premvos_amd.stream --track")
    assert s.open(0) is None
    frame = np.full((8, 12, 3), 7, np.uint8)
    zeros = s.blank("00000", frame)
    s.close()
    assert capsys.readouterr().out == "premvos_amd.stream --track: v: no templates, not evaluated\n"
    assert zeros.shape == (8, 12) and zeros.dtype == np.uint8 and not zeros.any()
    im = Image.open(s.png_path("00000"))
    assert im.mode == "P" and im.size == (12, 8) and not np.array(im).any()
    assert np.array_equal(np.array(im.getpalette(), np.uint8).reshape(-1, 3), track.voc_palette())
    assert len(written) == 1 and written[0][0] == str(tmp_path / "overlay" / "v" / "00000.jpg") and written[0][2] is None
    assert written[0][1][0] == "dev" and written[0][1][1] is frame                               # the frame itself, no id map
    assert evaluated == [] and not os.path.exists(tmp_path / "eval") and len(w.jobs) == 2
    # a file name as the frame: its size from the header, the overlay from the file
    Image.fromarray(frame).save(tmp_path / "f.jpg")
    assert s.blank("00001", str(tmp_path / "f.jpg")).shape == (8, 12) and written[1][1] == ("read", str(tmp_path / "f.jpg"))
    assert s.blank("00002", frame, (4, 6)).shape == (4, 6)                                       # the lockstep loop names the size


def test_an_evaluator_that_opens_as_none(tmp_path, capsys):
    from premvos_amd import track
    for k in range(2):
        track.write_png(str(tmp_path / "anns" / "v" / f"{k:05d}.png"), np.zeros((8, 12), np.uint8))
    evaluated = []
    s, w = _sink(tmp_path, anns=str(tmp_path / "anns"), eval_dir=str(tmp_path / "eval"), evaluated=evaluated)
    assert s.open(1) is None and s.evaluator is None
    out = capsys.readouterr().out
    assert "fewer than three annotated frames" in out and "no templates" not in out
    s.expect("00000")
    s.close()
    assert w.jobs == [] and evaluated == [] and not os.path.exists(tmp_path / "eval")


def test_an_evaluator_that_opens_is_dumped_once_and_named(tmp_path, monkeypatch):
    from premvos_amd import evaluate
    calls = []

    class Eval:
        @classmethod
        def open(cls, video, annotation_dir, device=None):
            calls.append(("open", video, annotation_dir, device))
            return cls()

        def expect(self, name):
            calls.append(("expect", name))

        def fetch(self):
            calls.append(("fetch",))
            return self

        def dump(self, eval_dir):
            calls.append(("dump", eval_dir))
    monkeypatch.setattr(evaluate, "LoopEval", Eval)
    evaluated = []
    s, w = _sink(tmp_path, "a/b", anns="/t/anns/", eval_dir="/t/eval", evaluated=evaluated)
    ev = s.open(2)
    assert isinstance(ev, Eval) and s.evaluator is ev
    s.expect("00001")
    s.close()
    s.close()
    assert calls == [("open", "a/b", "/t/anns/a/b", "cpu"), ("expect", "00001"), ("fetch",), ("dump", "/t/eval")]
    assert evaluated == ["a/b"] and len(w.jobs) == 1 and s.evaluator is None


def test_slot_writers_release_once_also_when_the_png_fails(tmp_path):
    from PIL import Image
    s, w = _sink(tmp_path)
    one = FakeSlot(np.full((8, 12), 3, np.uint8))
    s.pngs(one, [(None, "00000")])
    many = FakeSlot(np.stack([np.full((8, 12), k, np.uint8) for k in range(3)]))
    s.pngs(many, [(0, "00001"), (2, "00002")])
    assert (one.waited, one.released, many.waited, many.released) == (1, 1, 1, 1) and len(w.jobs) == 2
    assert [int(np.array(Image.open(s.png_path(f"{k:05d}"))).max()) for k in range(3)] == [3, 0, 2]

    class Event:
        n = 0

        def synchronize(self):
            self.n += 1
    ev = Event()
    s.pngs(torch.full((2, 8, 12), 5, dtype=torch.uint8), [(0, "00003"), (1, "00004")], ev)       # a host block with an event: nothing to release
    assert ev.n == 1 and int(np.array(Image.open(s.png_path("00004"))).min()) == 5
    (tmp_path / "file").write_text("x")                                                           # a PNG root whose parent is a file
    from premvos_amd.merge_out import VideoOut
    bad = VideoOut("v", str(tmp_path / "file" / "out"), w, "cpu")
    for slot, pairs in ((FakeSlot(np.zeros((8, 12), np.uint8)), [(None, "00000")]), (FakeSlot(np.zeros((2, 8, 12), np.uint8)), [(0, "00000"), (1, "00001")])):
        with pytest.raises(OSError):
            bad.pngs(slot, pairs)
        assert (slot.waited, slot.released) == (1, 1)


def test_stale_files_and_the_summary(tmp_path, monkeypatch, capsys):
    from premvos_amd import evaluate, merge_out
    d = tmp_path / "eval"
    merge_out.remove_stale(str(d), ["a"])                                                          # no directory yet
    merge_out.remove_stale(None, ["a"])
    d.mkdir()
    for v in "abc":
        (d / f"{v}.json").write_text("{}")
    merge_out.remove_stale(str(d), ["a", "c", "zz"])
    assert os.listdir(d) == ["b.json"]
    seen = []
    res = {"mean_J": 0.5, "mean_F": 0.25, "mean_JF_percent": 37.5}
    monkeypatch.setattr(evaluate, "summarise", lambda eval_dir, seqs: seen.append((eval_dir, seqs)) or res)
    fn = str(tmp_path / "sub" / "summary.json")
    merge_out.summarise(str(d), ["a", "b"], fn, "prog: mode:")
    assert seen == [(str(d), ["b"])] and capsys.readouterr().out == f"prog: mode: J 0.5  F 0.25  J&F 37.5  ->  {fn}\n"
    assert open(fn).read() == json.dumps(res, indent=1)
    merge_out.summarise(str(d), ["b"], fn, "prog:", indent=None)
    assert open(fn).read() == json.dumps(res) and capsys.readouterr().out == "prog: J 0.5  F 0.25  J&F 37.5  ->  " + fn + "\n"
    os.remove(fn)
    merge_out.summarise(str(d), ["a"], fn, "prog:")                                                # no video with a file: nothing
    assert not os.path.exists(fn) and capsys.readouterr().out == ""
