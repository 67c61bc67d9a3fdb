"""The inputs of the live loop's three trackers, stated once in premvos_amd/track.py (no GPU): ``_gt_idmap``, ``_flow_tensor``,
``_frame_array``, ``require_annotations``; and that the advance of a step lives in ``TrackerGroup`` alone.  The refusals' texts are the
ones ``Tracker._score_select_paint``, ``Tracker._sheet``, ``SearchGroup.step``, ``do_video`` and ``search_video`` raised before they
shared these helpers, written out here."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
WHO = ("the oracle merge", "the score sheet", "the weight search")


@pytest.mark.parametrize("who", WHO)
def test_gt_idmap_refuses_another_dtype_and_another_shape(who):
    from premvos_amd import _lib, track
    with pytest.raises(_lib.PremvosError) as e:
        track._gt_idmap(np.zeros((8, 12), np.int32), (8, 12), who)
    assert str(e.value) == f"{who}: gt must be a uint8 id map of shape (8, 12) (got torch.int32, (8, 12))"
    with pytest.raises(_lib.PremvosError) as e:
        track._gt_idmap(torch.zeros((12, 8), dtype=torch.uint8), torch.Size((8, 12)), who)
    assert str(e.value) == f"{who}: gt must be a uint8 id map of shape (8, 12) (got torch.uint8, (12, 8))"


def test_gt_idmap_copies_a_read_only_array_and_returns_a_tensor_as_it_is():
    from premvos_amd import track
    a = np.arange(96, dtype=np.uint8).reshape(8, 12)
    a.setflags(write=False)                                                                     # as np.asarray(PIL image) is
    g = track._gt_idmap(a, (8, 12), WHO[0])
    assert g.dtype == torch.uint8 and tuple(g.shape) == (8, 12) and np.array_equal(g.numpy(), a)
    assert not np.shares_memory(g.numpy(), a)
    g[0, 0] = 7                                                                                 # writable, and the array is untouched
    assert a[0, 0] == 0
    t = torch.zeros((8, 12), dtype=torch.uint8)
    assert track._gt_idmap(t, (8, 12), WHO[2]) is t


def test_flow_tensor_of_a_name_an_array_and_a_tensor(tmp_path):
    import track_restated as R
    from premvos_amd import track
    flow = np.random.default_rng(0).normal(0, 2, (8, 12, 2))                                    # float64
    fn = str(tmp_path / "00000.flo")
    R.write_flo(fn, flow)
    want = torch.from_numpy(flow.astype(np.float32))
    for given in (fn, flow, flow.astype(np.float32)):
        got = track._flow_tensor(given)
        assert got.dtype == torch.float32 and tuple(got.shape) == (8, 12, 2) and torch.equal(got, want)
    assert track._flow_tensor(want) is want


def test_frame_array_of_a_name_an_array_and_a_tensor(tmp_path):
    from PIL import Image
    from premvos_amd import track
    rgb = np.random.default_rng(1).integers(0, 256, (8, 12, 3), dtype=np.uint8)
    jpg, grey = str(tmp_path / "00000.jpg"), str(tmp_path / "grey.png")
    Image.fromarray(rgb).save(jpg, quality=95)
    Image.fromarray(rgb[..., 0], mode="L").save(grey)
    got = track._frame_array(jpg)
    assert got.dtype == np.uint8 and got.shape == (8, 12, 3) and np.array_equal(got, np.asarray(Image.open(jpg).convert("RGB")))
    got = track._frame_array(grey)                                                              # mode L: three equal channels
    assert got.dtype == np.uint8 and got.shape == (8, 12, 3) and all(np.array_equal(got[..., c], rgb[..., 0]) for c in range(3))
    t = torch.from_numpy(rgb)
    assert track._frame_array(rgb) is rgb and track._frame_array(t) is t


@pytest.mark.parametrize("what", ("the oracle merge needs", "the score sheets need", "the weight search needs"))
def test_require_annotations_names_exactly_the_missing_file(tmp_path, what):
    import track_restated as R
    from premvos_amd import _lib, track
    images, anns = str(tmp_path / "images") + "/", str(tmp_path / "anns") + "/"
    os.makedirs(images + "clip")
    os.makedirs(anns + "clip")
    fns = [images + f"clip/{t:05d}.jpg" for t in range(2)]
    for fn in fns:
        open(fn, "wb").close()
    R.write_index_png(anns + "clip/00000.png", np.zeros((8, 12), np.uint8))
    with pytest.raises(_lib.PremvosError) as e:
        track.require_annotations(fns, images, anns, "clip", what)
    assert str(e.value) == f"clip: {what} an annotation for every frame; missing: {anns}clip/00001.png"
    assert track.missing_annotations(fns, images, anns) == [anns + "clip/00001.png"]
    R.write_index_png(anns + "clip/00001.png", np.zeros((8, 12), np.uint8))
    assert track.require_annotations(fns, images, anns, "clip", what) is None


def test_the_advance_of_a_step_is_in_the_tracker_group_alone():
    from premvos_amd import track
    group, search = inspect.getsource(track.TrackerGroup), inspect.getsource(track.SearchGroup)
    for text in ("premvos_track_next_f32", "refine_group(", "embed_masks("):
        assert text in group and text not in search, text
