"""The largest-component clean-up on the GPU (csrc/components_ops.hip's three premvos_cc_* entries through ``components.label``,
``components.dilate``, ``components.keep_largest`` and ``python -m premvos_amd.components``) against the scipy restatement of the rule
(tests/components_restated.py).  Integers throughout: every comparison is exact.

The labelling works in tiles of 16 x 32 pixels; the 33 x 70 planes span two tiles and a tail in both directions, 130 x 260 eight and a
tail.  The dilation works in tiles of 64 x 64: the 130 x 70 case spans two and a tail in both directions."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import components_restated as X  # noqa: E402
import track_restated as R  # noqa: E402

SEED, SYNTHETIC, hand_cases = X.SEED, X.SYNTHETIC, X.hand_cases


def _dev():
    from premvos_amd import _lib
    _lib.require_gpu()
    return _lib.resolve_device(None)


def snake(H, W):
    """Full rows at every other line, joined alternately at the right and the left end: one component."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for j, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if j % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    m = np.zeros((H, W), np.uint8)
    m[H - 1] = 1
    m[:, 0::2] = 1                                                            # teeth joined at the bottom row: one component
    m[H // 2, :] = 0
    m[H - 1] = 1                                                              # ... the upper halves of the teeth are components of their own
    return m


@functools.lru_cache(maxsize=None)
def planes():
    """name -> (mask, its minimum-index labels by scipy), computed once."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:37, 0:53]
    out = {"snake_33x70": snake(33, 70), "checkerboard_37x53": ((yy + xx) % 2).astype(np.uint8), "comb_33x70": comb(33, 70),
           "empty_33x70": np.zeros((33, 70), np.uint8), "full_33x70": np.ones((33, 70), np.uint8), "snake_130x260": snake(130, 260),
           "one_pixel_1x1": np.ones((1, 1), np.uint8), "row_1x75": (rng.random((1, 75)) < 0.6).astype(np.uint8),
           "column_41x1": (rng.random((41, 1)) < 0.6).astype(np.uint8)}
    for density in (0.3, 0.45, 0.6):
        out[f"random_{density}_70x150"] = (rng.random((70, 150)) < density).astype(np.uint8)
    return {k: (m, X.min_index_labels(m)) for k, m in out.items()}


def test_the_planes_are_what_they_claim():
    p = planes()
    assert int(p["snake_33x70"][0].sum()) == 1206 and len(np.unique(p["snake_33x70"][1])) == 2       # one component of 1206 pixels (and -1)
    assert len(np.unique(p["checkerboard_37x53"][1])) == 2 and len(np.unique(p["snake_130x260"][1])) == 2
    assert len(np.unique(p["comb_33x70"][1])) == 2 + 35 and len(np.unique(p["random_0.3_70x150"][1])) > 50


@pytest.mark.parametrize("name", list(planes()))
def test_label_against_scipy(name):
    from premvos_amd import components
    mask, want = planes()[name]
    got = components.label(torch.from_numpy(mask).to(_dev()))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    again = components.label(torch.from_numpy(mask * 255).to(_dev())[None])                     # any non-zero value is set; a stack of one
    assert np.array_equal(again[0].cpu().numpy(), want)


def test_label_a_stack_equals_its_planes():
    from premvos_amd import components
    for size in ((33, 70), (70, 150)):
        group = [(m, w) for m, w in planes().values() if m.shape == size]
        assert len(group) >= 3
        got = components.label(torch.from_numpy(np.stack([m for m, _ in group])).to(_dev())).cpu().numpy()
        for j, (_, want) in enumerate(group):
            assert np.array_equal(got[j], want), (size, j)


@pytest.mark.parametrize("H, W", [(37, 53), (40, 260), (130, 70)])
def test_dilate_against_grey_dilation(H, W):
    from premvos_amd import components
    L = 3
    M = X.synthetic(H, W, L, SEED)
    M[0, 0], M[H - 1, W - 1], M[H - 1, 0] = 1, 2, 2                            # the corners: boxes clipped on two sides
    dev_map = torch.from_numpy(M).to(_dev())
    for D in (1, 2, 3, 4, 5, 16, 100):
        got = components.dilate(dev_map, L, D).cpu().numpy()
        assert got.shape == (L - 1, H, W) and got.dtype == np.uint8
        for k in range(1, L):
            assert np.array_equal(got[k - 1], X.dilate(M == k, D)), (D, k)
        if D == 1:
            assert np.array_equal(got[0], (M == 1).astype(np.uint8))
    sparse = np.zeros((H, W), np.uint8)
    sparse[H // 2, W // 2] = 2                                                # one pixel: the box itself, 255 wide and clipped
    got = components.dilate(torch.from_numpy(sparse).to(_dev())[None], L, 255).cpu().numpy()
    assert got.shape == (1, L - 1, H, W) and not got[0, 0].any() and np.array_equal(got[0, 1], X.dilate(sparse == 2, 255))


def _same(r, M, L, D):
    want = X.keep_largest(M, L, D)
    assert r["idmap"].dtype == torch.uint8 and r["removed"].dtype == torch.int32 and r["components"].dtype == torch.int32
    assert np.array_equal(r["idmap"].cpu().numpy(), want["idmap"][None])
    assert r["removed"].cpu().tolist() == [want["removed"].tolist()] and r["components"].cpu().tolist() == [want["components"].tolist()]
    return want


@pytest.mark.parametrize("H, W, L, D", SYNTHETIC)
def test_keep_largest_against_the_restatement(H, W, L, D):
    from premvos_amd import components
    M = X.synthetic(H, W, L, SEED)
    want = _same(components.keep_largest(torch.from_numpy(M).to(_dev())[None], L, D), M, L, D)
    assert want["removed"].sum() >= 0.05 * (M > 0).sum()


@pytest.mark.parametrize("name", list(hand_cases()))
def test_keep_largest_on_hand_made_cases(name):
    from premvos_amd import components
    M, D, keep, removed, ncomp = hand_cases()[name]
    r = components.keep_largest(torch.from_numpy(M).to(_dev())[None], 2, D)
    assert np.array_equal(r["idmap"][0].cpu().numpy(), keep) and r["removed"].tolist() == [[removed]] and r["components"].tolist() == [[ncomp]]
    _same(r, M, 2, D)


def test_keep_largest_with_absent_ids():
    """Ids {1, 3, 255}: L = 256, 252 planes without a pixel; and an id map with an id >= L, which is copied."""
    from premvos_amd import components
    M = X.synthetic(37, 53, 4, SEED)
    M[M == 2] = 255
    assert set(np.unique(M)) == {0, 1, 3, 255}
    want = _same(components.keep_largest(torch.from_numpy(M).to(_dev())[None], 256, 4), M, 256, 4)
    assert want["removed"][[0, 2, 254]].all() and want["removed"].sum() == want["removed"][[0, 2, 254]].sum()
    assert (want["components"] > 0).sum() == 3
    _same(components.keep_largest(torch.from_numpy(M).to(_dev())[None], 4, 4), M, 4, 4)          # 255 >= L: left alone


def test_a_stack_equals_its_frames_chunks_do_not_show_and_calls_repeat():
    from premvos_amd import components
    H, W, L, D = 37, 53, 3, 4
    maps = np.stack([X.synthetic(H, W, L, SEED + t) for t in range(3)])
    dev_maps = torch.from_numpy(maps).to(_dev())
    whole = components.keep_largest(dev_maps, L, D)
    assert whole["idmap"].shape == (3, H, W) and whole["removed"].shape == (3, L - 1) and whole["components"].shape == (3, L - 1)
    for t in range(3):
        want = X.keep_largest(maps[t], L, D)
        assert np.array_equal(whole["idmap"][t].cpu().numpy(), want["idmap"]), t
        assert whole["removed"][t].tolist() == want["removed"].tolist() and whole["components"][t].tolist() == want["components"].tolist(), t
    per_frame = components.PLANE_PIXEL_BYTES * (L - 1) * H * W
    for budget in (2 * per_frame, per_frame, 1, components.CHUNK_BYTES):
        part = components.keep_largest(dev_maps, L, D, chunk_bytes=budget)
        assert all(torch.equal(part[k], whole[k]) for k in ("idmap", "removed", "components")), budget
    assert torch.equal(dev_maps.cpu(), torch.from_numpy(maps))                                  # the input is left as it was


# -------------------------------------------------------------------------------------------------------------------- the command
def _listing(d):
    return {os.path.join(b, f): (os.path.getsize(os.path.join(b, f)), os.path.getmtime(os.path.join(b, f))) for b, _, fs in os.walk(d) for f in fs}


def test_the_command_on_a_tree(tmp_path, capsys):
    """Two videos of 3 frames of 24 x 40 under output/final, one of background alone: the PNGs under output/final_cc are byte for byte the
    restatement's maps through the same writer; the json's numbers; the eval files; output/final is left as it was."""
    from premvos_amd import components, track
    _dev()
    root = str(tmp_path)
    H, W, L, D = 24, 40, 3, 4
    anns = os.path.join(root, "data/DAVIS/Annotations/480p")
    maps = {}
    for video in ("clip", "void"):
        for d in (os.path.join(root, "output", "final", video), os.path.join(anns, video)):
            os.makedirs(d)
        for t in range(3):
            M = X.synthetic(H, W, L, SEED + t) if video == "clip" else np.zeros((H, W), np.uint8)
            maps[video, t] = M
            R.write_index_png(os.path.join(root, "output", "final", video, f"{t:05d}.png"), M)
            R.write_index_png(os.path.join(anns, video, f"{t:05d}.png"), M)
    before = _listing(os.path.join(root, "output", "final"))
    assert components.main(["--root", root, "--input", "final", "--dilate", str(D), "--eval"]) == 0
    said = capsys.readouterr().out
    out = os.path.join(root, "output")
    assert "final_cc" in said and _listing(os.path.join(out, "final")) == before
    assert sorted(os.listdir(out)) == ["eval_final_cc", "final", "final_cc", "final_cc.json", "premvos_amd_davis_eval_final_cc.json"]
    removed, ncomp = [], []
    for t in range(3):
        want = X.keep_largest(maps["clip", t], L, D)
        assert want["removed"].sum() > 0
        removed.append(want["removed"].tolist())
        ncomp.append(want["components"].tolist())
        for video, m in (("clip", want["idmap"]), ("void", maps["void", t])):
            fn = os.path.join(root, "expected.png")
            track.write_png(fn, m)
            assert open(os.path.join(out, "final_cc", video, f"{t:05d}.png"), "rb").read() == open(fn, "rb").read(), (video, t)
    res = json.load(open(os.path.join(out, "final_cc.json")))
    assert set(res) == {"videos", "frames", "dilate", "source"} and res["frames"] == 6 and res["dilate"] == D and res["source"] == "output/final"
    assert res["videos"] == {"clip": {"frames": 3, "L": L, "removed": removed, "components": ncomp},
                             "void": {"frames": 3, "L": 1, "removed": [[], [], []], "components": [[], [], []]}}
    assert os.listdir(os.path.join(out, "eval_final_cc")) == ["clip.json"]                      # (a video without objects is not scored)
    assert json.load(open(os.path.join(out, "premvos_amd_davis_eval_final_cc.json")))
    assert f"pixels removed: {sum(sum(r) for r in removed)}" in " ".join(said.split())
