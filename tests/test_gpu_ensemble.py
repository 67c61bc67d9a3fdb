"""The ensemble vote on the GPU (csrc/ensemble_ops.hip premvos_idmap_vote_u8, ``track.vote_idmaps``, ``track.EnsembleGroup``,
``track --ensemble``, ``track --prewarp --ensemble``, ``python -m premvos_amd.ensemble``) against the numpy restatement of the rule
(tests/ensemble_restated.py).  Everything is integer: every comparison is exact, no tolerance appears.

Kernel: ``voted``, ``votes`` and ``hist`` equal the restatement's for K in {1, 2, 3, 4, 5, 8} and pixel counts around the 16-byte
vector (1, 15, 16, 17), an odd plane (37 x 53), more than one workgroup with a tail (64 x 1024 + 5) and a 3 x 480 x 854 stack (many
workgroups: the atomics); with ``set_stride == pixels`` and ``pixels + 3`` (unaligned planes), ``voted`` one byte off an aligned buffer,
labels over {0..3} (many ties) and over 0..255, K identical maps, and a map in which every pattern of K = 4 labels appears.

Pipelines: the live form's voted stack is the restatement applied to its own members, and those members are ``search_video``'s id maps
for the same sets, byte for byte; the three commands write PNGs that decode to the restatement's maps and never the single merges'
places."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ensemble_restated as E  # noqa: E402
import live_search_restated as L  # noqa: E402
import track_restated as R  # noqa: E402
from test_gpu_live_search import SEARCH_SEED  # noqa: E402
from test_gpu_track_lockstep import _dev, _engines, _lay, _video  # noqa: E402

KS = (1, 2, 3, 4, 5, 8)
PIXELS = (1, 15, 16, 17, 37 * 53, 64 * 1024 + 5)
SETS3 = "0.25920137,0.22541801,0.0775609,0.12509281,0.3127269;1,0,0,0,0;0,0,0,1,0"      # merge.py:119's weights and two one-hot sets


def _labels(kind, K, pixels, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4 if kind == "ties" else 256, (K, pixels)).astype(np.uint8)


def _raw(maps_buf, K, stride, pixels, voted, votes, hist):
    """The entry itself, so that ``votes`` / ``hist`` can be NULL and the planes strided."""
    from premvos_amd import _lib
    _lib.check(_lib.load().premvos_idmap_vote_u8(maps_buf.data_ptr(), K, stride, pixels, voted.data_ptr(), None if votes is None else votes.data_ptr(),
                                                 None if hist is None else hist.data_ptr(), _lib.current_stream()), "idmap_vote")


def _run(maps_np, stride_extra=0, voted_offset=0, with_votes=True, with_hist=True):
    """maps uint8 [K,pixels] (host) through the entry with planes ``pixels + stride_extra`` apart and ``voted`` ``voted_offset`` bytes behind
    an aligned buffer -> (voted, votes or None, hist or None) on the host; the bytes around the outputs must stay as they were."""
    dev = _dev()
    K, pixels = maps_np.shape
    stride = pixels + stride_extra
    buf = torch.full((K * stride + 16,), 77, dtype=torch.uint8, device=dev)
    buf[:K * stride].view(K, stride)[:, :pixels] = torch.from_numpy(maps_np).to(dev)
    voted = torch.full((pixels + voted_offset + 16,), 200, dtype=torch.uint8, device=dev)
    votes = torch.full((pixels + 16,), 201, dtype=torch.uint8, device=dev) if with_votes else None
    hist = torch.zeros((K + 1,), dtype=torch.int64, device=dev) if with_hist else None
    assert buf.data_ptr() % 16 == 0 and voted.data_ptr() % 16 == 0
    _raw(buf, K, stride, pixels, voted[voted_offset:], votes, hist)
    v = voted.cpu().numpy()
    assert (v[:voted_offset] == 200).all() and (v[voted_offset + pixels:] == 200).all()         # nothing outside the output
    if votes is not None:
        assert (votes[pixels:] == 201).all()
    return (v[voted_offset:voted_offset + pixels], None if votes is None else votes[:pixels].cpu().numpy(), None if hist is None else hist.cpu().numpy())


def _check(maps_np, **how):
    want = E.vote(maps_np)
    got = _run(maps_np, **how)
    assert np.array_equal(got[0], want[0]), how
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), how
    if got[2] is not None:
        assert got[2].tolist() == want[2].tolist(), (how, got[2], want[2])
    return got


@pytest.mark.parametrize("pixels", PIXELS)
@pytest.mark.parametrize("K", KS)
def test_the_kernel_equals_the_restatement(K, pixels):
    for kind in ("ties", "bytes"):
        maps = _labels(kind, K, pixels, seed=1000 * K + pixels % 997)
        a = _check(maps)                                                                        # the 16-byte path (+ its scalar tail)
        b = _check(maps)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))                                  # two launches on zeroed hist: equal bits
        _check(maps, stride_extra=3)                                                            # unaligned planes
        _check(maps, stride_extra=-pixels % 16)                                                 # aligned planes, a partial last chunk
        _check(maps, voted_offset=1)                                                            # unaligned output
        _check(maps, with_votes=False)
        _check(maps, with_hist=False)
        _check(maps, with_votes=False, with_hist=False, stride_extra=3, voted_offset=1)
    same = np.repeat(_labels("bytes", 1, pixels, seed=K), K, axis=0)                            # K identical maps
    voted, votes, hist = _check(same)
    assert np.array_equal(voted, same[0]) and (votes == K).all() and hist[K] == pixels and hist.sum() == pixels


def test_a_stack_of_many_workgroups():
    """3 x 480 x 854 under 5 sets: 300 workgroups add into ``hist``; the wrapper on a [K,N,h,w] stack, twice."""
    from premvos_amd import track
    dev = _dev()
    rng = np.random.default_rng(5)
    maps = rng.integers(0, 4, (5, 3, 480, 854)).astype(np.uint8)
    maps[1:, :, 100:300] = maps[0, :, 100:300]                                                  # a unanimous band
    want = E.vote(maps)
    d = torch.from_numpy(maps).to(dev)
    a, b = track.vote_idmaps(d), track.vote_idmaps(d)
    for k, w in zip(("voted", "votes", "hist"), want):
        assert np.array_equal(a[k].cpu().numpy(), w) and torch.equal(a[k], b[k]), k
    assert a["voted"].shape == (3, 480, 854) and a["hist"][5] >= 3 * 200 * 854 and 0 < a["hist"][2]
    again = track.vote_idmaps(d, out=a["voted"], votes=a["votes"], hist=a["hist"])              # the entry only ADDS to hist
    assert again["hist"] is a["hist"] and a["hist"].cpu().numpy().tolist() == (2 * want[2]).tolist()
    eight = rng.integers(0, 3, (8, 480 * 854 + 7)).astype(np.uint8)                             # K = 8, aligned planes with a tail: a strided view
    planes = torch.zeros((8, 480 * 854 + 16), dtype=torch.uint8, device=dev)
    planes[:, :eight.shape[1]] = torch.from_numpy(eight).to(dev)
    got = track.vote_idmaps(planes[:, :eight.shape[1]])
    for k, w in zip(("voted", "votes", "hist"), E.vote(eight)):
        assert np.array_equal(got[k].cpu().numpy(), w), k


def test_every_tie_pattern_of_four_sets():
    """All 4^4 assignments of four labels to four sets (every partition of the sets, in every order), over {0, 1, 2, 3} and with the
    labels 0 / 255 among them: 2-2 splits, 2-1-1, all different, background against objects."""
    combos = np.array(list(itertools.product(range(4), repeat=4)), np.uint8).T                  # [4, 256]
    for table in ((0, 1, 2, 3), (255, 0, 7, 128), (3, 255, 0, 1)):
        maps = np.asarray(table, np.uint8)[combos]
        voted, votes, hist = _check(maps)
        _check(maps, stride_extra=3, voted_offset=1)
        assert hist.tolist() == [0, 24, 144 + 36, 48, 4]                                        # 4! | 6*4*3*2 + 3*4*3 | 4*4*3 | 4
        split = (maps[0] == maps[2]) & (maps[1] == maps[3]) & (maps[0] != maps[1])              # a 2-2 split: set 0's label
        assert split.sum() == 12 and np.array_equal(voted[split], maps[0][split]) and (votes[split] == 2).all()
        alone = (maps[1] == maps[2]) & (maps[2] == maps[3]) & (maps[0] != maps[1])              # three against set 0
        assert np.array_equal(voted[alone], maps[1][alone]) and (votes[alone] == 3).all()


def test_the_wrapper_refuses_what_the_entry_refuses():
    from premvos_amd import _lib, track
    dev = _dev()
    maps = torch.zeros((3, 64), dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.PremvosError, match="voted overlaps the maps"):
        track.vote_idmaps(maps, out=maps[1])
    with pytest.raises(AssertionError):
        track.vote_idmaps(torch.zeros((9, 4), dtype=torch.uint8, device=dev))
    r = track.vote_idmaps(torch.zeros((2, 0), dtype=torch.uint8, device=dev))                   # no pixel: a no-op
    assert r["voted"].shape == (0,) and r["hist"].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------- the live form
def test_the_live_ensemble_votes_its_own_members_and_they_are_the_searchs(tmp_path):
    """120x200, 5 frames, 3 objects, three weight sets (default, (1,0,0,0,0), (0,0,0,1,0)): the voted stack and ``hist`` are the
    restatement applied to the members; the members are ``search_video``'s id maps for the same sets, byte for byte (dropping the eval
    launch and adding the vote changed nothing a seat computes); the PNGs on disk decode to the voted stack."""
    from PIL import Image
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(tmp_path)
    n = 5
    _video(lay, "clip", n, 3, seed=SEARCH_SEED)
    ws = L.THREE_SETS
    r = track.ensemble_video("clip", lay, ws, ref_eng, reid_eng, record=True)
    assert r["frames"] == n and r["members"].shape == (3, n, 120, 200) and r["voted"].shape == (n, 120, 200)
    voted, _, hist = E.vote(r["members"])
    assert np.array_equal(r["voted"], voted) and r["hist"].tolist() == hist.tolist() and hist.sum() == n * 120 * 200
    print(f"unanimous {hist[3] / hist.sum():.4f}, hist {hist.tolist()}")
    assert r["members"].any() and set(np.unique(r["voted"])) <= {0, 1, 2, 3}
    s = track.search_video("clip", lay, ws, ref_eng, reid_eng, record=True)
    assert s["idmaps"].shape == r["members"].shape and s["idmaps"].tobytes() == r["members"].tobytes()
    for t in range(n):
        assert np.array_equal(np.array(Image.open(os.path.join(lay["out"], "clip", f"{t:05d}.png"))), voted[t]), t
    for v in range(3):                                                                          # as many engine calls per seat as a run makes
        calls = r["engine_logs"][v]
        assert sum(c["call"] == "refine" for c in calls) == n - 1 and sum(c["call"] == "reid" for c in calls) == n


def _live_root(root, monkeypatch):
    """A PReMVOS root whose live-loop inputs are ``_video``'s, with the reduced-depth engines behind the two ``*_net_init``."""
    from premvos_amd import track
    import premvos_amd.refinement.driver as fd
    import premvos_amd.reid.driver as qd
    ref_eng, reid_eng = _engines()
    monkeypatch.setattr(fd, "refinement_net_init", lambda: ref_eng)
    monkeypatch.setattr(qd, "ReID_net_init", lambda: reid_eng)
    lay = track._layout(str(root))
    for rel in ("code/refinement_net/configs", "code/ReID_net/configs"):
        os.makedirs(os.path.join(str(root), rel))
        open(os.path.join(str(root), rel, "live"), "w").write("{}")
    return lay


def test_the_command_on_a_tree(tmp_path, monkeypatch, capsys):
    """``track --ensemble <3 sets> --eval``: output/final_ensemble/<video>/*.png decode to ``ensemble_video``'s voted stack, a video
    without templates gets zeros, output/ensemble.json and the _ensemble summary are written, output/final/ is not."""
    from PIL import Image
    from premvos_amd import track
    root = tmp_path / "premvos"
    lay = _live_root(root, monkeypatch)
    _video(lay, "clip", 4, 2, seed=SEARCH_SEED)
    _video(lay, "void", 3, 1, seed=SEARCH_SEED + 1)
    R.write_index_png(os.path.join(lay["anns"], "void", "00000.png"), np.zeros((120, 200), np.uint8))      # no object in frame 0: no templates
    cwd = os.getcwd()
    try:
        assert track.main(["--root", str(root), "--ensemble", SETS3, "--eval"]) == 0
    finally:
        os.chdir(cwd)
    text = capsys.readouterr().out
    out = root / "output"
    assert "final_ensemble" in text and "ensemble.json" in text and not (out / "final").exists()
    ws = track.parse_ensemble_sets(SETS3)
    ref_eng, reid_eng = _engines()
    want = track.ensemble_video("clip", dict(lay, out=str(tmp_path / "again") + "/"), ws, ref_eng, reid_eng, record=True)
    assert np.array_equal(want["voted"], E.vote(want["members"])[0])
    pal = track.voc_palette().reshape(-1)
    for name, n in (("clip", 4), ("void", 3)):
        files = sorted(os.listdir(out / "final_ensemble" / name))
        assert files == [f"{t:05d}.png" for t in range(n)]
        for t, fn in enumerate(files):
            im = Image.open(out / "final_ensemble" / name / fn)
            px = np.array(im)
            assert im.mode == "P" and np.array_equal(np.array(im.getpalette(), np.uint8), pal)
            assert np.array_equal(px, want["voted"][t] if name == "clip" else np.zeros((120, 200), np.uint8)), (name, t)
    assert want["voted"].any()
    res = json.loads((out / "ensemble.json").read_text())
    assert set(res) == {"videos", "frames", "sets", "weights", "source"} and res["sets"] == 3 and res["frames"] == 7
    assert res["weights"] == ws.tolist() and res["source"] == "--ensemble" and set(res["videos"]) == {"clip", "void"}
    clip = res["videos"]["clip"]
    assert clip["frames"] == 4 and clip["hist"] == want["hist"].tolist() and clip["unanimous"] == clip["hist"][3] / (4 * 120 * 200)
    assert res["videos"]["void"] == {"frames": 3, "hist": [0, 0, 0, 3 * 120 * 200], "unanimous": 1.0}
    summary = json.loads((out / "premvos_amd_davis_eval_ensemble.json").read_text())
    assert (out / "eval_ensemble" / "clip.json").exists() and not (out / "eval_ensemble" / "void.json").exists() and summary
    assert not (out / "eval").exists() and not (out / "premvos_amd_davis_eval.json").exists()
    # --ensemble-from: the two best rows of a search result, best first
    (out / "live_search.json").write_text(json.dumps({"weights": ws.tolist(), "mean": [0.5, None, 0.75]}))
    try:
        assert track.main(["--root", str(root), "--ensemble-from", str(out / "live_search.json"), "--top", "2", "--videos", "clip"]) == 0
    finally:
        os.chdir(cwd)
    res = json.loads((out / "ensemble.json").read_text())
    assert res["weights"] == ws[[2, 0]].tolist() and res["source"].startswith("--ensemble-from") and list(res["videos"]) == ["clip"]
    two = track.ensemble_video("clip", dict(lay, out=str(tmp_path / "two") + "/"), ws[[2, 0]], ref_eng, reid_eng, record=True)
    assert np.array_equal(two["voted"], two["members"][0])                                       # K = 2: set 0 keeps every tie
    got = np.array([np.array(Image.open(out / "final_ensemble" / "clip" / f"{t:05d}.png")) for t in range(4)])
    assert np.array_equal(got, two["voted"])


# ---------------------------------------------------------------------------------------------------------------- the pre-warp form
def test_the_prewarp_ensemble_on_the_fixture_tree(tmp_path, monkeypatch, capsys):
    """``track --prewarp --ensemble``: the PNGs are the restatement over ``prewarp.merge_video(..., weights=w_k)``'s id maps, k = 0 .. 2;
    output/final_prewarp/ is not written."""
    from PIL import Image
    from test_gpu_prewarp import _stub_engines, _write_tree
    from premvos_amd import prewarp as pw, track
    root = str(tmp_path)
    _write_tree(root, ("alpha", "beta"))
    _stub_engines(monkeypatch)
    sets = "0.1639026729185494,0.3090363324359478,0.11728252456485666,0.18345061062541546,0.2263278594552307;1,0,0,0,0;0,0,0,1,1"
    assert track.main(["--root", root, "--prewarp", "--ensemble", sets, "--late-annotations", "--eval"]) == 0
    text = capsys.readouterr().out
    assert "final_prewarp_ensemble" in text and "prewarp_ensemble.json" in text
    out = os.path.join(root, "output")
    assert not os.path.exists(os.path.join(out, "final_prewarp")) and not os.path.exists(os.path.join(out, "final"))
    assert not os.path.exists(os.path.join(out, "eval_prewarp")) and os.path.isfile(os.path.join(out, "premvos_amd_davis_eval_prewarp_ensemble.json"))
    ws = track.parse_ensemble_sets(sets)
    res = json.load(open(os.path.join(out, "prewarp_ensemble.json")))
    assert res["sets"] == 3 and res["source"] == "--ensemble" and res["weights"] == [pw.normalised(w).tolist() for w in ws]
    lay = track._layout(root)
    add_reid = track._default_engine_calls(None, None)[1]
    for name in ("alpha", "beta"):
        frames, (h, w), fns, _ = pw.read_video(name, lay, True, add_reid, None)
        members = np.array([pw.merge_video(frames, h, w, weights=ws[k])["idmap_dev"].cpu().numpy() for k in range(3)])
        voted, _, hist = E.vote(members)
        got = np.array([np.array(Image.open(os.path.join(out, "final_prewarp_ensemble", name, os.path.basename(fn)[:-4] + ".png"))) for fn in fns])
        assert np.array_equal(got, voted), name
        assert res["videos"][name]["hist"] == hist.tolist() and res["videos"][name]["frames"] == len(fns)
        print(f"{name}: unanimous {res['videos'][name]['unanimous']:.4f}")
        assert os.path.isfile(os.path.join(out, "eval_prewarp_ensemble", name + ".json"))
        r = pw.ensemble_video(frames, h, w, ws, record=True)                                    # the library form: members and hist
        assert np.array_equal(r["members"].cpu().numpy(), members) and r["hist"].cpu().numpy().tolist() == hist.tolist()


# ------------------------------------------------------------------------------------------------------------------- the tree tool
def test_the_tree_tool_votes_png_trees(tmp_path, capsys):
    from PIL import Image
    from premvos_amd import ensemble
    root = str(tmp_path)
    rng = np.random.default_rng(3)
    n, h, w = 4, 37, 53
    base = np.zeros((n, h, w), np.uint8)
    for t in range(n):
        base[t, 5:20, 4 + t:30 + t] = 1
        base[t, 15:33, 25:50 - t] = 2
    trees = []
    for k, name in enumerate(("t0", "t1", "t2")):
        m = base.copy()
        ys, xs = rng.integers(0, h, 60), rng.integers(0, w, 60)
        m[rng.integers(0, n, 60), ys, xs] = rng.integers(0, 4, 60)                             # a few pixels differ per tree
        if k == 2:
            m[:, 0, 0] = 255
        trees.append(m)
        for t in range(n):
            os.makedirs(os.path.join(root, "output", name, "vid"), exist_ok=True)
            R.write_index_png(os.path.join(root, "output", name, "vid", f"{t:05d}.png"), m[t])
    for t in range(n):
        os.makedirs(os.path.join(root, "data/DAVIS/Annotations/480p/vid"), exist_ok=True)
        R.write_index_png(os.path.join(root, "data/DAVIS/Annotations/480p/vid", f"{t:05d}.png"), base[t])
    assert ensemble.main(["--root", root, "--inputs", "t0,t1,t2", "--eval"]) == 0
    assert "final_vote" in capsys.readouterr().out
    voted, _, hist = E.vote(np.array(trees))
    got = np.array([np.array(Image.open(os.path.join(root, "output", "final_vote", "vid", f"{t:05d}.png"))) for t in range(n)])
    assert np.array_equal(got, voted) and not np.array_equal(voted, trees[0]) and hist[3] < n * h * w
    res = json.load(open(os.path.join(root, "output", "final_vote.json")))
    assert res["videos"]["vid"] == {"frames": n, "hist": hist.tolist(), "unanimous": hist[3] / (n * h * w)} and res["weights"] is None
    assert res["source"] == ["output/t0", "output/t1", "output/t2"] and res["sets"] == 3
    assert os.path.isfile(os.path.join(root, "output", "eval_final_vote", "vid.json"))
    assert os.path.isfile(os.path.join(root, "output", "premvos_amd_davis_eval_final_vote.json"))
    assert ensemble.main(["--root", root, "--inputs", "t2,t1,t0", "--out", "other"]) == 0      # another priority, another place
    got = np.array([np.array(Image.open(os.path.join(root, "output", "other", "vid", f"{t:05d}.png"))) for t in range(n)])
    assert np.array_equal(got, E.vote(np.array(trees[::-1]))[0]) and not os.path.exists(os.path.join(root, "output", "eval_other"))
