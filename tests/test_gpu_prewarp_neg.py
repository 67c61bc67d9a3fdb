"""Negative first-frame templates of the pre-warp merge on the GPU (``--negatives``; premvos_prewarp_negatives_i32,
premvos_prewarp_gather_neg_u8, premvos_prewarp_chain_neg_f64, premvos_prewarp_paint_neg_bits_u8) against the numpy restatement
(tests/prewarp_neg_restated.py) and against what oldmerge.py computed with use_ff_negative_props = True (tests/golden/prewarp_neg_ref.npz)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prewarp_neg_restated as RN  # noqa: E402
import prewarp_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu
REF = np.load(os.path.join(HERE, "golden", "prewarp_neg_ref.npz"), allow_pickle=False)
G = json.load(open(os.path.join(HERE, "golden", "prewarp_neg_host_refs.json")))
MARGIN = 1e-6
SCORES = np.array([0.9, 0.75, 0.5, 0.25])                                                       # 4 distinct values: the stable tie order decides


# ---------------------------------------------------------------------------------------------------------------- the selection
def _selection_case(seed, h, w, P0, A0):
    """-> (masks [P0,h,w], annotations [A0,h,w], scores [P0], tail: rows of the pool (annotations first) that get bits beyond h*w)"""
    rng = np.random.default_rng(seed)
    ann = np.zeros((A0, h, w), np.uint8)
    for a in range(A0):
        y, x = 2 + 9 * a, 3 + 11 * a
        ann[a, y:y + 6, x:x + 7] = 1
    m = np.zeros((P0, h, w), np.uint8)
    for p in range(P0):
        y, x = rng.integers(0, h - 3), rng.integers(0, w - 3)
        m[p, y:y + rng.integers(1, 4), x:x + rng.integers(1, 4)] = 1
    tail = []
    if P0 >= 4 and A0 >= 1:
        m[0] = 0
        m[0, 1:3, 1:4] = 1                                     # touches annotation 0 by exactly one pixel, (2, 3)
        m[1] = 0
        m[1, h - 1, w - 4:w] = 1                               # touches nothing but, in the pool, annotation 0's bits beyond h*w
        m[2] = 0                                               # the empty mask ...
        tail = [0, A0 + 1, A0 + 2]                             # ... whose row also has bits beyond h*w
        assert int((m[0] & ann[0]).sum()) == 1 and not (m[1] & ann).any()
    scores = SCORES[rng.integers(0, 4, P0)]
    if P0 >= 4:
        scores[1] = scores[2] = SCORES[0]                      # among the first the walk sees
    return m, ann, scores, tail


def _select_on_gpu(m, ann, scores, tail, K, h, w):
    import torch
    from premvos_amd import _lib, prewarp as pw
    P0, A0, hw = len(m), len(ann), h * w
    rows = pw.pack_bits_host(np.concatenate([ann, m]) if P0 + A0 else np.zeros((0, h, w), np.uint8))
    for r in tail:                                                                              # bits beyond h*w: they do not count
        bits = np.unpackbits(rows[r], bitorder="little")
        bits[hw:] = 1
        rows[r] = np.packbits(bits, bitorder="little")
    dev = _lib.resolve_device(None)
    pool = torch.zeros((max(P0 + A0, 1), pw.row_bytes(hw)), dtype=torch.uint8, device=dev)
    if P0 + A0:
        pool[:] = torch.from_numpy(rows).to(dev)
    score = torch.from_numpy(np.ascontiguousarray(scores, np.float64)).to(dev) if P0 else torch.zeros((1,), dtype=torch.float64, device=dev)
    out = []
    for _ in range(2):                                                                          # two launches: equal bytes
        buf = torch.full((P0 + 1,), 77, dtype=torch.int32, device=dev)
        conflict = torch.empty((max(P0 * (A0 + P0), 1),), dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().premvos_prewarp_negatives_i32(pool.data_ptr(), pool.shape[0], pool.shape[1], hw, A0, P0, 0, A0, score.data_ptr(), K,
                                                             conflict.data_ptr(), buf.data_ptr(), buf.data_ptr() + 4 * P0, _lib.current_stream()),
                   "prewarp_negatives")
        out.append(buf.cpu().numpy())
    assert np.array_equal(out[0], out[1])
    return out[0][:P0], int(out[0][P0])


@pytest.mark.parametrize("h,w", ((33, 47), (40, 56)))
def test_selection_against_the_restatement(h, w):
    took_tail = took_any = 0
    for P0 in (0, 1, 70, 256):
        for A0 in (0, 1, 3):
            m, ann, scores, tail = _selection_case(100 * P0 + A0, h, w, P0, A0)
            if (h * w) % 64 == 0:
                tail = []                                                                       # (no bits beyond h*w in this size)
            for K in (-1, 0, 2):
                taken, count = _select_on_gpu(m, ann, scores, tail, K, h, w)
                want = RN.select_negatives(m, list(ann), scores, None if K < 0 else K)
                assert count == len(want) and taken[:count].tolist() == want and (taken[count:] == -1).all(), (P0, A0, K, taken[:count].tolist(), want)
                if K < 0 and tail:
                    assert 0 not in want and 1 in want and 2 in want                            # one pixel refuses; bits beyond h*w do not; empty is taken
                    took_tail += 1
                took_any += count
    assert took_any and (took_tail or (h * w) % 64 == 0)


def test_selection_nan_scores_and_a_full_frame():
    h, w = 480, 854
    rng = np.random.default_rng(5)
    m, ann = np.zeros((40, h, w), np.uint8), np.zeros((3, h, w), np.uint8)
    for a in range(3):
        ann[a, 50 + 120 * a:150 + 120 * a, 100:400] = 1
    for p in range(40):
        y, x = rng.integers(0, h - 60), rng.integers(0, w - 80)
        m[p, y:y + rng.integers(10, 60), x:x + rng.integers(10, 80)] = 1
    m[7] = 0
    m[7, h - 1, w - 1] = 1                                                                      # the very last pixel
    scores = SCORES[rng.integers(0, 4, 40)].copy()
    scores[[3, 11]] = np.nan                                                                    # never taken
    m[3] = 0                                                                                    # ... even where nothing is in its way
    taken, count = _select_on_gpu(m, ann, scores, [], -1, h, w)
    want = RN.select_negatives(m, list(ann), scores)
    assert taken[:count].tolist() == want and 3 not in want and 11 not in want and 7 in want and count >= 3


# ------------------------------------------------------------------------------------------------------- chain, paint and the gather
def _fixture_frames(name, late=True):
    frames = RN.fixture_video(REF, G, name, late)
    for f in frames:
        f["emb"] = f["reid"]
    return frames


def _margins_ok(frames, out, h, w):
    """the fixtures' condition for a video with negatives: every first maximum that is taken is MARGIN away from the runner-up, or
    exactly equal (the exact zeros of rows nothing snapped to: the equal-score rule orders them)"""
    T = out["chosen"].shape[1]
    flat = [o for f in frames for o in f["ann"]]
    for t, f in enumerate(frames):
        wt, P = out["weighted"][t], len(f["score"])
        if not P:
            continue
        if not np.isfinite(wt).all() or (np.sort(wt, axis=0)[-1] - np.sort(wt, axis=0)[-2]).min() < MARGIN:
            return False
        closest = np.argmax(wt, axis=0)
        for k in range(T):
            row = wt[k] * (closest == k)
            if row.any() and P > 1 and (np.sort(row)[-1] - np.sort(row)[-2]) < MARGIN:
                return False
        ch = out["chosen"][t]
        sel = [None if ch[k] < 0 else f["mask"][ch[k]] if ch[k] < P else flat[k]["mask"] for k in range(T)]
        for a in range(T):
            for b in range(a + 1, T):
                if sel[a] is not None and sel[b] is not None and (sel[a] & sel[b]).any() and 0 < abs(out["best"][t, a] - out["best"][t, b]) < MARGIN:
                    return False
    return True


_CACHE = {}


def _random_video():
    """12 frames of 33 x 47, P_t <= 9, 2 objects + a late one, at least 2 negatives, under the margin condition; with its restated result"""
    if "v" not in _CACHE:
        from test_gpu_prewarp import _draw
        h, w = 33, 47
        for seed in range(1000):
            frames = _draw(seed, [0, 0, 4], [9, 7, 8, 9, 5, 9, 6, 9, 9, 4, 8, 9], h, w)
            out = RN.merge_video(frames, h, w, negatives="all")
            if len(out["negatives"]) >= 2 and _margins_ok(frames, out, h, w):
                break
        else:
            raise AssertionError("no seed meets the margin condition: look at the generator")
        _CACHE["v"] = (frames, h, w, out)
    return _CACHE["v"]


def _cases():
    return [("alpha",) + (_fixture_frames("alpha"), G["h"], G["w"]), ("beta",) + (_fixture_frames("beta"), G["h"], G["w"]), ("random",) + _random_video()[:3]]


def test_gather_chain_and_paint_against_the_restatement():
    import torch
    from premvos_amd import prewarp as pw
    for name, frames, h, w in _cases():
        want = RN.merge_video(frames, h, w, G["weights"] if name != "random" else None, negatives="all")
        weights = pw.normalised(G["weights"] if name != "random" else None)
        dv = pw.upload(frames, h, w, negatives="all")
        tab = dv.tab
        n = len(want["negatives"])
        assert dv.negatives == want["negatives"] and (tab.n_neg, tab.T_ann, tab.T) == (n, want["T_ann"], want["T_ann"] + n) and n >= 2, name
        assert tab.blocks[0].tolist()[2:6] == [tab.ann0, len(frames[0]["ann"]), tab.neg0, n] and tab.S == tab.neg0 + n
        # the gather: the negatives' pool rows and embeddings are the proposals'
        pool, emb_t, emb_p = dv.pool.cpu().numpy(), dv.emb_t.cpu().numpy(), dv.emb_p.cpu().numpy()
        for j, p in enumerate(dv.negatives):
            assert np.array_equal(pool[tab.neg0 + j], pool[tab.cur0 + p]) and np.array_equal(emb_t[tab.T_ann + j], emb_p[p]), (name, j)
        assert np.array_equal(pw.unpack_bits_host(pool[tab.neg0:tab.neg0 + n], h, w), np.asarray(frames[0]["mask"])[dv.negatives])
        dv.prepare()
        c = dv.chain(weights[None], want_weighted=True)
        assert np.array_equal(c["chosen"][0].cpu().numpy(), want["chosen"]), name
        assert np.abs(c["best"][0].cpu().numpy() - want["best"]).max() <= 1e-12
        flat = np.concatenate([x.reshape(-1) for x in want["weighted"]])
        assert np.abs(c["weighted"][:len(flat)].cpu().numpy() - flat).max() <= 1e-12 and len(flat) == tab.T * tab.sumP
        assert (want["chosen"][:, tab.T_ann:] < np.diff(tab.poff)[:, None]).all()               # a negative is forced in no frame
        idmap, _ = dv.paint(c["chosen"], c["best"])
        assert np.array_equal(idmap.cpu().numpy(), want["idmap"]), name
        T0 = len(frames[0]["ann"])
        gt = REF[f"v_{name}_gt"] if name != "random" else np.random.default_rng(1).integers(0, T0 + 2, (len(frames), h, w)).astype(np.uint8)
        _, counts = dv.paint(c["chosen"], c["best"], idmap=False, gt_bits=pw.gt_bit_planes(gt, T0, dv.dev), T0=T0)
        assert np.array_equal(counts.cpu().numpy()[0], R.region_counts(want["index"], gt, T0)), name
        again = dv.chain(weights[None])                                                         # two launches: equal bits
        assert torch.equal(again["chosen"], c["chosen"]) and torch.equal(again["best"].view(torch.int64), c["best"].view(torch.int64))


def test_with_no_negatives_the_new_entries_give_the_old_entries_bytes():
    import torch
    from premvos_amd import _lib, prewarp as pw
    ref = np.load(os.path.join(HERE, "golden", "prewarp_ref.npz"), allow_pickle=False)         # the existing fixture
    g = json.load(open(os.path.join(HERE, "golden", "prewarp_host_refs.json")))
    for name in ("alpha", "beta"):
        frames = R.fixture_video(ref, g, name)
        for f in frames:
            f["emb"] = f["reid"]
        dv = pw.upload(frames, g["h"], g["w"])
        dv.prepare()
        tab, lib = dv.tab, _lib.load()
        old = dv.chain(pw.normalised()[None], want_weighted=True)
        old_map, _ = dv.paint(old["chosen"], old["best"])
        wd = torch.from_numpy(pw.normalised()[None].copy()).to(dv.dev)
        chosen, best, weighted = torch.full_like(old["chosen"], -7), torch.full_like(old["best"], -7.0), torch.full_like(old["weighted"], -7.0)
        _lib.check(lib.premvos_prewarp_chain_neg_f64(
            dv.inter.data_ptr(), tab.n_inter, dv.areas.data_ptr(), tab.n_areas, tab.blocks.ctypes.data, dv.blocks_dev.data_ptr(), tab.poff.ctypes.data,
            dv.poff_dev.data_ptr(), tab.first.ctypes.data, dv.first_dev.data_ptr(), tab.N, tab.T, 0, dv.score.data_ptr(), dv.reid.data_ptr(),
            dv.oreid.data_ptr(), wd.data_ptr(), 1, chosen.data_ptr(), best.data_ptr(), weighted.data_ptr(), _lib.current_stream()), "chain_neg")
        assert torch.equal(chosen, old["chosen"]) and torch.equal(best.view(torch.int64), old["best"].view(torch.int64))
        assert torch.equal(weighted.view(torch.int64), old["weighted"].view(torch.int64))
        im = torch.full_like(old_map, 99)
        _lib.check(lib.premvos_prewarp_paint_neg_bits_u8(
            dv.pool.data_ptr(), dv.pool.shape[0], dv.pool.shape[1], dv.hw, tab.blocks.ctypes.data, dv.blocks_dev.data_ptr(), tab.first.ctypes.data,
            dv.first_dev.data_ptr(), dv.ids_dev.data_ptr(), tab.ann0, chosen.data_ptr(), best.data_ptr(), tab.N, tab.T, 0, 1, im.data_ptr(), None, 0, None,
            _lib.current_stream()), "paint_neg")
        assert torch.equal(im, old_map) and np.array_equal(old_map.cpu().numpy(), ref[f"v_{name}_png"])
        # negatives asked for but none wanted (K = 0): today's tables, today's bytes
        zero = pw.merge_video(frames, g["h"], g["w"], negatives=0)
        zero["ready"].synchronize()
        assert zero["negatives"] == [] and np.array_equal(zero["idmap"].numpy(), ref[f"v_{name}_png"])


@pytest.mark.parametrize("name", ("alpha", "beta"))
def test_merge_video_with_negatives_reproduces_the_reference(name):
    from premvos_amd import prewarp as pw
    frames = _fixture_frames(name)
    r = pw.merge_video(frames, G["h"], G["w"], G["weights"], negatives="all", record=True)
    r["ready"].synchronize()
    assert r["negatives"] == REF[f"v_{name}_negatives"].tolist()
    assert np.array_equal(r["idmap"].numpy(), REF[f"v_{name}_png"]) and not np.array_equal(r["idmap"].numpy(), REF[f"v_{name}_png_off"])
    assert np.array_equal(r["chosen"][0].cpu().numpy(), REF[f"v_{name}_chosen"])
    assert np.abs(r["best"][0].cpu().numpy() - REF[f"v_{name}_best"]).max() <= 1e-12
    s = pw.search(_fixture_frames(name), G["h"], G["w"], REF[f"v_{name}_gt"], pw.normalised(G["weights"])[None], negatives="all")
    assert np.array_equal(s["scores"][0], REF[f"v_{name}_eval"]) and s["negatives"] == r["negatives"]      # eval_video's scores, exactly
    off = pw.merge_video(frames, G["h"], G["w"], G["weights"])                                  # without the flag: the other run's PNGs
    off["ready"].synchronize()
    assert off["negatives"] == [] and np.array_equal(off["idmap"].numpy(), REF[f"v_{name}_png_off"])
    two = pw.merge_video(frames, G["h"], G["w"], G["weights"], negatives=2)                     # the cap: the first two of the walk
    two["ready"].synchronize()
    want = RN.merge_video(frames, G["h"], G["w"], G["weights"], negatives=2)
    assert two["negatives"] == want["negatives"] == r["negatives"][:2] and np.array_equal(two["idmap"].numpy(), want["idmap"])
    none = [dict(f, ann=[]) for f in frames]                                                    # no annotated object: zero maps, no negatives
    z = pw.merge_video(none, G["h"], G["w"], negatives="all")
    assert z["negatives"] == [] and not z["idmap"].numpy().any()


def test_too_many_templates_are_refused_with_the_hint():
    from premvos_amd import _lib, prewarp as pw
    h, w, P0 = 16, 24, 70
    m = np.zeros((P0, h, w), np.uint8)
    for p in range(P0):
        m[p, 2 + p // 12 * 2, p % 12 * 2] = 1                                                   # 70 single pixels, none touching another
    ann = np.zeros((h, w), np.uint8)
    ann[0, 0] = 1
    emb = np.random.default_rng(0).standard_normal((P0, R.EMB))
    frames = [{"score": np.linspace(0.9, 0.1, P0), "mask": m, "fwd": m, "emb": emb, "ann": [{"id": 1, "mask": ann, "fwd": ann, "reid": emb[0]}]}]
    with pytest.raises(_lib.PremvosError, match="pass --negatives K"):
        pw.upload(frames, h, w, negatives="all")                                                # 1 + 70 templates
    dv = pw.upload(frames, h, w, negatives=63)                                                  # 1 + 63 = the cap
    assert dv.tab.T == 64 and dv.negatives == list(range(63))


# ------------------------------------------------------------------------------------------------------------------------ trees
def _png_stack(root, sub, name, n=5):
    from PIL import Image
    return np.array([np.array(Image.open(os.path.join(root, "output", sub, name, f"{t:05d}.png"))) for t in range(n)])


def test_track_prewarp_negatives_on_the_fixture_tree(tmp_path, monkeypatch, capsys):
    import test_gpu_prewarp as TP
    from premvos_amd import track
    monkeypatch.setattr(TP, "REF", REF)                                                         # its tree writer and engine stub, on this fixture
    monkeypatch.setattr(TP, "G", G)
    root = str(tmp_path)
    TP._write_tree(root, ("alpha", "beta"))
    TP._stub_engines(monkeypatch)
    before = TP._tree_state(root, ("output/intermediate",))
    assert track.main(["--root", root, "--prewarp", "--negatives", "--late-annotations"]) == 0
    assert "final_prewarp_neg" in capsys.readouterr().out
    listed = json.load(open(os.path.join(root, "output", "prewarp_negatives.json")))
    assert listed["negatives"] == "all"
    for name in ("alpha", "beta"):
        want = RN.merge_video(RN.fixture_video(REF, G, name), G["h"], G["w"], negatives="all")
        got = _png_stack(root, "final_prewarp_neg", name)
        assert np.array_equal(got, want["idmap"]) and np.array_equal(got, REF[f"v_{name}_png"]), name
        v = listed["videos"][name]
        assert v["candidates"] == 9 and v["taken"] == want["negatives"] and v["templates"] == want["chosen"].shape[1]
        assert v["scores"] == [float(REF[f"v_{name}_score"][0][i]) for i in want["negatives"]]
    out = os.path.join(root, "output")
    assert not os.path.exists(os.path.join(out, "final_prewarp")) and not os.path.exists(os.path.join(out, "final"))
    assert TP._tree_state(root, ("output/intermediate",)) == before
    # the cap, and the search: set 0 = the single pass's scores = the reference's eval_video
    assert track.main(["--root", root, "--prewarp", "--negatives", "1", "--late-annotations", "--videos", "beta"]) == 0
    want = RN.merge_video(RN.fixture_video(REF, G, "beta"), G["h"], G["w"], negatives=1)
    assert np.array_equal(_png_stack(root, "final_prewarp_neg", "beta"), want["idmap"])
    assert json.load(open(os.path.join(out, "prewarp_negatives.json")))["videos"]["beta"]["taken"] == want["negatives"]
    assert track.main(["--root", root, "--prewarp-search", "4", "--negatives", "--late-annotations"]) == 0
    r = json.load(open(os.path.join(out, "prewarp_neg_search.json")))
    ws = R.search_weights(4, 0)
    for name in ("alpha", "beta"):
        scores = np.array(r["videos"][name]["scores"])
        assert np.array_equal(scores[0], REF[f"v_{name}_eval"]), name
        frames = RN.fixture_video(REF, G, name)
        for i in range(4):
            idx = RN.merge_video(frames, G["h"], G["w"], ws[i], negatives="all")["index"]
            assert np.array_equal(scores[i], R.eval_video(idx, REF[f"v_{name}_gt"], len(frames[0]["ann"]))), (name, i)
    assert not os.path.exists(os.path.join(out, "prewarp_search.json"))
    # the ensemble: two sets, under its own names
    assert track.main(["--root", root, "--prewarp", "--negatives", "--late-annotations", "--ensemble", "1,1,1,1,1;" + ",".join(map(str, G["weights"]))]) == 0
    ens = json.load(open(os.path.join(out, "prewarp_neg_ensemble.json")))
    assert set(ens["videos"]) == {"alpha", "beta"} and _png_stack(root, "final_prewarp_neg_ensemble", "alpha").shape == (5, G["h"], G["w"])
    for gone in ("final_prewarp", "final", "final_prewarp_ensemble", "prewarp_ensemble.json"):
        assert not os.path.exists(os.path.join(out, gone)), gone


def test_stream_track_prewarp_negatives_writes_the_pngs_of_track_prewarp_negatives(tmp_path):
    """`stream --track --prewarp --negatives`, then `track --prewarp --negatives` on the tree the same run wrote: equal PNG bytes.  The
    annotated objects are small boxes in the frame's corners, so that proposals stay clear of them and negatives are taken."""
    import shutil
    import test_gpu_stream_prewarp as SP
    root = tmp_path / "a"
    SP._tree(root, {"bear": 5, "camel": 3})
    small = {"bear": np.zeros((120, 200), np.uint8), "camel": np.zeros((120, 200), np.uint8)}
    small["bear"][0:12, 0:14], small["bear"][108:120, 186:200], small["camel"][0:12, 186:200] = 1, 2, 1
    for name, ann in small.items():
        SP.R.write_index_png(str(root / "data" / "DAVIS" / "Annotations" / "480p" / name / "00000.png"), ann)
    out = SP._child("premvos_amd.stream", root, "--batch", "2", "--track", "--prewarp", "--negatives", *SP.T.STREAM_ARGS).stdout
    assert "frames: 8" in out
    o = root / "output"
    assert not (o / "final_prewarp").exists() and not (o / "final").exists()
    listed = json.load(open(o / "prewarp_negatives.json"))
    assert listed["negatives"] == "all" and set(listed["videos"]) == {"bear", "camel"}
    print("candidates / taken per video:", {k: (v["candidates"], v["taken"]) for k, v in listed["videos"].items()})
    assert any(v["taken"] for v in listed["videos"].values()), "no video took a negative: the comparison would show nothing of them"
    shutil.move(str(o / "final_prewarp_neg"), str(o / "streamed"))
    SP._child("premvos_amd.track", root, "--prewarp", "--negatives")
    files = SP._files(o / "streamed")
    assert files == SP._files(o / "final_prewarp_neg") == [f"bear/{t:05d}.png" for t in range(5)] + [f"camel/{t:05d}.png" for t in range(3)]
    for f in files:
        assert (o / "streamed" / f).read_bytes() == (o / "final_prewarp_neg" / f).read_bytes(), f
    again = json.load(open(o / "prewarp_negatives.json"))
    for name in ("bear", "camel"):
        assert again["videos"][name]["taken"] == listed["videos"][name]["taken"] and again["videos"][name]["templates"] == listed["videos"][name]["templates"]
