"""premvos_amd/csrc/prewarp_ops.hip and premvos_amd/prewarp.py on the GPU against tests/prewarp_restated.py (numpy) and against what
MergeTrack/oldmerge.py itself wrote (tests/golden/prewarp_ref.npz).  Inputs are drawn under the fixture's margin condition: the seed
is advanced until column maxima, row maxima and overlapping selections are 1e-6 apart, so another summation order cannot flip a
selection; the planes themselves are held to 1e-12 (numpy's dot order), selections, id maps and integer counts exactly."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prewarp_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu
REF = np.load(os.path.join(HERE, "golden", "prewarp_ref.npz"), allow_pickle=False)
G = json.load(open(os.path.join(HERE, "golden", "prewarp_host_refs.json")))
MARGIN = 1e-6


# ------------------------------------------------------------------------------------------------------------------------- overlap
def _popcount_ref(masks, blocks):
    inter, areas = [], []
    for a0, na, b0, nb, c0, nc, io, ao in blocks:
        hw = masks.shape[1] * masks.shape[2]
        a = masks[a0:a0 + na].reshape(na, hw).astype(np.int64)
        b = np.concatenate([masks[b0:b0 + nb], masks[c0:c0 + nc]]).reshape(nb + nc, hw).astype(np.int64)
        assert io == sum(len(x) for x in inter) and ao == sum(len(x) for x in areas)
        inter.append((a @ b.T).reshape(-1))
        areas.append(np.concatenate([a.sum(1), b.sum(1)]))
    return np.concatenate(inter), np.concatenate(areas)


def _blocks(shapes):
    """(a0, na, b0, nb, c0, nc) rows -> the table with its running offsets"""
    rows, io, ao = [], 0, 0
    for a0, na, b0, nb, c0, nc in shapes:
        rows.append((a0, na, b0, nb, c0, nc, io, ao))
        io, ao = io + na * (nb + nc), ao + na + nb + nc
    return np.array(rows, np.int32).reshape(-1, 8), io, ao


@pytest.mark.parametrize("h,w", ((40, 56), (33, 47), (480, 854)))
def test_overlap_against_numpy_popcounts(h, w):
    import torch
    from premvos_amd import prewarp as pw
    rng = np.random.default_rng(h)
    S = 90
    masks = (rng.random((S, h, w)) < rng.uniform(0.05, 0.6, (S, 1, 1))).astype(np.uint8)
    masks[3] = 0
    bits = pw.pack_bits_host(masks)
    hw = h * w
    if hw % 64:                                                                      # bits beyond h*w must not count: set them all
        bits[:, hw // 8] |= (0xFF << (hw % 8)) & 0xFF if hw % 8 else 0
        bits[:, (hw + 7) // 8:] = 0xFF
    pool = torch.from_numpy(bits).cuda()
    for shapes in ([(0, 1, 1, 1, 0, 0)], [(0, 40, 40, 41, 0, 0)],
                   [(0, 7, 20, 3, 0, 0), (7, 0, 0, 7, 81, 2), (7, 5, 30, 0, 0, 0), (12, 17, 40, 5, 88, 2), (29, 0, 0, 0, 0, 0), (29, 33, 45, 16, 3, 1)]):
        blocks, io, ao = _blocks(shapes)
        inter, areas = pw.bits_overlap(pool, hw, blocks, io, ao)
        want_i, want_a = _popcount_ref(masks, blocks.tolist())
        assert np.array_equal(inter.cpu().numpy(), want_i) and np.array_equal(areas.cpu().numpy(), want_a), shapes
        again = pw.bits_overlap(pool, hw, blocks, io, ao)
        assert torch.equal(again[0], inter) and torch.equal(again[1], areas)


# ------------------------------------------------------------------------------------------------------------------ random videos
def _draw(seed, starts, P, h, w, ids=None, no_reid=()):
    rng = np.random.default_rng(seed)
    T = len(starts)
    units = rng.standard_normal((T + 3, R.EMB))
    yy, xx = np.mgrid[:h, :w]

    def blob(cy, cx, ry, rx):
        return ((np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)).astype(np.uint8)
    centre = np.stack([rng.integers(2, h - 2, T), rng.integers(2, w - 2, T)], 1)
    frames = []
    for t, n in enumerate(P):
        who = rng.integers(0, T + 3, n)
        mask = np.zeros((n, h, w), np.uint8)
        for p in range(n):
            cy, cx = centre[who[p]] if who[p] < T else (rng.integers(0, h), rng.integers(0, w))
            mask[p] = blob(cy + rng.integers(-2, 3), cx + rng.integers(-2, 3), rng.integers(1, 5), rng.integers(1, 6))
        fwd = np.roll(mask, 1, axis=2)
        emb = units[who] + 0.3 * rng.standard_normal((n, R.EMB))
        for (tt, p) in no_reid:
            if tt == t:
                emb[p] = np.inf
        ann = [{"id": (ids[k] if ids else k + 1), "mask": blob(*centre[k], 3, 4), "fwd": np.roll(blob(*centre[k], 3, 4), 1, axis=1), "reid": units[k]}
               for k in range(T) if starts[k] == t]
        frames.append({"score": np.round(rng.uniform(0.2, 1.0, n), 3), "mask": mask, "fwd": fwd, "reid": emb, "emb": emb, "ann": ann})
    return frames


def _margins_ok(frames, out, h, w, weights):
    ids, start, _, first = R.templates_of(frames)
    T = len(ids)
    flat = [o for f in frames for o in f["ann"]]
    for t, f in enumerate(frames):
        wt, P = out["weighted"][t], len(f["score"])
        if not P:
            continue
        if not np.isfinite(wt).all():
            return False
        if T > 1 and (np.sort(wt, axis=0)[-1] - np.sort(wt, axis=0)[-2]).min() < MARGIN:
            return False
        closest = np.argmax(wt, axis=0)
        for k in range(T):
            row = wt[k] * (closest == k)
            if row.any() and P > 1 and (np.sort(row)[-1] - np.sort(row)[-2]) < MARGIN:
                return False
        sel = [None if out["chosen"][t, k] < 0 else f["mask"][out["chosen"][t, k]] if out["chosen"][t, k] < P else flat[k]["mask"] for k in range(T)]
        for a in range(T):
            for b in range(a + 1, T):
                if sel[a] is not None and sel[b] is not None and (sel[a] & sel[b]).any() and 0 < abs(out["best"][t, a] - out["best"][t, b]) < MARGIN:
                    # (exactly equal scores -- the exact zeros of rows nothing snapped to, the exact ones of annotations -- are no
                    # matter of rounding: the equal-score rule orders them)
                    return False
    return True


_CACHE = {}


def _case(name, weights=None):
    """a video drawn under the margin condition for ``weights`` (every row of it), with its restated result: computed once, shared"""
    if name in _CACHE:
        return _CACHE[name]
    spec = {"T1": dict(starts=[0], P=[5, 9, 4, 6], h=16, w=24),
            "T3late": dict(starts=[0, 0, 2], P=[7, 7, 7, 7, 7], h=16, w=24, no_reid=((1, 2), (3, 0))),
            "empty": dict(starts=[0, 1], P=[6, 0, 5, 0, 0, 4], h=11, w=13, ids=[1, 2]),
            "big": dict(starts=[0] * 30 + [1] * 10, P=[128, 128, 128], h=24, w=40)}[name]
    ws = R.search_weights(7, 5) if weights is None else weights
    h, w = spec["h"], spec["w"]
    for seed in range(1000):
        frames = _draw(seed, spec["starts"], spec["P"], h, w, spec.get("ids"), spec.get("no_reid", ()))
        outs = [R.merge_video(frames, h, w, x) for x in (ws if name != "big" else ws[:1])]
        if all(_margins_ok(frames, o, h, w, x) for o, x in zip(outs, ws)):
            break
    else:
        raise AssertionError("no seed meets the margin condition: look at the generator")
    _CACHE[name] = (frames, h, w, ws[:len(outs)], outs)
    return _CACHE[name]


def _flat(per_frame, T):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in per_frame]) if per_frame else np.zeros(0)


@pytest.mark.parametrize("name", ("T1", "T3late", "empty", "big"))
def test_reid_and_chain_against_the_restatement(name):
    import torch
    from premvos_amd import prewarp as pw
    frames, h, w, ws, outs = _case(name)
    dv = pw.upload(frames, h, w)
    dv.prepare()
    reid, oreid = R.reid_planes(frames)
    T, n = dv.tab.T, dv.tab.T * dv.tab.sumP
    assert np.abs(dv.reid[:n].cpu().numpy() - _flat(reid, T)).max() <= 1e-12 and np.abs(dv.oreid[:n].cpu().numpy() - _flat(oreid, T)).max() <= 1e-12
    one = dv.chain(ws[:1], want_weighted=True)
    assert np.array_equal(one["chosen"][0].cpu().numpy(), outs[0]["chosen"])
    assert np.abs(one["best"][0].cpu().numpy() - outs[0]["best"]).max() <= 1e-12
    assert np.abs(one["weighted"][:n].cpu().numpy() - _flat(outs[0]["weighted"], T)).max() <= 1e-12
    many = dv.chain(ws)                                                               # W = 7 (1 for the large case), set 0 as alone
    for i, o in enumerate(outs):
        assert np.array_equal(many["chosen"][i].cpu().numpy(), o["chosen"]), i
        assert np.abs(many["best"][i].cpu().numpy() - o["best"]).max() <= 1e-12
    assert torch.equal(many["chosen"][0], one["chosen"][0]) and torch.equal(many["best"][0], one["best"][0])
    dv.prepare()                                                                      # two launches: equal bits
    again = dv.chain(ws)
    assert torch.equal(again["chosen"], many["chosen"]) and torch.equal(again["best"].view(torch.int64), many["best"].view(torch.int64))
    if name == "empty":
        assert (outs[0]["chosen"][3] == -1).all() and (outs[0]["best"][3] == 0).all()       # no proposals, nothing annotated in it
        assert outs[0]["chosen"][1].tolist() == [-1, 0] and outs[0]["best"][1].tolist() == [0.0, 1.0]      # ... but for the object annotated there
    if name == "T3late":
        assert np.isinf(frames[1]["emb"][2]).all()


@pytest.mark.parametrize("name", ("T1", "T3late", "empty", "big"))
def test_paint_against_the_restatement(name):
    import torch
    from premvos_amd import prewarp as pw
    frames, h, w, ws, outs = _case(name)
    dv = pw.upload(frames, h, w)
    dv.prepare()
    c = dv.chain(ws)
    T0 = len(frames[0]["ann"])
    gt = np.random.default_rng(1).integers(0, T0 + 2, (len(frames), h, w)).astype(np.uint8)
    gt[1][gt[1] == 1] = 0                                                             # id 1 absent from a frame
    gtb = pw.gt_bit_planes(gt, T0, dv.dev)
    idmap, _ = dv.paint(c["chosen"][:1], c["best"][:1])
    assert np.array_equal(idmap.cpu().numpy(), outs[0]["idmap"])
    _, counts = dv.paint(c["chosen"], c["best"], idmap=False, gt_bits=gtb, T0=T0)
    both_map, both = dv.paint(c["chosen"][:1], c["best"][:1], idmap=True, gt_bits=gtb, T0=T0)
    counts = counts.cpu().numpy()
    for i, o in enumerate(outs):
        assert np.array_equal(counts[i], R.region_counts(o["index"], gt, T0)), i
    assert torch.equal(both_map, idmap) and np.array_equal(both.cpu().numpy()[0], counts[0])
    scores = pw.scores_from_counts(counts)
    for i, o in enumerate(outs):
        assert np.array_equal(scores[i], R.eval_video(o["index"], gt, T0))
    if name == "T3late":
        o = outs[0]
        hidden = [(t, k) for t in range(2) for k in (2,) if ((o["index"][t] == k + 1) & (o["idmap"][t] == 0)).any()]
        assert hidden, "the not-yet-annotated template painted nothing: the case does not test that it hides lower scores"


def test_paint_rules_of_our_own():
    """crafted selections: equal scores (the higher index on top), a NaN score (on top of everything), a template not annotated yet
    that hides a lower score, a mask size whose h*w is no multiple of 8"""
    import torch
    from premvos_amd import prewarp as pw
    h, w = 33, 47
    m = np.zeros((4, h, w), np.uint8)
    m[0, 2:20, 2:30], m[1, 10:28, 10:40], m[2, 0:33, 20:25], m[3, 15:18, 0:47] = 1, 1, 1, 1
    ann = [{"id": 7, "mask": m[0], "fwd": m[0], "reid": np.zeros(R.EMB)}, {"id": 9, "mask": m[1], "fwd": m[1], "reid": np.ones(R.EMB)}]
    late = [{"id": 4, "mask": m[2], "fwd": m[2], "reid": np.full(R.EMB, 2.0)}]
    emb = np.random.default_rng(0).standard_normal((4, R.EMB))
    fr = lambda a: {"score": np.full(4, 0.5), "mask": m, "fwd": m, "emb": emb, "reid": emb, "ann": a}         # noqa: E731
    frames = [fr(ann), fr([]), fr(late)]
    dv = pw.upload(frames, h, w)
    dv.prepare()
    chosen = torch.tensor([[[4, 5, 2], [0, 1, 3], [3, 2, 4]]], dtype=torch.int32, device=dv.dev)
    best = torch.tensor([[[1.0, 1.0, 0.3], [0.4, 0.4, 0.9], [float("nan"), 0.2, 1.0]]], dtype=torch.float64, device=dv.dev)
    idmap, _ = dv.paint(chosen, best)
    got = idmap.cpu().numpy()
    want = np.zeros((3, h, w), np.uint8)
    labels = [[7, 9, 0], [7, 9, 0], [7, 9, 4]]
    sel = [[m[0], m[1], m[2]], [m[0], m[1], m[3]], [m[3], m[2], m[2]]]
    for t in range(3):
        idx = np.zeros((h, w), np.uint8)
        for k in R.paint_order(best[0, t].cpu().numpy()):
            idx[sel[t][k] != 0] = k + 1
        for k in range(3):
            want[t][idx == k + 1] = labels[t][k]
    assert np.array_equal(got, want)
    assert (got[0][(m[0] & m[1]) != 0] == 9).all()                                    # equal scores: the higher index on top
    assert (got[1][m[3] != 0] == 0).all() and (m[3] & m[0]).any()                     # label 0 hides what lies under it
    assert (got[2][m[3] != 0] == 7).all()                                             # a NaN score paints last


# ------------------------------------------------------------------------------------------------------------------- the fixture
def _fixture_frames(name, late=True):
    frames = R.fixture_video(REF, G, name, late)
    for f in frames:
        f["emb"] = f["reid"]
    return frames


@pytest.mark.parametrize("name", ("alpha", "beta"))
def test_merge_video_reproduces_the_reference(name):
    from premvos_amd import prewarp as pw
    frames = _fixture_frames(name)
    r = pw.merge_video(frames, G["h"], G["w"], record=True)
    r["ready"].synchronize()
    assert r["idmap"].is_pinned() and np.array_equal(r["idmap"].numpy(), REF[f"v_{name}_png"])
    assert np.array_equal(r["chosen"][0].cpu().numpy(), REF[f"v_{name}_chosen"])
    assert np.abs(r["best"][0].cpu().numpy() - REF[f"v_{name}_best"]).max() <= 1e-12
    T = r["video"].tab.T
    want = np.concatenate([REF[f"v_{name}_weighted_{t}"].reshape(-1) for t in range(len(frames))])
    assert np.abs(r["weighted"][:len(want)].cpu().numpy() - want).max() <= 1e-12 and len(want) == T * r["video"].tab.sumP


def _write_tree(root, names):
    from PIL import Image
    from premvos_amd import rle
    h, w = G["h"], G["w"]
    for name in names:
        frames = R.fixture_video(REF, G, name)
        for sub in ("data/DAVIS/JPEGImages/480p", "data/DAVIS/Annotations/480p", "output/intermediate/ReID_proposals", "output/intermediate/flow"):
            os.makedirs(os.path.join(root, sub, name))
        for t, f in enumerate(frames):
            Image.fromarray(np.full((h, w, 3), 90 + t, np.uint8)).save(os.path.join(root, "data/DAVIS/JPEGImages/480p", name, f"{t:05d}.jpg"))
            ann = REF[f"v_{name}_gt"][t].copy()
            for k, o in enumerate(G["videos"][name]["objects"]):                     # an object is annotated from the frame on in which it starts
                if t < o["start"]:
                    ann[ann == o["id"]] = 0
            im = Image.frombytes("P", (w, h), ann.tobytes())
            im.putpalette([0, 0, 0, 128, 0, 0] + [0] * (3 * 254))
            im.save(os.path.join(root, "data/DAVIS/Annotations/480p", name, f"{t:05d}.png"))
            props = []
            for p in range(len(f["score"])):
                d = {"score": float(f["score"][p]), "segmentation": rle.encode(f["mask"][p])}
                if np.isfinite(f["reid"][p]).all():
                    d["ReID"] = f["reid"][p].tolist()
                props.append(d)
            with open(os.path.join(root, "output/intermediate/ReID_proposals", name, f"{t:05d}.json"), "w") as fh:
                json.dump(props, fh)
            if t < len(frames) - 1:
                with open(os.path.join(root, "output/intermediate/flow", name, f"{t:05d}.flo"), "wb") as fh:
                    np.array([202021.25], np.float32).tofile(fh)
                    np.array([w, h], np.int32).tofile(fh)
                    REF[f"v_{name}_flow"][t].astype(np.float32).tofile(fh)
    os.makedirs(os.path.join(root, "code/ReID_net/configs"))
    open(os.path.join(root, "code/ReID_net/configs/live"), "w").write("{}")


def _stub_engines(monkeypatch):
    """the annotation objects' embeddings are the fixture's (the reference read them from its first-frame proposal files)"""
    from premvos_amd import track
    import premvos_amd.reid.driver as rd

    def add_reid(templates, image_fn, net):
        name = os.path.basename(os.path.dirname(image_fn))
        for t in templates:
            t["ReID"] = REF[f"v_{name}_ann_emb"][int(t["id"]) - 1].tolist()
        return templates
    monkeypatch.setattr(rd, "ReID_net_init", lambda: "stub ReID engine")
    monkeypatch.setattr(track, "_default_engine_calls", lambda a, b: (None, add_reid))


def _tree_state(root, subs):
    return {os.path.relpath(os.path.join(d, f), root): os.path.getmtime(os.path.join(d, f)) for s in subs for d, _, fs in os.walk(os.path.join(root, s)) for f in fs}


def test_track_prewarp_on_the_fixture_tree(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from premvos_amd import track
    root = str(tmp_path)
    _write_tree(root, ("alpha", "beta"))
    _stub_engines(monkeypatch)
    before = _tree_state(root, ("output/intermediate",))
    assert track.main(["--root", root, "--prewarp", "--late-annotations"]) == 0
    assert "final_prewarp" in capsys.readouterr().out
    for name in ("alpha", "beta"):
        got = np.array([np.array(Image.open(os.path.join(root, "output/final_prewarp", name, f"{t:05d}.png"))) for t in range(5)])
        assert np.array_equal(got, REF[f"v_{name}_png"]), name
    assert not os.path.exists(os.path.join(root, "output/final")) and _tree_state(root, ("output/intermediate",)) == before
    assert track.main(["--root", root, "--prewarp", "--videos", "alpha"]) == 0       # late annotations off: merge.py:78's rule
    got = np.array([np.array(Image.open(os.path.join(root, "output/final_prewarp", "alpha", f"{t:05d}.png"))) for t in range(5)])
    want = R.merge_video(R.fixture_video(REF, G, "alpha", late=False), G["h"], G["w"])["idmap"]
    assert not (got == 3).any() and (REF["v_alpha_png"] == 3).any() and np.array_equal(got, want)


def test_prewarp_search_on_the_fixture_tree(tmp_path, monkeypatch):
    from premvos_amd import track
    root = str(tmp_path)
    _write_tree(root, ("alpha", "beta"))
    _stub_engines(monkeypatch)
    before = _tree_state(root, ("output/intermediate",))
    assert track.main(["--root", root, "--prewarp-search", "7", "--seed", "3", "--late-annotations"]) == 0
    r = json.load(open(os.path.join(root, "output", "prewarp_search.json")))
    ws = R.search_weights(7, 3)
    assert np.array_equal(np.array(r["weights"]), ws) and r["seed"] == 3
    for name in ("alpha", "beta"):
        scores = np.array(r["videos"][name]["scores"])
        assert np.array_equal(scores[0], REF[f"v_{name}_eval"]), name                  # set 0 == the reference's eval_video
        frames = R.fixture_video(REF, G, name)
        T0 = R.check_first_frame_ids(frames)
        for i in range(7):
            assert np.array_equal(scores[i], R.eval_video(R.merge_video(frames, G["h"], G["w"], ws[i])["index"], REF[f"v_{name}_gt"], T0)), (name, i)
    assert np.array_equal(np.array(r["mean"]), [np.mean(np.concatenate([np.array(r["videos"][n]["scores"])[i] for n in ("alpha", "beta")])) for i in range(7)])
    assert not os.path.exists(os.path.join(root, "output/final")) and not os.path.exists(os.path.join(root, "output/final_prewarp"))
    assert _tree_state(root, ("output/intermediate",)) == before


def test_flow_path_over_more_than_eight_frames():
    """the forward masks the package makes itself: 12 frames with a flow each (premvos_mask_warp_seats_u8 takes 8 per launch) -- every
    row of the pool against ``mergetrack.warp_masks`` frame by frame, the proposals as run boundaries (``track.parse_fresh``'s route)"""
    import torch
    from premvos_amd import mergetrack, prewarp as pw, rle, track
    h, w, N, P = 33, 47, 12, 3
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    frames, masks, flows, anns = [], [], [], {}
    for t in range(N):
        m = np.zeros((P, h, w), np.uint8)
        for p in range(P):
            y, x = rng.integers(0, h - 8), rng.integers(0, w - 8)
            m[p, y:y + rng.integers(3, 9), x:x + rng.integers(3, 9)] = 1
        flow = np.stack([2.5 * np.sin(yy / 9.0 + t) + 1.25, 1.5 * np.cos(xx / 7.0 - t) - 0.5], -1).astype(np.float32)
        pool, offsets = track.boundaries_from_segmentations([rle.encode(x) for x in m])
        ann = []
        if t in (0, 9):
            a = np.zeros((h, w), np.uint8)
            a[4 + t:14 + t, 5:25] = 1
            ann, anns[t] = [{"id": 1 + t, "mask": a, "reid": rng.standard_normal(R.EMB)}], a
        fr = {"score": rng.uniform(0.2, 1, P), "emb": rng.standard_normal((P, R.EMB)), "pool": pool, "offsets": offsets, "ann": ann}
        if t < N - 1:
            fr["flow"] = flow
        frames.append(fr)
        masks.append(m)
        flows.append(flow)
    dv = pw.upload(frames, h, w)
    got = dv.pool.cpu().numpy()
    tab = dv.tab
    for t in range(N):
        want = mergetrack.warp_masks(masks[t], flows[t]).cpu().numpy() if t < N - 1 else np.zeros_like(masks[t])
        assert np.array_equal(got[tab.cur0 + t * P:tab.cur0 + (t + 1) * P], pw.pack_bits_host(masks[t])), t
        assert np.array_equal(got[tab.fwd0 + t * P:tab.fwd0 + (t + 1) * P], pw.pack_bits_host(want)), t
        assert want.any() or t == N - 1
    for k, t in enumerate((0, 9)):
        assert np.array_equal(got[tab.ann0 + k], pw.pack_bits_host(anns[t][None])[0])
        assert np.array_equal(got[tab.annfwd0 + k], pw.pack_bits_host(mergetrack.warp_masks(anns[t][None], flows[t]).cpu().numpy())[0])
    dv.prepare()                                                                      # ... and the video merges
    c = dv.chain(pw.normalised()[None])
    assert (c["chosen"][0, :, 0] >= 0).all()


def test_track_prewarp_eval_and_overlay(tmp_path, monkeypatch, capsys):
    """``--eval`` / ``--overlay`` get every id map from HBM: the counts equal premvos_amd.evaluate on the PNGs, the JPEGs are the bytes
    premvos_amd.overlay makes of frame + PNG; nothing of the live loop's outputs is touched"""
    import torch
    from PIL import Image
    from premvos_amd import evaluate as ev, jpeg, overlay, track
    root = str(tmp_path)
    _write_tree(root, ("alpha", "beta"))
    _stub_engines(monkeypatch)
    assert track.main(["--root", root, "--prewarp", "--late-annotations", "--eval", "--overlay"]) == 0
    out = capsys.readouterr().out
    assert "J&F" in out and "overlay_prewarp" in out
    for sub in ("output/final", "output/eval", "output/overlay", "output/premvos_amd_davis_eval.json"):
        assert not os.path.exists(os.path.join(root, sub)), sub
    got = ev.summarise(os.path.join(root, "output/eval_prewarp"), ["alpha", "beta"])
    want = ev.evaluate(os.path.join(root, "output/final_prewarp"), os.path.join(root, "data/DAVIS/Annotations/480p"), ["alpha", "beta"])
    assert got == want and json.load(open(os.path.join(root, "output/premvos_amd_davis_eval_prewarp.json"))) == json.loads(json.dumps(got))
    for name in ("alpha", "beta"):
        for t in range(5):
            png = np.array(Image.open(os.path.join(root, "output/final_prewarp", name, f"{t:05d}.png")))
            assert np.array_equal(png, REF[f"v_{name}_png"][t])
            jpg = os.path.join(root, "data/DAVIS/JPEGImages/480p", name, f"{t:05d}.jpg")
            ref_fn = os.path.join(root, "want.jpg")
            overlay.write_jpg(ref_fn, overlay.forward(jpeg.imread(jpg, torch.device("cuda", 0)), torch.from_numpy(png).cuda()))
            assert open(os.path.join(root, "output/overlay_prewarp", name, f"{t:05d}.jpg"), "rb").read() == open(ref_fn, "rb").read(), (name, t)
