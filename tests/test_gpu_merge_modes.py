"""The oracle merge and the probabilistic combination on the GPU (csrc/merge_modes_ops.hip, ``premvos_amd.track``) against the numpy
restatement (tests/merge_modes_restated.py, itself pinned to the reference executed: tests/test_cpu_merge_modes.py) and against the
reference's recorded outputs (tests/golden/merge_modes_ref.npz).  One process, no subprocess.

Bounds.  Counts: exact integers.  IoU planes: one correctly rounded division of the same integers, the weighted sum the same five
products and four sums in the same order: 1e-12 is the project's float64 bar (they come out bit-equal).  Probabilities: exp of the same
argument (another libm: a few ulp), the same sums in the same order; numpy's own ``sum(axis=1)`` is pairwise from 8 terms on (<= P ulp
apart): 1e-12 relative.  Labels, id maps, masks: bit for bit against the restatement FED THE DEVICE'S probabilities, on inputs of which
the test first asserts (on the CPU, zero pixels left out) that every pixel's two largest values are equal or >= 1e-9 apart."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import merge_modes_restated as MM  # noqa: E402
import track_restated as R  # noqa: E402
from premvos_amd import rle  # noqa: E402

TOL = 1e-12
SIZES = [(5, 7), (24, 40), (67, 131)]          # a tail only; less than one workgroup's span; several workgroups + a ragged tail


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _masks(rng, P, h, w, kind):
    """uint8 [P,h,w], nonzero = foreground (values 1 .. 255): ellipses or dense random; from P = 3 on, mask 0 covers the frame and mask 1
    is empty."""
    m = MM.ellipses(rng, h, w, P) if kind == "ellipse" else (rng.random((P, h, w)) < 0.4).astype(np.uint8)
    if P >= 3:
        m[0], m[1] = 1, 0
    return (m * rng.integers(1, 256, (P, 1, 1))).astype(np.uint8)


def _counts_ref(masks, labels, T):
    P = len(masks)
    inter = np.zeros((T, P), np.int64)
    for p in range(P):
        inter[:, p] = np.bincount(labels[masks[p] != 0].ravel(), minlength=257)[1:T + 1]
    return inter, (masks != 0).reshape(P, -1).sum(1).astype(np.int64), np.bincount(labels.ravel(), minlength=257)[1:T + 1].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ label overlap
@pytest.mark.parametrize("h,w", SIZES)
def test_label_overlap_equals_numpy(h, w):
    from premvos_amd import track
    dev = _dev()
    rng = np.random.default_rng(100 * h + w)
    for P in (1, 3, 300):
        masks = _masks(rng, P, h, w, "ellipse" if P == 3 else "random")
        md = torch.from_numpy(masks).to(dev)
        for T in (1, 2, 32, 255):
            maps = [rng.integers(0, min(T + 4, 256), (h, w)).astype(np.uint8),                  # holds 0 and, below 255, labels above T
                    np.zeros((h, w), np.uint8)]
            if T == 2:
                blob = np.zeros((h, w), np.uint8)                                               # object-like: long runs of one label
                blob[: h // 2] = 1
                blob[h // 2:, w // 3:] = 2
                blob[-1, -1] = 200
                maps.append(blob)
            for labels in maps:
                ld = torch.from_numpy(labels).to(dev)
                got = [t.cpu().numpy() for t in track.track_label_overlap(md, ld, T)]
                again = [t.cpu().numpy() for t in track.track_label_overlap(md, ld, T)]
                want = _counts_ref(masks, labels, T)
                for g, a, x, name in zip(got, again, want, ("inter", "area_p", "area_l")):
                    assert g.dtype == np.int64 and g.shape == x.shape and np.array_equal(g, x), (name, P, T)
                    assert g.tobytes() == a.tobytes(), name                                     # two launches: the same bytes
    labels = rng.integers(0, 5, (h, w)).astype(np.uint8)                                        # the helper above IS the restatement's count
    for g, x in zip(_counts_ref(masks[:5], labels, 3), MM.label_overlap(masks[:5], labels, 3)):
        assert np.array_equal(g, x)


def test_label_overlap_of_a_view_and_wrong_inputs():
    from premvos_amd import track
    dev = _dev()
    rng = np.random.default_rng(3)
    masks = _masks(rng, 6, 9, 13, "random")                                                      # 117 pixels: every later mask is unaligned
    labels = rng.integers(0, 4, (9, 13)).astype(np.uint8)
    md = torch.from_numpy(masks).to(dev)
    got = track.track_label_overlap(md[1:], torch.from_numpy(labels).to(dev), 3)
    for g, x in zip(got, _counts_ref(masks[1:], labels, 3)):
        assert np.array_equal(g.cpu().numpy(), x)
    with pytest.raises(AssertionError):
        track.track_label_overlap(md, torch.zeros((9, 12), dtype=torch.uint8, device=dev), 3)


# ---------------------------------------------------------------------------------------------------------------- gt scores
@pytest.mark.parametrize("T,P,seed", [(1, 1, 0), (2, 3, 1), (3, 300, 2), (32, 40, 3), (255, 7, 4)])
def test_gt_scores_equal_the_restatement(T, P, seed):
    from premvos_amd import track
    dev = _dev()
    rng = np.random.default_rng(seed)
    h, w = 24, 40
    masks = _masks(rng, P, h, w, "ellipse" if seed % 2 else "random")
    labels = rng.integers(0, min(T + 2, 256), (h, w)).astype(np.uint8)
    if T >= 2:
        labels[labels == 2] = 0                                                                 # the annotation lacks object 2
    counts = track.track_label_overlap(torch.from_numpy(masks).to(dev), torch.from_numpy(labels).to(dev), T)
    got = {k: v.cpu().numpy() for k, v in track.track_gt_scores(*counts).items()}
    again = {k: v.cpu().numpy() for k, v in track.track_gt_scores(*counts).items()}
    planes = MM.gt_planes_from_counts(*_counts_ref(masks, labels, T))
    d = float(np.abs(got["planes"] - planes).max())
    print(f"T={T} P={P}: max |d| planes {d:.3e}")
    assert got["planes"].shape == (5, T, P) and d <= TOL and np.isfinite(got["planes"]).all()
    for k in range(1, 5):
        assert np.array_equal(got["planes"][k], got["planes"][0])
    if T >= 2:
        assert not got["planes"][:, 1].any() and got["selected"][1] == P                        # a missing object: the empty proposal
    if P >= 3:
        assert not got["planes"][:, :, 1].any()                                                 # the empty candidate
    full, index, best = R.select_from_weighted(R.weighted_from_planes(got["planes"]))           # the restatement ON the device's planes
    assert np.array_equal(got["weighted"], full)
    assert got["selected"].tolist() == index.tolist() and np.array_equal(got["final_score"], best)
    assert np.array_equal(got["object_score"], (got["planes"][0] + got["planes"][1]).max(axis=1))
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    other = track.track_gt_scores(*counts, weights=[0.5, 0.1, 0.1, 0.2, 0.1], score_thresh=0.3)
    full, index, best = R.select_from_weighted(R.weighted_from_planes(got["planes"], [0.5, 0.1, 0.1, 0.2, 0.1]), 0.3)
    assert np.array_equal(other["weighted"].cpu().numpy(), full) and other["selected"].cpu().numpy().tolist() == index.tolist()


# ------------------------------------------------------------------------------------------------------------------ combine
def _run_combine(masks, ws, ids, stride_col):
    from premvos_amd import track
    dev = _dev()
    w_in = np.append(ws, np.full((len(ws), 1), 7.0), axis=1) if stride_col else ws               # [T,P+1]: the last column is not read
    out = track.track_combine(torch.from_numpy(masks).to(dev), torch.from_numpy(np.ascontiguousarray(w_in)).to(dev),
                              torch.tensor(ids, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_combine(masks, ws, ids, stride_col=False):
    T, P = ws.shape
    probs, _, best = MM.probs_from_weighted(ws)
    full = MM.combined_from_probs(masks, probs)
    assert MM.gap_violations(full) == 0, "the inputs of this case must keep the 1e-9 condition: pick another seed"
    got = _run_combine(masks, ws, ids, stride_col)
    rel = float((np.abs(got["probs"] - probs) / probs).max())
    srt = np.sort(full, axis=0)
    gaps = (srt[-1] - srt[-2])[(srt[-1] - srt[-2]) != 0]
    print(f"T={T} P={P} hw={masks.shape[1:]}: probs max rel {rel:.3e}; background {float((np.argmax(full, 0) == 0).mean()):.2f}; "
          f"smallest non-zero top-two gap {float(gaps.min()) if gaps.size else np.inf:.3e}")
    assert got["probs"].shape == (T, P) and rel <= TOL
    assert np.array_equal(got["final_score"], best)
    labels, idmap, refined, _ = MM.combine_from_probs(masks, got["probs"], ids)                 # the restatement FED the device's probabilities
    for name, x in (("labels", labels), ("idmap", idmap), ("refined", refined)):
        assert got[name].dtype == np.uint8 and got[name].shape == x.shape and got[name].tobytes() == x.tobytes(), (name, T, P)
    assert set(np.unique(got["idmap"])) <= {0} | {int(i) for i in ids}
    again = _run_combine(masks, ws, ids, stride_col)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k                                        # two launches: the same bytes
    return got


@pytest.mark.parametrize("h,w", SIZES)
def test_combine_equals_the_restatement(h, w):
    rng = np.random.default_rng(7 * h + w)
    n = 0
    for T in (1, 2, 10, 32):
        for P in (1, 2, 30, 300):
            kind = "ellipse" if n % 2 == 0 else "random"                                        # object-like masks in half the cases
            masks = _masks(rng, P, h, w, kind)
            ws = rng.uniform(0.0, 1.0, (T, P))
            ids = (np.sort(rng.permutation(255)[:T]) + 1).tolist()                              # not 1 .. T
            _check_combine(masks, ws, ids, stride_col=bool(n % 3 == 0))
            n += 1


def test_combine_special_cases():
    a = MM.load_fixture()
    # equal scores: a pixel ONE of the two covers is 0.5 against a background of 0.5 -> background; both -> the object
    got = _check_combine(a["tie_masks"], np.array([[0.5, 0.5]]), [9])
    m = a["tie_masks"] != 0
    assert not got["labels"][m[0] ^ m[1]].any() and (got["labels"][m[0] & m[1]] == 1).all() and (got["idmap"][m[0] & m[1]] == 9).all()
    assert np.array_equal(got["probs"], [[0.5, 0.5]])
    # non-contiguous ids, a full-frame and an empty mask, non-finite scores (count as 0)
    rng = np.random.default_rng(5)
    masks = _masks(rng, 6, 24, 40, "ellipse")
    ws = rng.uniform(0, 1, (3, 6))
    ws[0, 2], ws[1, 0], ws[2, 5] = np.nan, np.inf, -np.inf
    got = _check_combine(masks, ws, [3, 7, 200], stride_col=True)
    assert set(np.unique(got["idmap"])) <= {0, 3, 7, 200} and len(np.unique(got["idmap"])) > 2
    clean = np.where(np.isfinite(ws), ws, 0.0)
    assert np.array_equal(got["probs"], _run_combine(masks, clean, [3, 7, 200], False)["probs"])
    # more candidates than one staging round holds (1024), more templates than one register group (8)
    masks = _masks(rng, 1100, 24, 40, "ellipse")
    ws = rng.uniform(0, 0.3, (10, 1100))
    ws[np.arange(10), 1030 + 5 * np.arange(10)] = 0.9                                           # each object's dominant candidate: in the second round
    got = _check_combine(masks, ws, list(range(1, 11)))
    assert len(np.unique(got["labels"])) > 3
    # T = 255
    _check_combine(_masks(rng, 4, 9, 11, "random"), rng.uniform(0, 1, (255, 4)), list(range(1, 256)))


def test_offsets_past_two_to_the_31():
    """5300 candidates of 480x854: the last one's bytes lie beyond a 32-bit offset.  All candidates are empty but the first and the last
    (an empty candidate adds 0 to every sum), so the expectation needs those two only."""
    from premvos_amd import track
    dev = _dev()
    h, w, P = 480, 854, 5300
    assert P * h * w > 2 ** 31
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[:h, :w]
    first = ((((yy - 200) / 90) ** 2 + ((xx - 300) / 140) ** 2 <= 1) * 3).astype(np.uint8)
    last = ((((yy - 260) / 120) ** 2 + ((xx - 480) / 160) ** 2 <= 1) * 200).astype(np.uint8)
    masks = torch.zeros((P, h, w), dtype=torch.uint8, device=dev)
    masks[0].copy_(torch.from_numpy(first))
    masks[P - 1].copy_(torch.from_numpy(last))
    labels = rng.integers(0, 4, (h, w)).astype(np.uint8)
    inter, area_p, area_l = (t.cpu().numpy() for t in track.track_label_overlap(masks, torch.from_numpy(labels).to(dev), 3))
    wi, wp, wl = _counts_ref(np.stack([first, last]), labels, 3)
    assert np.array_equal(inter[:, [0, P - 1]], wi) and not inter[:, 1:P - 1].any()
    assert np.array_equal(area_p[[0, P - 1]], wp) and not area_p[1:P - 1].any() and np.array_equal(area_l, wl)
    ws = np.zeros((2, P))
    ws[0, P - 1], ws[1, 0] = 0.9, 1.0                                                           # object 0 leans on the last candidate
    got = {k: v.cpu().numpy() for k, v in track.track_combine(masks, torch.from_numpy(ws).to(dev),
                                                              torch.tensor([5, 9], dtype=torch.int32, device=dev)).items()}
    probs = MM.probs_from_weighted(ws)[0]
    assert float((np.abs(got["probs"] - probs) / probs).max()) <= TOL
    two = np.stack([first, last])
    for pr in (probs, got["probs"]):                                                            # the 1e-9 condition, then the device's own probabilities
        acc = np.where(two[0] != 0, pr[:, 0][:, None, None], 0.0) + np.where(two[1] != 0, pr[:, P - 1][:, None, None], 0.0)
        combined = acc / MM.denom_of(pr)[:, None, None]
        full = np.append(1.0 - combined.max(axis=0)[None], combined, axis=0)
        assert MM.gap_violations(full) == 0
    want = np.argmax(full, axis=0).astype(np.uint8)
    assert set(np.unique(want)) == {0, 1, 2} and got["labels"].tobytes() == want.tobytes()
    assert got["idmap"].tobytes() == np.where(want == 1, 5, np.where(want == 2, 9, 0)).astype(np.uint8).tobytes()
    assert got["refined"].tobytes() == np.stack([want == 1, want == 2]).astype(np.uint8).tobytes()


def test_combine_limits():
    from premvos_amd import _lib, track
    dev = _dev()
    with pytest.raises(_lib.PremvosError, match="255"):
        track.track_combine(torch.zeros((2, 4, 4), dtype=torch.uint8, device=dev), torch.zeros((256, 2), dtype=torch.float64, device=dev),
                            torch.ones((256,), dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------- the reference's recorded calls
@pytest.mark.parametrize("tag", ["t1p1", "tie", "t3p6", "edge"])
def test_the_fixtures_direct_calls(tag):
    from premvos_amd import track
    a = MM.load_fixture()
    masks, ws, labels = a[f"{tag}_masks"], a[f"{tag}_weighted"], a[f"{tag}_labels"]
    T, P = ws.shape
    templates = [{"id": t + 1} for t in range(T)]
    props = [{"segmentation": s} for s in MM.segs_of(masks)]
    gt_props = [{"id": int(i), "segmentation": rle.encode((labels == i).astype(np.uint8))} for i in np.unique(labels) if i != 0]
    planes = track.calculate_gt_scores(props, gt_props, templates)
    assert planes.shape == (5, T, P) and planes.dtype == np.float64 and np.abs(planes - a[f"{tag}_gt_planes"]).max() <= TOL
    out = track.probabilitic_combination(props, ws, templates, 1e-10)
    assert set(out[0]) == {"segmentation", "bbox", "final_score", "mask", "id"} and len(out) == T
    assert np.array_equal(np.array([p["mask"] for p in out]), a[f"{tag}_out_masks"])
    assert [p["id"] for p in out] == a[f"{tag}_out_ids"].tolist()
    assert np.array_equal(np.array([p["final_score"] for p in out]), a[f"{tag}_out_final_score"])
    assert np.array_equal(np.array([p["bbox"] for p in out], np.float64), a[f"{tag}_out_bbox"])
    for p, m in zip(out, a[f"{tag}_out_masks"]):
        assert p["segmentation"]["counts"] == rle.encode(m)["counts"] and list(p["segmentation"]["size"]) == [24, 32]
    dev = _dev()
    probs = track.track_combine(torch.from_numpy(masks).to(dev), torch.from_numpy(ws).to(dev),
                                torch.arange(1, T + 1, dtype=torch.int32, device=dev))["probs"].cpu().numpy()
    assert np.abs(probs - a[f"{tag}_probs"]).max() <= TOL


# ------------------------------------------------------------------------------------------------- the loop, the command
H, W, FRAMES = 24, 32, 4
VIDEOS = {"va": [(7.0, 8.0, 4.0, 5.0), (16.0, 20.0, 5.0, 7.0)], "vb": [(12.0, 14.0, 6.0, 8.0)]}   # per object: cy, cx, ry, rx in frame 0


def _ell(cy, cx, ry, rx):
    yy, xx = np.mgrid[:H, :W]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1).astype(np.uint8)


def _make_tree(root, seed=0):
    """2 videos x 4 frames of 24x32 in the PReMVOS layout (built by tests/track_restated.py's ``make_video_tree``, linked into the
    layout): objects drifting one pixel per frame, an annotation for EVERY frame, integer flows, fresh proposals per frame that CONTAIN the
    frame's ground-truth masks next to distractors."""
    rng = np.random.default_rng(seed)
    arrays, g = {}, {"h": H, "w": W, "videos": {}}
    anns = {}
    for name, objs in VIDEOS.items():
        props, gts = {}, []
        for t in range(FRAMES):
            gt = np.zeros((H, W), np.uint8)
            for i, (cy, cx, ry, rx) in enumerate(objs):
                gt[(_ell(cy, cx + t, ry, rx) != 0) & (gt == 0)] = i + 1
            fresh = [(gt == i + 1).astype(np.uint8) for i in range(len(objs))]
            fresh += [_ell(rng.uniform(4, 20), rng.uniform(4, 28), rng.uniform(2, 7), rng.uniform(2, 9)) for _ in range(3)]
            fresh.append(_ell(objs[0][0] + 1, objs[0][1] + t + 1, objs[0][2], objs[0][3]))      # near object 1, not it
            props[f"{t:05d}"] = [{"bbox": [float(v) for v in rle.to_bbox(rle.encode(m))], "score": round(float(rng.uniform(0.55, 0.99)), 2),
                                  "segmentation": rle.encode(m), "conf_score": "0.5", "ReID": rng.normal(0, 0.4, 128).round(3).tolist()}
                                 for m in fresh]
            gts.append(gt)
        flow = np.zeros((FRAMES - 1, H, W, 2), np.float32)
        flow[..., 0] = 1.0                                                                       # one pixel to the right per frame
        arrays[f"v_{name}_flow"], arrays[f"v_{name}_ann"] = flow, gts[0]
        g["videos"][name] = {"frames": FRAMES, "proposals": props, "with_annotation": True}
        anns[name] = gts
    tree = os.path.join(str(root), "tree")
    for name in VIDEOS:
        d = R.make_video_tree(tree, name, arrays, g)
        for t in range(1, FRAMES):
            R.write_index_png(os.path.join(d["anns"], name, f"{t:05d}.png"), anns[name][t])
    for link, k in (("data/DAVIS/JPEGImages/480p", "images"), ("data/DAVIS/Annotations/480p", "anns"),
                    ("output/intermediate/ReID_proposals", "props"), ("output/intermediate/flow", "flows")):
        os.makedirs(os.path.dirname(os.path.join(str(root), link)), exist_ok=True)
        os.symlink(d[k].rstrip("/"), os.path.join(str(root), link))
    for net in ("refinement_net", "ReID_net"):
        os.makedirs(os.path.join(str(root), "code", net, "configs"))
        open(os.path.join(str(root), "code", net, "configs", "live"), "w").write("{}")
    return anns


class _StubEngines:
    """Deterministic stand-ins for do_refinement / add_ReID (functions of the warped mask and of the box) that LOG what they return,
    so the restatement is replayed with ``track_restated.ReplayEngines``, which also checks that it is asked about the same boxes."""

    def __init__(self):
        self.masks, self.reid, self.bbox = [], [], []

    def do_refinement(self, proposals, image_fn, net):
        out = []
        for p in proposals:
            m = p["mask"]
            m = (m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)).astype(np.uint8)
            new = m.copy()
            new[1:] |= m[:-1]                                     # grows one pixel downwards ...
            new[:, ::5] &= m[:, ::5]                              # ... except in every fifth column
            p["segmentation"], p["conf_score"] = rle.encode(new), "0.25"
            out.append(new)
        self.masks.append(np.array(out, np.uint8))
        self.bbox.append(np.array([np.asarray(p["bbox"], np.float64) for p in proposals]))
        return proposals

    def add_ReID(self, proposals, image_fn, net):
        embs = []
        for p in proposals:
            x, y, w, h = (float(v) for v in p["bbox"])
            e = np.round((np.arange(128) % 7 - 3) * 0.05 + 0.01 * x * (np.arange(128) % 3) - 0.01 * y * (np.arange(128) % 2) + 0.002 * w * h / 8, 4)
            p["ReID"] = e.tolist()
            embs.append(e)
        self.reid.append(np.array(embs, np.float64))
        return proposals


def _run_command(root, monkeypatch, flags):
    """``track.main`` with the stub engines in the drivers' places -> {video: the stubs' log}."""
    from premvos_amd import track
    from premvos_amd.refinement import driver as rd
    from premvos_amd.reid import driver as qd
    logs = {}

    def pick(image_fn):
        name = os.path.basename(os.path.dirname(image_fn))
        return logs.setdefault(name, _StubEngines())

    monkeypatch.setattr(rd, "refinement_net_init", lambda: "stub refinement engine")
    monkeypatch.setattr(qd, "ReID_net_init", lambda: "stub ReID engine")
    monkeypatch.setattr(rd, "do_refinement", lambda p, fn, net: pick(fn).do_refinement(p, fn, net))
    monkeypatch.setattr(qd, "add_ReID", lambda p, fn, net: pick(fn).add_ReID(p, fn, net))
    assert track.main(["--root", str(root)] + flags) == 0
    return logs


@pytest.mark.parametrize("combine,oracle", [("probabilistic", False), ("argmax", True), ("probabilistic", True)])
def test_the_command_writes_the_restated_loops_pngs(tmp_path, monkeypatch, combine, oracle):
    from PIL import Image
    from premvos_amd import track
    _make_tree(tmp_path)
    flags = (["--combine", combine] if combine != "argmax" else []) + (["--oracle"] if oracle else [])
    logs = _run_command(tmp_path, monkeypatch, flags)
    lay = track.mode_layout(str(tmp_path), combine, oracle)
    assert lay["out"].endswith({("probabilistic", False): "final_prob/", ("argmax", True): "final_oracle/", ("probabilistic", True): "final_oracle_prob/"}[(combine, oracle)])
    assert not os.path.exists(os.path.join(str(tmp_path), "output", "final"))                   # a mode never writes the live loop's place
    assert sorted(os.listdir(os.path.join(str(tmp_path), "output"))) == sorted(["intermediate", os.path.basename(lay["out"].rstrip("/"))])
    base = track._layout(str(tmp_path))
    for name in VIDEOS:
        eng = R.ReplayEngines(logs[name].masks, logs[name].reid, logs[name].bbox)
        ref = MM.do_video(os.path.join(base["images"], name) + "/", base["images"], base["anns"], base["props"], base["flows"],
                          eng.do_refinement, eng.add_ReID, combine=combine, oracle=oracle)
        assert len(ref) == FRAMES and eng.n_refine == FRAMES - 1 and eng.n_reid == FRAMES
        painted = 0
        for t, rec in enumerate(ref):
            if combine == "probabilistic":
                assert rec["gap_violations"] == 0, (name, t)
            elif not oracle:
                srt = np.sort(rec["weighted"], axis=1)
                assert float((srt[:, -1] - srt[:, -2]).min()) >= 1e-6
            im = Image.open(os.path.join(lay["out"], name, f"{t:05d}.png"))
            assert im.mode == "P" and np.array_equal(np.array(im), rec["png"]), (name, t)
            painted += int(np.count_nonzero(rec["png"]))
        assert painted > 0


def test_the_oracle_with_eval_reports_j_of_one(tmp_path, monkeypatch):
    """The fresh proposals contain each frame's ground-truth masks: under the oracle every object selects its own, J = 1 exactly."""
    from premvos_amd import track
    anns = _make_tree(tmp_path)
    _run_command(tmp_path, monkeypatch, ["--oracle", "--eval"])
    lay = track.mode_layout(str(tmp_path), "argmax", True)
    assert not os.path.exists(os.path.join(str(tmp_path), "output", "final")) and not os.path.exists(os.path.join(str(tmp_path), "output", "eval"))
    for name, objs in VIDEOS.items():
        d = json.load(open(os.path.join(lay["eval"], name + ".json")))
        counts = np.array(d["counts"], np.int64)
        assert d["frames"] == ["00001", "00002"] and d["ids"] == list(range(1, len(objs) + 1)) and counts.shape == (2, len(objs), 6)
        assert (counts[..., 0] == counts[..., 1]).all() and (counts[..., 0] > 0).all()         # |R and G| == |R or G| per object and frame
        assert all(v == 1.0 for v in d["J"].values())
        for t in range(FRAMES):
            from PIL import Image
            assert np.array_equal(np.array(Image.open(os.path.join(lay["out"], name, f"{t:05d}.png"))), anns[name][t])
    s = json.load(open(lay["summary"]))
    assert s["mean_J"] == 1.0 and lay["summary"].endswith("premvos_amd_davis_eval_oracle.json")


def test_the_oracle_refuses_what_it_cannot_score(tmp_path):
    from premvos_amd import _lib, track
    dev = _dev()
    eng = _StubEngines()
    seg = rle.encode(_ell(10, 10, 4, 4))
    tr = track.Tracker(None, None, do_refinement=eng.do_refinement, add_ReID=eng.add_ReID, oracle=True)
    tr.add_templates([{"id": 2, "segmentation": seg, "score": 1.0, "ReID": [0.0] * 128}], None)
    with pytest.raises(_lib.PremvosError, match="annotation"):
        tr.step([])                                                                             # no gt
    with pytest.raises(_lib.PremvosError, match="1 .. 1"):
        tr.step([], gt=np.zeros((H, W), np.uint8))                                              # template ids are not 1 .. T
    ok = track.Tracker(None, None, do_refinement=eng.do_refinement, add_ReID=eng.add_ReID, oracle=True, record=True)
    ok.add_templates([{"id": 1, "segmentation": seg, "score": 1.0, "ReID": [0.0] * 128}], None)
    with pytest.raises(_lib.PremvosError, match="uint8 id map"):
        ok.step([], gt=np.zeros((H, W + 1), np.uint8))
    r = ok.step([], gt=torch.from_numpy(_ell(10, 10, 4, 4)).to(dev))                            # a CUDA tensor is taken as it is
    assert np.array_equal(r["planes"], np.ones((5, 1, 1))) and np.array_equal(r["idmap"].cpu().numpy(), _ell(10, 10, 4, 4))
    with pytest.raises(ValueError, match="combine"):
        track.Tracker(None, None, do_refinement=eng.do_refinement, add_ReID=eng.add_ReID, combine="soft")


# ------------------------------------------------------------------------------------------------------ the resident step
def test_resident_step_with_the_combination_equals_the_dict_step():
    """One last frame (flow=None) through ``step_resident`` and through ``step`` on the same arrays, combine="probabilistic"."""
    import test_gpu_track_resident as TR
    case = TR.crafted_case(3, 20)
    a = TR._tracker(case, record=True, combine="probabilistic")
    want = a.step(TR._fresh_dicts(case))
    b = TR._tracker(case, combine="probabilistic")
    fm, rows, sc = TR._fresh_arrays(case, b.device)
    got = b.step_resident(fm, rows, sc)
    for k in ("selected", "weighted", "planes", "final_score", "object_score", "labels", "probs"):
        assert got[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    idmap = got["idmap"].wait().copy()
    got["idmap"].release()
    assert idmap.tobytes() == want["idmap"].cpu().numpy().tobytes() and idmap.any()
    assert want["probs"].shape == (3, 23) and np.abs(want["probs"].sum(axis=1) - 1).max() <= 1e-12
    assert np.array_equal(want["final_score"], want["weighted"][:, :-1].max(axis=1))            # the row maximum, not the threshold's
    # and the default tracker still carries no "probs"
    c = TR._tracker(case, record=True)
    assert "probs" not in c.step(TR._fresh_dicts(case))
