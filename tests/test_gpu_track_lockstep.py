"""Several videos per launch (csrc/track_ops.hip ``*_seats_*``, premvos_mask_warp_seats_u8, ``track.TrackerGroup``, ``track --lockstep``).

Kernels: per seat against (a) the single-video entry point on that seat's slices -- the same arithmetic in the same order, so every
output bit for bit -- and (b) the numpy restatement (tests/track_restated.py) under test_gpu_track.py's bounds (planes 0 / 3 / 4, labels,
id maps, masks equal; planes 1 / 2 and the weighted scores <= 1e-12; selections equal on inputs with a margin >= 1e-6, which is asserted
for every seat but the one that holds a template without ReID, whose row is all NaN -> 0).  A NaN INPUT score is compared with (a)
only: the kernels' fmax drops it where numpy's maximum keeps it, in the single-video entry as here.

The group: one seat against the ``Tracker`` loop bit for bit (the same plans and launches); several seats against the restatement fed
with what the engines returned (another batch size may pick another k-split inside the nets, so the sequential run's bytes are not
promised -- DESIGN.md 8.4)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import track_restated as R  # noqa: E402
from premvos_amd import rle  # noqa: E402
from test_gpu_track import TOL, _blobs, _check_scores, _score_inputs  # noqa: E402

TABLES = {"V1": [(1, 0)],
          "V3": [(1, 1), (0, 0), (5, 12)],
          "V8": list(zip((1, 2, 3, 7, 10, 32, 1, 4), (0, 40, 17, 300, 110, 480, 1, 0)))}
NAN_SEAT = {"V1": None, "V3": 2, "V8": 3}            # the seat whose template 1 has no ReID (its ReID row is NaN)
CASES = [("V1", 9, 7), ("V3", 9, 7), ("V1", 31, 45), ("V3", 31, 45), ("V8", 31, 45), ("V3", 40, 56), ("V8", 40, 56), ("V3", 480, 854)]


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _pool(name, h, w, seed):
    """One pool in which candidate and fresh blocks of different seats alternate, with a foreign mask between any two blocks: a wrong
    offset reads a neighbour's mask.  -> (pool uint8 [S,h,w] numpy, SeatTable)"""
    from premvos_amd import track
    rng = np.random.default_rng(seed)
    blocks, rows, at = [], [], 0
    for v, (T, F) in enumerate(TABLES[name]):
        order = (("f", F), ("c", T)) if v % 2 == 0 else (("c", T), ("f", F))
        slot = {"c": 0, "f": 0}
        for kind, n in order:
            blocks.append(np.stack([_blobs(rng, h, w, 2)]))                                     # the foreign mask
            at += 1
            slot[kind] = at
            if n:
                blocks.append(np.stack([_blobs(rng, h, w, 2) * rng.integers(1, 256) for _ in range(n)]))   # nonzero = foreground
            at += n
        rows.append((T, F, slot["c"], slot["f"]))
    return np.concatenate(blocks).astype(np.uint8), track.SeatTable(rows)


def _seat_masks(pool, st, v):
    T, F, c, f = (int(x) for x in st.rows[v])
    return torch.cat([pool[c:c + T], pool[f:f + F]]) if T else pool[:0]


# ----------------------------------------------------------------------------------------------------------------- overlap
@pytest.mark.parametrize("name,h,w", CASES)
def test_overlap_seats_equal_the_single_video_entry_per_seat(name, h, w):
    from premvos_amd import mergetrack, track
    pool_np, st = _pool(name, h, w, seed=h + len(name))
    pool = torch.from_numpy(pool_np).to(_dev())
    got = track.mask_overlap_seats(pool, st)
    again = track.mask_overlap_seats(pool, st)
    for k in got:
        assert torch.equal(got[k], again[k]), k                                                # two launches: the same bits
    for v in range(st.V):
        if not st.T[v]:
            continue
        m = _seat_masks(pool, st, v)
        T = int(st.T[v])
        inter, area_p, area_t = mergetrack.mask_overlap(m, m[:T])
        mine = st.views(got, v)
        assert torch.equal(mine["inter"], inter) and torch.equal(mine["area_p"], area_p) and torch.equal(mine["area_t"], area_t), v
        b = m.cpu().numpy() != 0                                                                # (b) the counts themselves
        assert np.array_equal(mine["area_p"].cpu().numpy(), b.reshape(len(b), -1).sum(1))
        if h * w <= 4096:
            assert np.array_equal(mine["inter"].cpu().numpy(), (b[:T, None] & b[None]).reshape(T, len(b), -1).sum(2))


# ------------------------------------------------------------------------------------------------------------------ scores
def _seat_score_inputs(name, seed):
    """Per seat ``_score_inputs``: NAN_SEAT gets a template without ReID, every seat with enough fresh rows proposals without ReID (+inf rows)."""
    per = []
    for v, (T, F) in enumerate(TABLES[name]):
        if not T:
            per.append(None)
            continue
        P = T + F
        a = list(_score_inputs(seed + 17 * v, T, P, no_reid=[j for j in (1, P - 2) if 0 <= j < P and P > 4 and j >= T]))
        a[4][:T] = a[3]                                      # the template score IS the candidate score of the same slot
        if v == NAN_SEAT[name]:
            a[6][1] = np.inf
        per.append(a)
    return per


def _pooled(per, dev):
    live = [a for a in per if a is not None]
    cat = lambda parts, shape, dt: torch.from_numpy(np.concatenate([np.asarray(p, dt).reshape(shape) for p in parts])).to(dev)  # noqa: E731
    T_of = [len(a[3]) for a in live]
    overlap = {"inter": cat([a[0] for a in live], (-1,), np.int64), "area_p": cat([a[1] for a in live], (-1,), np.int64),
               "area_t": cat([a[2] for a in live], (-1,), np.int64)}
    cand_score = cat([a[4][:T] for a, T in zip(live, T_of)], (-1,), np.float64)
    cand_emb = cat([a[5][:T] for a, T in zip(live, T_of)], (-1, 128), np.float64)
    templ_emb = cat([a[6] for a in live], (-1, 128), np.float64)
    fresh_score = cat([a[4][T:] for a, T in zip(live, T_of)], (-1,), np.float64)
    fresh_emb = cat([a[5][T:] for a, T in zip(live, T_of)], (-1, 128), np.float64)
    return overlap, cand_score, cand_emb, templ_emb, fresh_score, fresh_emb


@pytest.mark.parametrize("name,seed", [("V1", 3), ("V3", 5), ("V8", 6)])
def test_scores_seats_equal_the_single_video_entry_and_the_restatement(name, seed):
    from premvos_amd import track
    dev = _dev()
    per = _seat_score_inputs(name, seed)
    st = track.SeatTable([(T, F, 0, 0) for T, F in TABLES[name]])
    overlap, cs, ce, te, fs, fe = _pooled(per, dev)
    got = track.track_scores_seats(overlap, cs, ce, te, fs if len(fs) else None, fe if len(fe) else None, st)
    again = track.track_scores_seats(overlap, cs, ce, te, fs if len(fs) else None, fe if len(fe) else None, st)
    torch.cuda.synchronize()
    for k in got:
        assert got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    for v, a in enumerate(per):
        if a is None:
            continue
        mine = {k: x.cpu().numpy() for k, x in st.views(got, v).items()}
        inter, area_p, area_t, ts, ps, ep, et = a
        one = track.track_scores(torch.from_numpy(inter).to(dev), torch.from_numpy(area_p).to(dev), torch.from_numpy(area_t).to(dev), ts, ps, ep, et)
        for k, x in one.items():
            assert mine[k].shape == x.shape and mine[k].tobytes() == x.cpu().numpy().tobytes(), (v, k)   # (a) bit for bit
        _check_scores(mine, a, need_margin=v != NAN_SEAT[name])                                 # (b)
        if v == NAN_SEAT[name]:
            assert np.isnan(mine["planes"][1][1]).any() and np.isnan(mine["object_score"][1])


def test_scores_seats_twins_tie_and_a_nan_input_score():
    """Twin templates (equal masks, embeddings, scores) have equal rows: equal final scores, the tie the paint rule orders.  And NaN
    input scores, against the single-video entry only (see the module docstring)."""
    from premvos_amd import track
    dev = _dev()
    per = []
    for v, (T, P) in enumerate(((3, 9), (2, 2), (4, 30))):
        a = list(_score_inputs(40 + v, T, P))
        a[4][:T] = a[3]
        per.append(a)
    a = per[2]
    a[0][1], a[2][1], a[3][1], a[6][1], a[4][1] = a[0][0], a[2][0], a[3][0], a[6][0], a[4][0]    # template 1 := template 0
    per[0][4][[1, 5]] = np.nan                                                                  # a candidate's and a fresh row's score
    st = track.SeatTable([(len(x[3]), len(x[4]) - len(x[3]), 0, 0) for x in per])
    overlap, cs, ce, te, fs, fe = _pooled(per, dev)
    got = track.track_scores_seats(overlap, cs, ce, te, fs, fe, st)
    for v, a in enumerate(per):
        mine = {k: x.cpu().numpy() for k, x in st.views(got, v).items()}
        inter, area_p, area_t, ts, ps, ep, et = a
        one = track.track_scores(torch.from_numpy(inter).to(dev), torch.from_numpy(area_p).to(dev), torch.from_numpy(area_t).to(dev),
                                 ps[:len(ts)], ps, ep, et)
        for k, x in one.items():
            assert mine[k].tobytes() == x.cpu().numpy().tobytes(), (v, k)
        if v:
            _check_scores(mine, a)
    tw = {k: x.cpu().numpy() for k, x in st.views(got, 2).items()}
    assert tw["final_score"][0] == tw["final_score"][1] and tw["selected"][0] == tw["selected"][1]
    assert np.array_equal(tw["weighted"][0], tw["weighted"][1])


# ------------------------------------------------------------------------------------------------------------------- paint
@pytest.mark.parametrize("name,h,w", CASES)
def test_paint_seats_equal_the_single_video_entry_and_the_restatement(name, h, w):
    from premvos_amd import track
    dev = _dev()
    pool_np, st = _pool(name, h, w, seed=3 * h + len(name))
    pool = torch.from_numpy(pool_np).to(dev)
    rng = np.random.default_rng(w)
    sel, fsc, ids = [], [], []
    for v in range(st.V):
        T, P = int(st.T[v]), int(st.P[v])
        s = rng.integers(0, P + 1, T)                                                           # P = the empty proposal
        f = rng.permutation(T).astype(np.float64) / max(T, 1) + 1e-3
        if T > 1:
            s[1] = P
        if T > 2:
            f[2], s[2] = f[0], s[0]                                                             # a tie on one mask: the higher index wins
        sel.append(s), fsc.append(f), ids.append(rng.permutation(255)[:T] + 1)
    nT = int(st.oT[-1])
    slots = (nT + 3 - st.oT[1:]).astype(np.int32)                                               # reverse seat order, 3 planes in front
    args = (pool, st, torch.from_numpy(np.concatenate(sel).astype(np.int32)).to(dev), torch.from_numpy(np.concatenate(fsc)).to(dev),
            torch.from_numpy(np.concatenate(ids).astype(np.int32)).to(dev), slots)
    outs = []
    for _ in range(2):
        keep = [torch.full((st.V, h, w), 7, dtype=torch.uint8, device=dev), torch.full((st.V, h, w), 7, dtype=torch.uint8, device=dev),
                torch.full((nT + 5, h, w), 7, dtype=torch.uint8, device=dev)]
        outs.append(track.track_paint_seats(*args, labels=keep[0], idmap=keep[1], refined=keep[2]))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    labels, idmap, refined = outs[0]
    written = np.zeros(nT + 5, bool)
    for v in range(st.V):
        T = int(st.T[v])
        if not T:
            assert bool((labels[v] == 7).all()) and bool((idmap[v] == 7).all())               # nothing is written for an empty seat
            continue
        m = _seat_masks(pool, st, v)
        mine = (labels[v], idmap[v], refined[slots[v]:slots[v] + T])
        written[slots[v]:slots[v] + T] = True
        one = track.track_paint(m, torch.from_numpy(sel[v].astype(np.int32)).to(dev), torch.from_numpy(fsc[v]).to(dev),
                                torch.from_numpy(ids[v].astype(np.int32)).to(dev))
        ref = R.paint_from_arrays(m.cpu().numpy(), sel[v], fsc[v], ids[v])
        for a, b, c, what in zip(mine, one, ref, ("labels", "idmap", "refined")):
            assert torch.equal(a, b), (v, what)                                                 # (a)
            assert np.array_equal(a.cpu().numpy(), c), (v, what)                                # (b)
        if T > 2 and sel[v][0] < st.P[v]:
            assert not bool(refined[slots[v]].any()) and not bool((labels[v] == 1).any())                                             # object 2 took every pixel of object 0
    assert bool((refined[torch.from_numpy(~written).to(dev)] == 7).all())


# -------------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("h,w", [(9, 7), (31, 45), (40, 56), (480, 854)])
def test_warp_seats_equal_one_warp_call_per_flow(h, w):
    from premvos_amd import mergetrack
    dev = _dev()
    rng = np.random.default_rng(h)
    masks = torch.from_numpy(np.stack([_blobs(rng, h, w, 2) for _ in range(6)])).to(dev)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    flows = np.stack([np.stack([1.75 * np.sin(yy / 7.0) + 0.3125, 1.25 * np.cos(xx / 5.0) - 0.40625], -1),      # sub-pixel parts
                      np.stack([np.full((h, w), w + 2.5), np.full((h, w), -0.5)], -1),                           # out of the frame
                      np.stack([xx / 3 - 2.28125, -(yy / 2) + 1.53125], -1)]).astype(np.float32)                  # partly out
    flows_d = torch.from_numpy(flows).to(dev)
    which = [2, 0, 1, 1, 0, 2]
    fom = torch.tensor(which, dtype=torch.int32, device=dev)
    got = mergetrack.warp_masks_seats(masks, fom, flows_d)
    assert torch.equal(got, mergetrack.warp_masks_seats(masks, fom, flows_d))
    for f in range(3):
        idx = [i for i, x in enumerate(which) if x == f]
        one = mergetrack.warp_masks(masks[idx].contiguous(), flows_d[f])
        assert torch.equal(got[idx], one), f
    assert bool(got[[1, 4]].any()) and not bool(got[[2, 3]].any())
    # (b) the restated remap of the oracle, on the first flow
    from oracle import merge_oracle as MO
    if h * w <= 4096:
        for i in (1, 4):
            assert np.array_equal(got[i].cpu().numpy(), MO.warp_flow(masks[i].cpu().numpy(), flows[0]))
    # a mask of no seat is not written
    out = torch.full_like(masks, 7)
    mergetrack.warp_masks_seats(masks, torch.tensor([2, 0, -1, 1, 3, 2], dtype=torch.int32, device=dev), flows_d, out=out)
    assert bool((out[[2, 4]] == 7).all()) and torch.equal(out[[0, 1, 3, 5]], got[[0, 1, 3, 5]])


# ------------------------------------------------------------------------------------------------------ the group, real engines
LOCKSTEP_SEED = 5
_ENGINES = []


def _engines():
    """The reduced-depth engines of test_gpu_track.py (synthetic weights), built once for this file."""
    if not _ENGINES:
        from oracle import refinement_oracle as RO
        from oracle import reid_oracle as QO
        from test_gpu_plumbing import MIDDLE, REID_UNITS
        from premvos_amd.refinement import RefinementNet
        from premvos_amd.refinement.driver import RefinementEngine
        from premvos_amd.reid import ReIDEngine, ReIDNet
        _ENGINES.append((RefinementEngine(RefinementNet(RO.synth_weights(0, MIDDLE), MIDDLE)),
                         ReIDEngine(ReIDNet(QO.synth_weights(0, REID_UNITS), units=[(n_, f, k, s) for n_, _, f, k, s in REID_UNITS]))))
    return _ENGINES[0]


def _video(lay, name, n_frames, n_obj, seed, no_props=()):
    """``n_frames`` of 120x200 under the five roots ``lay``: ``n_obj`` objects drifting by sub-pixel steps, an annotation for EVERY frame
    (the loop reads the first; --eval the others), fresh proposals per frame except ``no_props`` (near the objects and elsewhere, one
    without ReID), flows with sub-pixel parts."""
    from PIL import Image
    from premvos_amd import synth
    H, W = 120, 200
    rng = np.random.default_rng(seed)
    for k in ("images", "anns", "props", "flows"):
        os.makedirs(os.path.join(lay[k], name))
    frames = synth.clip_frames(0, n_frames, H, W, seed=70 + seed).numpy()
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    centres, radii = [(35, 50), (75, 100), (50, 155)][:n_obj], [(14, 18), (16, 22), (12, 15)][:n_obj]
    vel = [(0.75, 1.5), (-0.5, 1.25), (1.0, -1.25)][:n_obj]
    for t in range(n_frames):
        ann = np.zeros((H, W), np.uint8)
        for i, ((cy, cx), (ry, rx), (vy, vx)) in enumerate(zip(centres, radii, vel)):
            ann[((yy - cy - vy * t) / ry) ** 2 + ((xx - cx - vx * t) / rx) ** 2 <= 1] = (1, 2, 3)[i]
        R.write_index_png(os.path.join(lay["anns"], name, f"{t:05d}.png"), ann)
        Image.fromarray(frames[t]).save(os.path.join(lay["images"], name, f"{t:05d}.jpg"), quality=95)
        if t < n_frames - 1:
            flow = np.stack([1.5 * np.sin(yy / 23.0 + 0.1 * t) + 0.75, 1.0 * np.cos(xx / 31.0 - 0.07 * t) - 0.5], -1).astype(np.float32)
            R.write_flo(os.path.join(lay["flows"], name, f"{t:05d}.flo"), flow)
        if t in no_props:
            continue
        fresh = []
        for i, ((cy, cx), (ry, rx), (vy, vx)) in enumerate(zip(centres, radii, vel)):
            m = (((yy - cy - vy * t) / (ry + i)) ** 2 + ((xx - cx - vx * t) / (rx - i)) ** 2 <= 1).astype(np.uint8)
            seg = rle.encode(m)
            fresh.append({"bbox": rle.to_bbox(seg), "score": round(float(rng.uniform(0.6, 0.99)), 2), "segmentation": seg,
                          "conf_score": "0.5", "ReID": rng.normal(0, 0.05, 128).round(4).tolist()})
        for _ in range(3):
            cy, cx = rng.uniform(15, 105), rng.uniform(20, 180)
            m = (((yy - cy) / rng.uniform(6, 16)) ** 2 + ((xx - cx) / rng.uniform(6, 20)) ** 2 <= 1).astype(np.uint8)
            seg = rle.encode(m)
            fresh.append({"bbox": rle.to_bbox(seg), "score": round(float(rng.uniform(0.5, 0.95)), 2), "segmentation": seg,
                          "conf_score": "0.5", "ReID": rng.normal(0, 0.3, 128).round(4).tolist()})
        del fresh[-1]["ReID"]
        with open(os.path.join(lay["props"], name, f"{t:05d}.json"), "w") as f:
            json.dump(fresh, f)


def _lay(root):
    return {k: os.path.join(str(root), k) + "/" for k in ("images", "anns", "props", "flows", "out", "overlay")}


def test_group_of_one_seat_equals_the_tracker_loop_bit_for_bit(tmp_path):
    """120x200, 5 frames, 3 objects: ``do_video`` with its ``Tracker`` against a ``TrackerGroup`` of one seat -- the same plans and
    launches: selections, weighted scores, planes and the PNG files are equal byte for byte."""
    from premvos_amd import io_pipeline as iop
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(tmp_path)
    _video(lay, "clip", 5, 3, seed=LOCKSTEP_SEED)
    a = track.do_video(os.path.join(lay["images"], "clip") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"], ref_eng, reid_eng,
                       record=True, tracker=track.Tracker(ref_eng, reid_eng, record=True))
    lay_b = dict(lay, out=os.path.join(str(tmp_path), "out_b") + "/")
    with iop.Writer() as writer:
        b = track.do_videos_lockstep(["clip"], lay_b, 1, ref_eng, reid_eng, writer, record=True)["clip"]
    assert len(a) == len(b) == 5
    for t, (x, y) in enumerate(zip(a, b)):
        for k in ("selected", "weighted", "planes", "final_score", "object_score", "labels", "png"):
            assert x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), (t, k)
        assert os.path.basename(x["png_fn"]) == os.path.basename(y["png_fn"]) == f"{t:05d}.png"
        assert open(x["png_fn"], "rb").read() == open(y["png_fn"], "rb").read(), t
    assert np.unique(a[0]["png"]).tolist() == [0, 1, 2, 3] and a[-1]["png"].any()               # non-vacuous: objects are painted to the end


LENGTHS, OBJECTS = {"a": 3, "b": 5, "c": 4}, {"a": 1, "b": 3, "c": 2}


def _three_in_two(root, seed, eval_dir=None):
    from premvos_amd import io_pipeline as iop
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(root)
    for i, name in enumerate("abc"):
        _video(lay, name, LENGTHS[name], OBJECTS[name], seed=seed + i, no_props=(2,) if name == "b" else ())
    calls = {}
    with iop.Writer() as writer:
        logs = track.do_videos_lockstep(["c", "a", "b"], lay, 2, ref_eng, reid_eng, writer, eval_dir=eval_dir, record=True, engine_logs=calls)
    refs, engines = {}, {}
    for name in "abc":
        c = calls[name]
        eng = R.ReplayEngines([x["mask"] for x in c if x["call"] == "refine"], [x["ReID"] for x in c if x["call"] == "reid"],
                              [x["bbox"] for x in c if x["call"] == "refine"])
        refs[name] = R.do_video(os.path.join(lay["images"], name) + "/", lay["images"], lay["anns"], lay["props"], lay["flows"],
                                eng.do_refinement, eng.add_ReID)
        engines[name] = (eng, c)
    return lay, logs, refs, engines


def test_three_videos_in_two_seats_against_the_replayed_restatement(tmp_path):
    """Videos of 3, 5 and 4 frames with 1, 3 and 2 objects in two seats: 'a' and 'b' start, 'c' takes a's seat after three steps, b's
    seat is empty for the last two; 'b' has a frame without a proposal file.  What the engines returned per video is replayed into the
    restatement of merge.py:69-115: selections and PNG index arrays equal, scores within 1e-12, as many refinement and ReID calls per
    video as the sequential loop makes, both margins >= 1e-6 per video (LOCKSTEP_SEED was chosen on the GPU so that they hold: weighted /
    paint margins a 2.5e-1 / none (one object), b 1.1e-2 / 3.1e-4, c 2.8e-3 / 2.6e-3; seed 7 has a paint margin of 0); and with eval_dir,
    counts equal to evaluate() on the PNGs that were written."""
    from PIL import Image
    from premvos_amd import evaluate as ev
    eval_dir = str(tmp_path / "eval")
    lay, logs, refs, engines = _three_in_two(tmp_path, LOCKSTEP_SEED, eval_dir)
    for name in "abc":
        n = LENGTHS[name]
        log, ref, (eng, calls) = logs[name], refs[name], engines[name]
        assert len(log) == len(ref) == n and eng.n_refine == n - 1 and eng.n_reid == n
        assert sum(c["call"] == "refine" for c in calls) == n - 1 and sum(c["call"] == "reid" for c in calls) == n
        mw, mp = R.margins(ref)
        print(f"{name}: weighted margin {mw:.3e}, paint margin {mp:.3e}, selections {[r['selected'].tolist() for r in ref]}")
        assert mw >= 1e-6 and mp >= 1e-6, name
        for t, (x, y) in enumerate(zip(log, ref)):
            assert x["selected"].tolist() == y["selected"].tolist(), (name, t)
            assert np.abs(x["weighted"] - y["weighted"]).max() <= TOL and np.abs(x["planes"] - y["planes"]).max() <= TOL
            assert np.array_equal(x["png"], y["png"]), (name, t)
            assert np.array_equal(np.array(Image.open(x["png_fn"])), y["png"]), (name, t)      # the file the writer wrote from the ring
            assert set(np.unique(x["png"])) <= set(range(OBJECTS[name] + 1))
        assert any(x["png"].any() for x in log)
    want = ev.evaluate(lay["out"], lay["anns"], ["a", "b", "c"])
    assert ev.summarise(eval_dir, ["a", "b", "c"]) == want and want["objects"] == 6


def test_two_seats_with_more_boxes_than_the_reid_engine_embeds_at_once(tmp_path):
    """Two 4-frame videos of 3 objects each in two seats with a ReID engine of ``max_boxes`` 4: the step's nA = 6 masks go through
    ``ReIDEngine.embed_masks`` in chunks of 4 (4 + 2, both padded to 4 slots) instead of the net's single launch, and ``bbox`` is made
    contiguous.  Checked like the three videos above, against the restatement replayed from the seats' engine logs; both margins
    >= 1e-6 per video with LOCKSTEP_SEED (weighted / paint on the GPU: a 8.9e-3 / 5.9e-4, b 9.1e-4 / 2.8e-4; they are printed)."""
    from premvos_amd import io_pipeline as iop
    from premvos_amd import track
    from premvos_amd.reid import ReIDEngine
    ref_eng, reid_eng = _engines()
    small = ReIDEngine(reid_eng.net, max_boxes=4)
    lay = _lay(tmp_path)
    n = 4
    for i, name in enumerate("ab"):
        _video(lay, name, n, 3, seed=LOCKSTEP_SEED + i)
    calls = {}
    with iop.Writer() as writer:
        logs = track.do_videos_lockstep(["a", "b"], lay, 2, ref_eng, small, writer, record=True, engine_logs=calls)
    for name in "ab":
        c = calls[name]
        assert sum(x["call"] == "refine" for x in c) == n - 1 and sum(x["call"] == "reid" for x in c) == n
        eng = R.ReplayEngines([x["mask"] for x in c if x["call"] == "refine"], [x["ReID"] for x in c if x["call"] == "reid"],
                              [x["bbox"] for x in c if x["call"] == "refine"])
        ref = R.do_video(os.path.join(lay["images"], name) + "/", lay["images"], lay["anns"], lay["props"], lay["flows"],
                         eng.do_refinement, eng.add_ReID)
        log = logs[name]
        assert len(log) == len(ref) == n and eng.n_refine == n - 1 and eng.n_reid == n
        mw, mp = R.margins(ref)
        print(f"{name}: weighted margin {mw:.3e}, paint margin {mp:.3e}, selections {[r['selected'].tolist() for r in ref]}")
        assert mw >= 1e-6 and mp >= 1e-6, name
        for t, (x, y) in enumerate(zip(log, ref)):
            assert x["selected"].tolist() == y["selected"].tolist(), (name, t)
            assert np.abs(x["weighted"] - y["weighted"]).max() <= TOL and np.abs(x["planes"] - y["planes"]).max() <= TOL
            assert np.array_equal(x["png"], y["png"]), (name, t)
            assert set(np.unique(x["png"])) <= {0, 1, 2, 3}
        assert any(x["png"].any() for x in log)


# ------------------------------------------------------------------------------------------------------------ the command
def test_the_command_with_two_seats(tmp_path):
    """``track --lockstep 2`` on the ``_make_tree`` tree of test_gpu_plumbing (one annotated video, one without annotation): one mode-P PNG per frame with
    the VOC palette, pixel values within {0} + the annotation's ids, all zeros for the video without annotation."""
    from PIL import Image
    from test_gpu_plumbing import REID_NETWORK, _make_tree
    from premvos_amd import stream, track
    from premvos_amd.reid import driver as qd
    root = tmp_path / "premvos"
    root.mkdir()
    videos = {"bear": 4, "camel": 3}
    _make_tree(root, videos=videos)
    (root / "code" / "refinement_net" / "configs").mkdir(parents=True)
    (root / "code" / "refinement_net" / "configs" / "live").write_text(json.dumps({"model": "live", "load": "../weights/refinement_specific_weights"}))
    reid_cfg = {"model": "Re-ID", "load": "../weights/ReID_general_weights", "input_size": [128, 128], "network": REID_NETWORK}
    (root / "code" / "ReID_net" / "configs" / "live").write_text(json.dumps(reid_cfg))
    (root / "code" / "ReID_net" / "configs" / "run").write_text(json.dumps(dict(
        reid_cfg, image_input_dir="../data/DAVIS/JPEGImages/480p/", bb_input_dir="../output/intermediate/refined_proposals/",
        output_dir="../output/intermediate/ReID_proposals/")))
    ann_dir = root / "data" / "DAVIS" / "Annotations" / "480p" / "bear"
    ann_dir.mkdir(parents=True)
    ann = np.zeros((120, 200), np.uint8)
    ann[20:70, 30:90] = 1
    ann[60:110, 120:180] = 3
    R.write_index_png(str(ann_dir / "00000.png"), ann)
    cwd = os.getcwd()
    try:
        assert stream.main(["--root", str(root), "--batch", "2", "--flow_weights", "weights/pwc.pth.tar", "--general_weights",
                            "weights/proposal_general_weights", "--specific_weights", "weights/specific.pt", "--refinement_weights",
                            "weights/refinement_specific_weights"]) == 0
        os.chdir(root / "code")
        assert qd.main(["ReID_net/configs/run"]) == 0
        os.chdir(cwd)
        assert track.main(["--root", str(root), "--lockstep", "2"]) == 0
    finally:
        os.chdir(cwd)
    pal = track.voc_palette().reshape(-1)
    for name, n in videos.items():
        files = sorted(os.listdir(root / "output" / "final" / name))
        assert files == [f"{t:05d}.png" for t in range(n)]
        for t, fn in enumerate(files):
            im = Image.open(root / "output" / "final" / name / fn)
            px = np.array(im)
            assert im.mode == "P" and px.shape == (120, 200) and np.array_equal(np.array(im.getpalette(), np.uint8), pal)
            if name == "bear":
                assert set(np.unique(px)) <= {0, 1, 3}
                if t == 0:
                    assert np.array_equal(px, ann)
            else:
                assert not px.any()
