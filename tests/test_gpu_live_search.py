"""The live loop's weight search on the GPU (csrc/track_ops.hip premvos_track_scores_sets_f64 / premvos_track_eval_seats_i64,
``track.SearchGroup``, ``track --search W``, ``track --live-weights``).

Kernels.  The scores entry per seat against (a) premvos_track_scores_seats_f64 called with that seat's weights on arrays in which the
fresh rows are replicated per seat -- the same device function in the same order, so bit for bit -- and (b) the numpy restatement under
test_gpu_track.py's bounds (planes 0 / 3 / 4 equal, planes 1 / 2 and the weighted scores <= 1e-12, selections equal).  Selections need a
margin >= 1e-6 between the best and the second-best weighted score where the weighted score carries the 1e-12: asserted for every seat
whose weights are not one-hot.  Under (1,0,0,0,0) and (0,0,0,1,0) the weighted score IS plane 0 / plane 3 (every other product is an
exact zero of a finite number), which the kernel reproduces bit for bit; there ties are exact in both and both take the first maximum,
so the selections are compared without a margin and the weighted scores are required to be EQUAL.  The eval entry: integer counts
against numpy's, exactly.

The group: one seat against the ``Tracker`` loop byte for byte; three sets in three seats against the restatement
(tests/live_search_restated.py) fed with what the engines returned to each seat."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import live_search_restated as L  # noqa: E402
import prewarp_restated as PR  # noqa: E402
import track_restated as R  # noqa: E402
from test_gpu_track import TOL, _blobs, _score_inputs  # noqa: E402
from test_gpu_track_lockstep import _dev, _engines, _lay, _pooled, _video  # noqa: E402


def _one_hot(w):
    return int(np.count_nonzero(w)) == 1


def _check_against_the_restatement(mine, a, w, v):
    planes = R.scores_from_arrays(*a)
    full, index, best = R.select_from_weighted(R.weighted_from_planes(planes, w))
    for k in (0, 3, 4):
        assert np.array_equal(mine["planes"][k], planes[k], equal_nan=True), (v, k)
    assert np.array_equal(np.isnan(mine["planes"]), np.isnan(planes))
    d12 = max(float(np.nanmax(np.abs(mine["planes"][k] - planes[k]))) for k in (1, 2))
    dw = float(np.abs(mine["weighted"] - full).max())
    srt = np.sort(full, axis=1)
    margin = float((srt[:, -1] - srt[:, -2]).min())
    print(f"seat {v} T={planes.shape[1]} P={planes.shape[2]} w={np.round(w, 3).tolist()}: max |d| planes 1,2 {d12:.3e}  weighted {dw:.3e}  margin {margin:.3e}")
    assert d12 <= TOL and dw <= TOL and np.abs(mine["final_score"] - best).max() <= TOL
    if _one_hot(w):
        assert np.array_equal(mine["weighted"], full), v                                        # the one plane, bit for bit: ties are exact ties
    else:
        assert margin >= 1e-6, "the inputs of this seat must have a margin: pick another seed"
    assert mine["selected"].tolist() == index.tolist(), v
    assert np.array_equal(mine["final_score"], mine["weighted"][np.arange(len(index)), mine["selected"]])


# ------------------------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("name,seed", [("V1", 3), ("V3", 5), ("V3F0", 4), ("V2F300", 7), ("V8", 6)])
def test_scores_sets_equal_the_seats_entry_per_weight_set_and_the_restatement(name, seed):
    from premvos_amd import track
    dev = _dev()
    V, tf = L.SETS_CASES[name]
    F = tf[0][1]
    per, fs, fe = L.sets_inputs(name, seed)
    ws = L.weight_sets(V, seed)
    st = track.SeatTable([(T, F, 0, 0) for T, _ in tf])
    overlap, cs, ce, te, fs_rep, fe_rep = _pooled(per, dev)                                     # the fresh rows replicated per seat
    shared = (torch.from_numpy(fs).to(dev), torch.from_numpy(fe.reshape(F, 128)).to(dev)) if F else (None, None)
    got = track.track_scores_sets(overlap, cs, ce, te, shared[0], shared[1], st, ws)
    again = track.track_scores_sets(overlap, cs, ce, te, shared[0], shared[1], st, ws)
    torch.cuda.synchronize()
    for k in got:
        assert got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k            # two launches: the same bits
    sels = {}
    for v, a in enumerate(per):
        if a is None:
            continue
        mine = {k: x.cpu().numpy() for k, x in st.views(got, v).items()}
        one = track.track_scores_seats(overlap, cs, ce, te, fs_rep if F else None, fe_rep if F else None, st, weights=ws[v])
        for k, x in st.views(one, v).items():
            assert mine[k].shape == x.shape and mine[k].tobytes() == x.cpu().numpy().tobytes(), (v, k)   # (a) bit for bit
        _check_against_the_restatement(mine, a, ws[v], v)                                       # (b)
        sels.setdefault(len(a[3]), []).append(mine["selected"].tolist())
    if name in L.DIFFER:                                                                        # seats of EQUAL inputs: only the weights differ
        assert any(len(s) > 1 and any(t != s[0] for t in s[1:]) for s in sels.values()), sels


def test_scores_sets_twins_tie_and_nan_input_scores():
    """``test_scores_seats_twins_tie_and_a_nan_input_score``'s rows under three weight sets: twin templates (equal rows, equal final
    scores), a NaN candidate score and a NaN fresh score, a fresh row without ReID (+inf); NaN inputs are compared with the seats entry
    only (the kernels' fmax drops a NaN where numpy's maximum keeps it, in every scores entry alike)."""
    from premvos_amd import track
    dev = _dev()
    F = 6
    fresh = _score_inputs(77, 1, F, no_reid=[4])
    fs, fe = fresh[4].copy(), fresh[5].copy()
    fs[2] = np.nan
    per = []
    for v, T in enumerate((3, 2, 4)):
        a = list(_score_inputs(40 + v, T, T + F))
        a[4][:T] = a[3]
        a[4][T:], a[5][T:] = fs, fe
        per.append(a)
    a = per[2]
    a[0][1], a[2][1], a[3][1], a[6][1], a[4][1] = a[0][0], a[2][0], a[3][0], a[6][0], a[4][0]    # template 1 := template 0
    per[0][4][1] = np.nan                                                                       # a candidate's score
    ws = L.weight_sets(3)
    st = track.SeatTable([(len(x[3]), F, 0, 0) for x in per])
    overlap, cs, ce, te, fs_rep, fe_rep = _pooled(per, dev)
    got = track.track_scores_sets(overlap, cs, ce, te, torch.from_numpy(fs).to(dev), torch.from_numpy(fe).to(dev), st, ws)
    for v in range(3):
        one = track.track_scores_seats(overlap, cs, ce, te, fs_rep, fe_rep, st, weights=ws[v])
        for k, x in st.views(one, v).items():
            assert st.views(got, v)[k].cpu().numpy().tobytes() == x.cpu().numpy().tobytes(), (v, k)
    tw = {k: x.cpu().numpy() for k, x in st.views(got, 2).items()}
    assert tw["final_score"][0] == tw["final_score"][1] and tw["selected"][0] == tw["selected"][1]
    assert np.array_equal(tw["weighted"][0], tw["weighted"][1])
    assert np.isfinite(st.views(got, 0)["weighted"].cpu().numpy()).all()                        # a non-finite weighted score counts as 0


# ------------------------------------------------------------------------------------------------------ the shared fresh block
@pytest.mark.parametrize("h,w", [(9, 7), (31, 45), (40, 56)])
def test_overlap_seats_with_one_shared_fresh_block(h, w):
    """Every seat's ``fresh_slot`` pointing at ONE block gives, per seat, what a pool with the block copied once per seat gives."""
    from premvos_amd import track
    dev = _dev()
    rng = np.random.default_rng(h + w)
    Ts, F = (2, 0, 5, 1), 7
    cands = [np.stack([_blobs(rng, h, w, 2) * rng.integers(1, 256) for _ in range(T)]).astype(np.uint8) if T else np.zeros((0, h, w), np.uint8)
             for T in Ts]
    fresh = np.stack([_blobs(rng, h, w, 2) for _ in range(F)]).astype(np.uint8)
    foreign = _blobs(rng, h, w, 3)[None].astype(np.uint8)
    at, rows_shared, rows_copied, parts_s, parts_c = 0, [], [], [], []
    for T, c in zip(Ts, cands):                                                                 # shared: [cands..., foreign, fresh]
        rows_shared.append([T, F, at, 0])
        parts_s.append(c)
        at += T
    for r in rows_shared:
        r[3] = at + 1
    shared = np.concatenate(parts_s + [foreign, fresh])
    at = 0
    for T, c in zip(Ts, cands):                                                                 # copied: [cands_v, fresh]... per seat
        rows_copied.append((T, F, at, at + T))
        parts_c += [c, fresh]
        at += T + F
    copied = np.concatenate(parts_c)
    st_s, st_c = track.SeatTable(rows_shared), track.SeatTable(rows_copied)
    a = track.mask_overlap_seats(torch.from_numpy(shared).to(dev), st_s)
    b = track.mask_overlap_seats(torch.from_numpy(copied).to(dev), st_c)
    for v, T in enumerate(Ts):
        if not T:
            continue
        x, y = st_s.views(a, v), st_c.views(b, v)
        for k in ("inter", "area_p", "area_t"):
            assert torch.equal(x[k], y[k]), (v, k)
        m = np.concatenate([cands[v], fresh]) != 0
        assert np.array_equal(x["area_p"].cpu().numpy(), m.reshape(len(m), -1).sum(1))
        assert np.array_equal(x["inter"].cpu().numpy(), (m[:T, None] & m[None]).reshape(T, len(m), -1).sum(2))
        assert int(x["inter"][:, T:].sum()) > 0 or h * w < 100                                  # the fresh block was met


# -------------------------------------------------------------------------------------------------------------------- eval
@pytest.mark.parametrize("h,w,V,T0", [(9, 7, 1, 1), (9, 7, 3, 3), (31, 45, 3, 3), (31, 45, 8, 20), (120, 200, 8, 20), (120, 200, 1, 3),
                                      (480, 854, 3, 3), (480, 854, 8, 1), (480, 854, 1, 20)])
def test_eval_seats_counts_equal_numpy(h, w, V, T0):
    from premvos_amd import prewarp, track
    dev = _dev()
    rng = np.random.default_rng(h * 7 + V * 31 + T0)
    N, lead = 4, 3
    R_ = V * T0 + lead + 2
    first = (lead + (V - 1 - np.arange(V)) * T0).astype(np.int32)                               # reverse seat order, 3 planes in front
    gts = []
    for _ in range(2):
        gt = np.zeros((h, w), np.uint8)
        for i in rng.permutation(T0 + 2):                                                       # ids 1 .. T0 + 2: two of them above T0
            if T0 >= 2 and i == 1:
                continue                                                                        # id 2 is absent from the annotation
            gt[_blobs(rng, h, w, 1) != 0] = i + 1
        gts.append(gt)
    planes = np.zeros((2, R_, h, w), np.uint8)
    for f in range(2):
        planes[f] = 9                                                                           # planes of no seat: never read
        for v in range(V):
            for k in range(T0):
                m = _blobs(rng, h, w, 2) if (v + k + f) % 4 else np.zeros((h, w), np.uint8)     # some planes are all zero
                if k == 0 and v == 0:
                    m = (gts[f] == 1).astype(np.uint8)                                          # one exact hit
                planes[f, first[v] + k] = m * (1 if k % 2 else 255)                             # nonzero = foreground
    outs = []
    for _ in range(2):
        counts = torch.zeros((V, N, T0, 3), dtype=torch.int64, device=dev)
        for f, t in enumerate((0, 2)):                                                          # two frames into one tensor
            track.track_eval_seats(torch.from_numpy(planes[f]).to(dev), torch.from_numpy(gts[f]).to(dev), first, T0, counts, t)
        outs.append(counts.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])                                                     # two launches: the same bits
    got = outs[0]
    want = np.zeros((V, N, T0, 3), np.int64)
    for f, t in enumerate((0, 2)):
        for v in range(V):
            for k in range(T0):
                r, g = planes[f, first[v] + k] != 0, gts[f] == k + 1
                want[v, t, k] = np.count_nonzero(r & g), np.count_nonzero(r | g), np.count_nonzero(r)
    assert np.array_equal(got, want)
    assert not got[:, 1].any() and not got[:, 3].any() and got[:, 0].any() and got[:, 2].any()  # unwritten slices stay zero
    assert got[0, 0, 0].tolist() == [int((gts[0] == 1).sum())] * 3                              # the exact hit: |R and G| = |R or G| = |R|
    mine = prewarp.scores_from_counts(got)
    assert mine.shape == (V, T0)
    for v in range(V):
        assert np.array_equal(mine[v], PR.scores_from_counts(got[v]))


# ------------------------------------------------------------------------------------------------------ the group, real engines
SEARCH_SEED = 7


def _gts(lay, name, n):
    return np.array([L.read_gt(os.path.join(lay["anns"], name, f"{t:05d}.png")) for t in range(n)])


def test_one_seat_is_the_tracker_byte_for_byte(tmp_path):
    """120x200, 5 frames, 3 objects: ``search_video`` with one weight set (the default) gives ``do_video``'s id maps byte for byte -- the
    same plans and launches -- and its scores are eval_video of them."""
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(tmp_path)
    _video(lay, "clip", 5, 3, seed=SEARCH_SEED)
    a = track.do_video(os.path.join(lay["images"], "clip") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"], lay["out"], ref_eng, reid_eng,
                       record=True, tracker=track.Tracker(ref_eng, reid_eng, record=True))
    r = track.search_video("clip", lay, track.live_search_weights(1), ref_eng, reid_eng, record=True)
    assert r["frames"] == 5 and r["idmaps"].shape == (1, 5, 120, 200) and r["scores"].shape == (1, 3) and r["counts"].shape == (1, 5, 3, 3)
    for t in range(5):
        assert r["idmaps"][0, t].tobytes() == a[t]["png"].tobytes(), t
        for k in ("selected", "weighted", "planes", "final_score", "object_score", "labels"):
            assert r["logs"][0][t][k].tobytes() == a[t][k].tobytes(), (t, k)
    assert np.unique(a[0]["png"]).tolist() == [0, 1, 2, 3] and a[-1]["png"].any()
    want = PR.eval_video(r["idmaps"][0], _gts(lay, "clip", 5), 3)
    assert np.array_equal(r["scores"][0], want) and (want > 0).any()


def test_three_sets_in_three_seats_against_the_replayed_restatement(tmp_path):
    """6 frames, 3 objects, the weight sets (default, (1,0,0,0,0), (0,0,0,1,0)) in three seats.  What the engines returned to each seat is
    replayed into the restatement under that seat's weights: selections and id maps equal, weighted scores and planes within 1e-12,
    scores[i] = eval_video of seat i's id maps exactly, as many refinement and ReID calls per seat as the sequential loop makes, and the
    seats do not all select alike.

    Margins (``track_restated.margins``: weighted / paint; SEARCH_SEED = 7 was chosen on the GPU among the seeds 1 .. 16): seat 0 (the
    default weights) 6.3e-3 / 2.4e-3, both asserted >= 1e-6 (seeds 5, 8 and 16 have a paint margin of 0 there, seed 15 one of 2.3e-5).
    The two one-hot seats have NO margin for any of the 16 seeds, 0 / 0 each, and cannot have one.  Under (1,0,0,0,0) the weighted row
    of EVERY template is the objectness plane, so in frame 0 the three annotation objects (score 1.0 each) tie exactly and all
    templates choose the same candidate.  Under (0,0,0,1,0) a row is the IoU plane: the reduced-depth nets refine different boxes to
    masks that coincide, and candidates without overlap are exact zeros.  For these seats the comparison does not lean on a margin:
    their weighted scores must EQUAL the restatement's -- the one plane that enters is reproduced bit for bit, every other product is an
    exact zero -- so ties are exact on both sides and are broken by the same rules (first maximum; equal final scores: the higher index
    is painted last).  That asks more of the kernel than a margin would, and is what the margins are for: selections and id maps that
    do not hang on the last bits."""
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(tmp_path)
    n = 6
    _video(lay, "clip", n, 3, seed=SEARCH_SEED)
    ws = L.THREE_SETS
    r = track.search_video("clip", lay, ws, ref_eng, reid_eng, record=True)
    gts = _gts(lay, "clip", n)
    assert r["scores"].shape == (3, 3) and r["idmaps"].shape == (3, n, 120, 200)
    all_sel = []
    for v in range(3):
        calls = r["engine_logs"][v]
        assert sum(c["call"] == "refine" for c in calls) == n - 1 and sum(c["call"] == "reid" for c in calls) == n
        eng = R.ReplayEngines([x["mask"] for x in calls if x["call"] == "refine"], [x["ReID"] for x in calls if x["call"] == "reid"],
                              [x["bbox"] for x in calls if x["call"] == "refine"])
        ref, want = L.do_video(os.path.join(lay["images"], "clip") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"],
                               eng.do_refinement, eng.add_ReID, ws[v])
        assert len(ref) == n and eng.n_refine == n - 1 and eng.n_reid == n
        mw, mp = R.margins(ref)
        print(f"seat {v}: weighted margin {mw:.3e}, paint margin {mp:.3e}, scores {r['scores'][v].tolist()}, "
              f"selections {[x['selected'].tolist() for x in ref]}")
        for t, (x, y) in enumerate(zip(r["logs"][v], ref)):
            assert x["selected"].tolist() == y["selected"].tolist(), (v, t)
            assert np.abs(x["weighted"] - y["weighted"]).max() <= TOL and np.abs(x["planes"] - y["planes"]).max() <= TOL, (v, t)
            if _one_hot(ws[v]):
                assert np.array_equal(x["weighted"], y["weighted"]), (v, t)
            assert np.array_equal(x["idmap"], y["png"]) and np.array_equal(r["idmaps"][v, t], y["png"]), (v, t)
        if not _one_hot(ws[v]):                                                                 # (the one-hot seats: exact, see the docstring)
            assert mw >= 1e-6 and mp >= 1e-6, (v, mw, mp)
        assert np.array_equal(r["scores"][v], want) and np.array_equal(want, PR.eval_video(r["idmaps"][v], gts, 3)), v
        all_sel.append([x["selected"].tolist() for x in r["logs"][v]])
    assert any(all_sel[a] != all_sel[b] for a in range(3) for b in range(a + 1, 3)), all_sel    # the weights are not ignored
    assert r["idmaps"].any()


def test_two_sets_with_more_boxes_than_the_reid_engine_embeds_at_once(tmp_path):
    """4 frames, 3 objects, the first two of the three sets above (default, (1,0,0,0,0)) with a ReID engine of ``max_boxes`` 4: the
    step's nA = 6 masks go through ``ReIDEngine.embed_masks`` in chunks of 4 (4 + 2, both padded to 4 slots) instead of the net's single
    launch, and ``bbox`` is made contiguous.  Checked like the three sets above: seat 0 with both margins >= 1e-6 (SEARCH_SEED: weighted /
    paint 1.4e-2 / 2.4e-3 on the GPU; they are printed), the one-hot seat (no margin, 0 / 0) with EQUAL weighted scores."""
    from premvos_amd import track
    from premvos_amd.reid import ReIDEngine
    ref_eng, reid_eng = _engines()
    small = ReIDEngine(reid_eng.net, max_boxes=4)
    lay = _lay(tmp_path)
    n = 4
    _video(lay, "clip", n, 3, seed=SEARCH_SEED)
    ws = L.THREE_SETS[:2]
    r = track.search_video("clip", lay, ws, ref_eng, small, record=True)
    gts = _gts(lay, "clip", n)
    assert r["scores"].shape == (2, 3) and r["idmaps"].shape == (2, n, 120, 200)
    for v in range(2):
        calls = r["engine_logs"][v]
        assert sum(c["call"] == "refine" for c in calls) == n - 1 and sum(c["call"] == "reid" for c in calls) == n
        eng = R.ReplayEngines([x["mask"] for x in calls if x["call"] == "refine"], [x["ReID"] for x in calls if x["call"] == "reid"],
                              [x["bbox"] for x in calls if x["call"] == "refine"])
        ref, want = L.do_video(os.path.join(lay["images"], "clip") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"],
                               eng.do_refinement, eng.add_ReID, ws[v])
        assert len(ref) == n and eng.n_refine == n - 1 and eng.n_reid == n
        mw, mp = R.margins(ref)
        print(f"seat {v}: weighted margin {mw:.3e}, paint margin {mp:.3e}, scores {r['scores'][v].tolist()}, "
              f"selections {[x['selected'].tolist() for x in ref]}")
        for t, (x, y) in enumerate(zip(r["logs"][v], ref)):
            assert x["selected"].tolist() == y["selected"].tolist(), (v, t)
            assert np.abs(x["weighted"] - y["weighted"]).max() <= TOL and np.abs(x["planes"] - y["planes"]).max() <= TOL, (v, t)
            if _one_hot(ws[v]):
                assert np.array_equal(x["weighted"], y["weighted"]), (v, t)
            assert np.array_equal(x["idmap"], y["png"]) and np.array_equal(r["idmaps"][v, t], y["png"]), (v, t)
        if not _one_hot(ws[v]):
            assert mw >= 1e-6 and mp >= 1e-6, (v, mw, mp)
        assert np.array_equal(r["scores"][v], want) and np.array_equal(want, PR.eval_video(r["idmaps"][v], gts, 3)), v
    assert r["idmaps"].any()


def test_nine_sets_make_two_rounds(tmp_path):
    """W = 9 on a 4-frame video: a round of 8 seats and a round of 1.  Set 0's scores are the W = 1 run's; the second round's only seat
    gives the counts of a one-set search with set 8; the json lists 9 sets."""
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    lay = _lay(tmp_path)
    _video(lay, "clip", 4, 2, seed=SEARCH_SEED)
    ws = track.live_search_weights(9, seed=2)
    one = track.search_video("clip", lay, ws[:1], ref_eng, reid_eng)
    nine = track.search_video("clip", lay, ws, ref_eng, reid_eng)
    assert nine["scores"].shape == (9, 2) and nine["counts"].shape == (9, 4, 2, 3) and nine["frames"] == 4
    assert np.array_equal(nine["scores"][0], one["scores"][0])
    last = track.search_video("clip", lay, ws[8:], ref_eng, reid_eng)                           # the second round alone: one seat, Tracker's bytes
    assert np.array_equal(nine["counts"][8], last["counts"][0])
    res = track.live_search_result({"clip": nine}, ws, 2)
    assert len(res["weights"]) == len(res["mean"]) == len(res["videos"]["clip"]["scores"]) == 9 and res["frames"] == 4
    assert all(0 <= s <= 1 for row in res["videos"]["clip"]["scores"] for s in row) and res["best"] == int(np.argmax(res["mean"]))
    json.dumps(res)


# ------------------------------------------------------------------------------------------------------------ the commands
def test_the_commands_on_a_tree(tmp_path, capsys):
    """``track --search 3 --seed 1``, ``--live-weights 1,1,1,1,1`` and ``--search --check-only`` on the ``_make_tree`` tree of
    test_gpu_plumbing: 'bear' with the ids 1, 2 annotated in every frame, 'camel' with empty annotations (no templates: skipped)."""
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
    for name, n in videos.items():
        ann_dir = root / "data" / "DAVIS" / "Annotations" / "480p" / name
        ann_dir.mkdir(parents=True)
        for t in range(n):
            ann = np.zeros((120, 200), np.uint8)
            if name == "bear":
                ann[20:70, 30 + 2 * t:90 + 2 * t] = 1
                ann[60:110, 120 - t:180 - t] = 2
            R.write_index_png(str(ann_dir / f"{t:05d}.png"), ann)
    cwd = os.getcwd()
    try:
        assert stream.main(["--root", str(root), "--batch", "2", "--flow_weights", "weights/pwc.pth.tar", "--general_weights",
                            "weights/proposal_general_weights", "--specific_weights", "weights/specific.pt", "--refinement_weights",
                            "weights/refinement_specific_weights"]) == 0
        os.chdir(root / "code")
        assert qd.main(["ReID_net/configs/run"]) == 0
        os.chdir(cwd)
        assert track.main(["--root", str(root), "--search", "3", "--seed", "1"]) == 0
        out = root / "output"
        assert not [d for d in os.listdir(out) if d.startswith(("final", "eval", "overlay", "viz"))]     # no PNG, eval file or overlay
        res = json.loads((out / "live_search.json").read_text())
        assert set(res) == {"videos", "weights", "seed", "mean", "frames", "best", "skipped"} and res["seed"] == 1 and res["frames"] == 4
        assert res["weights"] == track.live_search_weights(3, 1).tolist() and list(res["videos"]) == ["bear"]
        scores = np.array(res["videos"]["bear"]["scores"])
        assert scores.shape == (3, 2) and ((scores >= 0) & (scores <= 1)).all()
        assert res["mean"] == [float(np.mean(s)) for s in scores] and res["best"] == int(np.argmax(res["mean"]))
        assert list(res["skipped"]) == ["camel"] and "no templates" in res["skipped"]["camel"]
        capsys.readouterr()
        assert track.main(["--root", str(root), "--live-weights", "1,1,1,1,1"]) == 0
        assert not (out / "final").exists() and "final_weights" in capsys.readouterr().out
        pal = track.voc_palette().reshape(-1)
        for name, n in videos.items():
            files = sorted(os.listdir(out / "final_weights" / name))
            assert files == [f"{t:05d}.png" for t in range(n)]
            for fn in files:
                im = Image.open(out / "final_weights" / name / fn)
                px = np.array(im)
                assert im.mode == "P" and px.shape == (120, 200) and np.array_equal(np.array(im.getpalette(), np.uint8), pal)
                assert set(np.unique(px)) <= ({0, 1, 2} if name == "bear" else {0})
        assert np.array(Image.open(out / "final_weights" / "bear" / "00000.png")).any()
        gone = root / "data" / "DAVIS" / "Annotations" / "480p" / "bear" / "00002.png"
        gone.unlink()
        capsys.readouterr()
        assert track.main(["--root", str(root), "--search", "3", "--check-only"]) == 2
        text = capsys.readouterr().out
        assert str(gone) in text and "--search" in text
    finally:
        os.chdir(cwd)
