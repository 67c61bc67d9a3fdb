"""``Tracker.step_resident`` (premvos_amd.stream --track): the merge loop's frame on arrays that are in HBM already.  The yardstick is
``Tracker.step`` / ``_advance`` -- the route of a tree read from files, itself pinned against the reference's ``do_video`` by
tests/test_gpu_track.py -- and the bar is equality: the same kernels run on the same bits.  Also here: the two C-ABI entries the
resident step adds, against numpy bit for bit, and the rule that the step never synchronises with the host.
One process, no subprocess fan-out."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from premvos_amd import rle  # noqa: E402

H, W = 480, 854
THRESH = 0.7            # between the best score of the template that must select the empty proposal and everybody else's (see crafted_case)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


_ENGINES = []


def _engines():
    """The reduced real engines of tests/test_gpu_track.py (synthetic weights), once per process."""
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


# ------------------------------------------------------------------------------------------------------ the two new entries
def _inputs_ref(cs, ce, fs, rows, T, F):
    ps = np.concatenate([cs[:T], fs[:F]])
    box = rows[:F, 128:].copy().view(np.int32)
    fresh = rows[:F, :128].astype(np.float64)
    fresh[(box[:, 2] <= 0) | (box[:, 3] <= 0)] = np.inf
    return ps, np.concatenate([ce[:T], fresh])


@pytest.mark.parametrize("T,F", [(0, 1), (1, 0), (1, 1), (3, 1), (3, 100), (10, 0), (10, 100), (32, 0), (32, 1), (32, 100)])
def test_track_inputs_entry_equals_numpy_bit_for_bit(T, F):
    from premvos_amd import _lib
    rng = np.random.default_rng(100 * T + F)
    cs = rng.uniform(0.5, 1.0, max(T, 1))
    ce = rng.normal(0, 2, (max(T, 1), 128))
    fs = np.round(rng.uniform(0, 1, max(F, 1)), 2)
    rows = np.zeros((max(F, 1), 132), np.float32)
    rows[:, :128] = rng.normal(0, 2, (max(F, 1), 128)).astype(np.float32)
    rows[0, :4] = [np.float32(1e-8), np.float32(-3.0), np.float32(0.1), np.float32(16777217.0)]
    box = rng.integers(1, 300, (max(F, 1), 4)).astype(np.int32)
    if F >= 100:
        box[3, 2] = 0                      # w = 0
        box[7, 3] = 0                      # h = 0
        box[11, 2] = -5                    # a negative width
        box[13, 2:] = 0
        box[17, 3] = -2147483648
    rows[:, 128:] = box.view(np.float32)
    dev = _dev()
    d = [torch.from_numpy(x).to(dev) for x in (cs, ce, fs, rows)]
    ps = torch.full((T + F,), -7.0, dtype=torch.float64, device=dev)
    ep = torch.full((T + F, 128), -7.0, dtype=torch.float64, device=dev)
    lib = _lib.load()
    _lib.check(lib.premvos_track_inputs_f64(d[0].data_ptr() if T else None, d[1].data_ptr() if T else None, d[2].data_ptr() if F else None,
                                            d[3].data_ptr() if F else None, T, F, ps.data_ptr(), ep.data_ptr(), _lib.current_stream()))
    want_ps, want_ep = _inputs_ref(cs, ce, fs, rows, T, F)
    assert not np.isnan(want_ep).any()
    assert ps.cpu().numpy().tobytes() == want_ps.tobytes() and ep.cpu().numpy().tobytes() == want_ep.tobytes()
    if F >= 100:
        got = ep.cpu().numpy()[T:]
        assert all(np.isposinf(got[j]).all() for j in (3, 7, 11, 13, 17)) and np.isfinite(got[[0, 1, 2, 4, 99]]).all()


@pytest.mark.parametrize("T", [1, 3, 10, 32])
def test_track_next_entry_equals_numpy_bit_for_bit(T):
    from premvos_amd import _lib
    rng = np.random.default_rng(T)
    fs = rng.uniform(0, 1, T)
    fs[:min(T, 3)] = [0.0, 1e-10, 1 - 2.0 ** -53][:min(T, 3)]
    box = np.stack([rng.integers(0, W - 10, T), rng.integers(0, H - 10, T), rng.integers(1, 10, T), rng.integers(1, 10, T)], 1).astype(np.int32)
    special = [[0, 0, W, H], [0, 0, 0, 0], [W - 1, H - 1, 1, 1], [0, 17, 5, H - 17], [33, 0, W - 33, 9]]   # all four borders; the empty mask's
    box[-min(T, 5):] = special[:min(T, 5)]
    dev = _dev()
    fd, bd = torch.from_numpy(fs).to(dev), torch.from_numpy(box).to(dev)
    score = torch.full((T,), -7.0, dtype=torch.float64, device=dev)
    yx = torch.full((T, 4), -7.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().premvos_track_next_f32(fd.data_ptr(), bd.data_ptr(), T, score.data_ptr(), yx.data_ptr(), _lib.current_stream()))
    want_score = 0.5 * (fs + 1)                                                               # merge_functions.py:234
    want_yx = np.array([[b[1], b[0], b[1] + b[3], b[0] + b[2]] for b in box.tolist()], np.float32)   # what Tracker._advance builds
    assert score.cpu().numpy().tobytes() == want_score.tobytes() and yx.cpu().numpy().tobytes() == want_yx.tobytes()
    assert torch.equal(score, 0.5 * (fd + 1))                                                 # and what _advance computes on the device


# -------------------------------------------------------------------------------------- the resident step against the dict step
def _rect(y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def crafted_case(T, F, seed=0):
    """Templates / candidates / fresh proposals of one frame, as arrays.  With T >= 3 and F >= 1 (and the raised threshold THRESH):
    template 0's candidate is weak (score 0.55, an embedding far from the template's) while fresh proposal 0 has the candidate's
    mask, the template's embedding and score 0.99 -> template 0 selects index T (a FRESH proposal); template 2's candidate has score
    0.5 and an embedding far from its template's, and no proposal is near it -> its row stays below THRESH: the EMPTY proposal;
    every other template keeps its own strong candidate.  F = 20: fresh proposal 5 is an empty mask (box 0 0 0 0) whose ROW holds
    template 0's embedding and score 0.99 -- used as it stands it would score; the file has no "ReID" for it, so it must act as +inf.
    The numbers were checked with tests/track_restated.py on the CPU (margins in the test's assertions)."""
    rng = np.random.default_rng(1000 * T + 10 * F + seed)
    cols, rows_ = 5, 2
    slots = [(40 + 210 * r, 60 + 160 * c) for r in range(rows_) for c in range(cols)]
    tmasks = np.stack([_rect(y, y + 90 + 5 * t, x, x + 70 + 3 * t) for t, (y, x) in enumerate(slots[:T])])
    templ_emb = rng.normal(0, 2, (T, 128)).astype(np.float32).astype(np.float64)
    cand_emb = (templ_emb + rng.normal(0, 0.05, (T, 128))).astype(np.float32).astype(np.float64)
    cand_score = np.round(rng.uniform(0.9, 0.99, T), 4)
    if T >= 3:
        cand_score[0], cand_score[2] = 0.55, 0.5
        cand_emb[0] = rng.normal(0, 2, 128).astype(np.float32)
        cand_emb[2] = rng.normal(0, 2, 128).astype(np.float32)
    fmasks = np.zeros((F, H, W), np.uint8)
    femb = rng.normal(0, 2, (F, 128)).astype(np.float32)
    fscore = np.round(rng.uniform(0.5, 0.85, F), 2)
    for j in range(F):
        y, x = int(rng.integers(390, 440)), int(rng.integers(0, 700))
        fmasks[j] = _rect(y, y + int(rng.integers(5, 40)), x, x + int(rng.integers(20, 150)))                 # below the templates' rows
    if F >= 1:
        fmasks[0], femb[0], fscore[0] = tmasks[0], templ_emb[0].astype(np.float32), 0.99
    if F >= 20:
        fmasks[5], femb[5], fscore[5] = 0, templ_emb[0].astype(np.float32), 0.99
    return {"tmasks": tmasks, "templ_emb": templ_emb, "cand_emb": cand_emb, "cand_score": cand_score, "fmasks": fmasks, "femb": femb,
            "fscore": fscore, "ids": [2 * t + 1 for t in range(T)]}


def _tracker(case, **kw):
    """A Tracker in the state 'some frame of a video': the templates of ``case``, candidates with their own scores / embeddings."""
    from premvos_amd import track
    ref_eng, reid_eng = _engines()
    tr = track.Tracker(ref_eng, reid_eng, **kw)
    templates = [{"id": i, "segmentation": rle.encode(m), "score": 1.0, "ReID": e.tolist()}
                 for i, m, e in zip(case["ids"], case["tmasks"], case["templ_emb"])]
    tr.add_templates(templates, None)
    tr.cand_score = torch.from_numpy(case["cand_score"]).to(tr.device)
    tr.cand_emb = torch.from_numpy(case["cand_emb"]).to(tr.device)
    return tr


def _fresh_dicts(case):
    """What ``read_props`` returns for the frame: the embedding as Python floats, all-inf where the mask's box is empty."""
    out = []
    for m, e, s in zip(case["fmasks"], case["femb"], case["fscore"]):
        seg = rle.encode(m)
        bb = rle.to_bbox(seg)
        out.append({"bbox": bb, "score": float(s), "segmentation": seg, "conf_score": "0.5",
                    "ReID": np.array(e, np.float32).tolist() if bb[2] > 0 and bb[3] > 0 else np.inf * np.ones(128)})
    return out


def _fresh_arrays(case, dev):
    """The same proposals as the streaming driver holds them: masks, [F,132] rows (embedding + rleToBbox box bits), scores."""
    F = len(case["fmasks"])
    if F == 0:
        return None, None, None
    boxes = np.array([rle.to_bbox(rle.encode(m)) for m in case["fmasks"]]).astype(np.int32)
    rows = np.concatenate([case["femb"].astype(np.float32), boxes.view(np.float32)], axis=1)
    return (torch.from_numpy(case["fmasks"]).to(dev), torch.from_numpy(np.ascontiguousarray(rows)).to(dev),
            torch.tensor([float(s) for s in case["fscore"]], dtype=torch.float64).to(dev))


@pytest.mark.parametrize("T", [1, 3, 10])
@pytest.mark.parametrize("F", [0, 1, 20])
def test_resident_step_equals_the_dict_step(T, F):
    case = crafted_case(T, F)
    a = _tracker(case, record=True, score_thresh=THRESH)
    want = a.step(_fresh_dicts(case))
    P = T + F
    if T >= 3 and F >= 1:                                   # the three facts, on the yardstick's result
        sel = want["selected"].tolist()
        print(f"T={T} F={F}: selected {sel}, final {want['final_score'].tolist()}")
        assert sel[0] == T, "template 0 must select the fresh proposal 0"
        assert sel[2] == P, "template 2 must select the empty proposal"
        assert sel[1] == 1
        if F == 20:
            bb = rle.to_bbox(rle.encode(case["fmasks"][5]))
            assert bb[2] == 0 and bb[3] == 0 and (want["planes"][1][:, T + 5] == 0).all()       # no ReID: its ReID score is 0 everywhere
    b = _tracker(case, score_thresh=THRESH)
    fm, rows, sc = _fresh_arrays(case, b.device)
    got = b.step_resident(fm, rows, sc)
    for k in ("selected", "weighted", "planes", "final_score", "object_score", "labels"):
        assert got[k].cpu().numpy().tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    idmap = got["idmap"].wait().copy()
    got["idmap"].release()
    assert idmap.tobytes() == want["idmap"].cpu().numpy().tobytes()
    assert set(np.unique(idmap)) <= {0} | set(case["ids"])
    if F >= 20 and T >= 3:                                  # the row's finite embedding, had it been used, WOULD have changed the scores
        rows2 = rows.clone()
        rows2[5, 128:] = torch.from_numpy(np.array([0, 0, 4, 4], np.int32).view(np.float32)).to(rows2.device)
        c = _tracker(case, score_thresh=THRESH)
        other = c.step_resident(fm, rows2, sc)
        assert other["planes"].cpu().numpy().tobytes() != want["planes"].tobytes()
        other["idmap"].release()


def _advance_case():
    """Three objects; a flow that moves two of them by sub-pixel amounts and takes every sample of the third from outside the frame."""
    case = crafted_case(3, 1)
    case["tmasks"] = np.stack([_rect(60, 200, 80, 260), _rect(250, 420, 300, 520), _rect(100, 300, 680, 820)])
    case["fmasks"][0] = case["tmasks"][0]
    case["cand_score"] = np.array([0.97, 0.95, 0.93])
    case["cand_emb"] = case["templ_emb"].copy()
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([1.25 + 0.5 * np.sin(yy / 97.0), -0.75 + 0.5 * np.cos(xx / 131.0)], -1).astype(np.float32)
    flow[:, 600:, 0] = 3000.0                                                                  # every sample of x >= 600 lies outside
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frame[100:300, 200:500] //= 3
    return case, flow, frame


def test_resident_advance_equals_the_dict_advance_with_the_real_engines():
    from premvos_amd import mergetrack
    case, flow, frame = _advance_case()
    a = _tracker(case, record=True)
    assert a._direct
    want = a.step(_fresh_dicts(case), flow, frame)
    labels = torch.from_numpy(want["labels"]).to(a.device)
    refined = torch.stack([(labels == t + 1).to(torch.uint8) for t in range(3)])
    warped = mergetrack.warp_masks(refined, flow).cpu().numpy()
    assert refined[2].any() and not warped[2].any(), "object 2 must be painted in this frame and leave the next one entirely"
    assert warped[0].sum() > 1000 and warped[1].sum() > 1000
    b = _tracker(case)
    fm, rows, sc = _fresh_arrays(case, b.device)
    got = b.step_resident(fm, rows, sc, torch.from_numpy(flow).to(b.device), torch.from_numpy(frame).to(b.device))
    got["idmap"].release()
    assert got["selected"].cpu().numpy().tolist() == want["selected"].tolist()
    assert b.cand_score.cpu().numpy().tobytes() == a.cand_score.cpu().numpy().tobytes()
    assert b.cand_masks.cpu().numpy().tobytes() == a.cand_masks.cpu().numpy().tobytes()
    ea, eb = a.cand_emb.cpu().numpy(), b.cand_emb.cpu().numpy()
    print("next candidates' embeddings, max |resident - dict|:", float(np.abs(ea - eb).max()), " empty object's finite:", np.isfinite(ea[2]).all())
    assert np.isfinite(ea).all() and eb.tobytes() == ea.tobytes()
    assert a.cand_masks[:2].any()
    # and the frame after it: the carried state is used the same way (the empty object's finite embedding takes part in the scores)
    want2 = a.step(_fresh_dicts(case))
    got2 = b.step_resident(fm, rows, sc)
    for k in ("selected", "weighted", "planes", "final_score"):
        assert got2[k].cpu().numpy().tobytes() == np.ascontiguousarray(want2[k]).tobytes(), k
    assert got2["idmap"].wait().tobytes() == want2["idmap"].cpu().numpy().tobytes()
    got2["idmap"].release()


def test_more_objects_than_the_engines_hold_is_refused_with_a_message():
    from premvos_amd import _lib
    case = crafted_case(3, 1)
    b = _tracker(case)
    b.refinement_net = type(b.refinement_net)(b.refinement_net.net, max_boxes=2)
    fm, rows, sc = _fresh_arrays(case, b.device)
    flow = torch.zeros((H, W, 2), dtype=torch.float32, device=b.device)
    with pytest.raises(_lib.PremvosError, match="3 objects"):
        b.step_resident(fm, rows, sc, flow, torch.zeros((H, W, 3), dtype=torch.uint8, device=b.device))


# ----------------------------------------------------------------------------------------------- no synchronisation in the step
def test_ten_resident_steps_never_synchronise_with_the_host(monkeypatch):
    """torch.cuda.synchronize, Stream.synchronize, Event.synchronize, Tensor.cpu / .item / .numpy / .tolist are counted on this
    thread while ten consecutive frames go through ``step_resident`` (flow, refinement and ReID included): zero calls.  The engines'
    launch plans exist before the count starts (two frames through an identical tracker: building and tuning a plan is one-time
    set-up, not part of a step).  The ten id maps, read afterwards through their events, are the dict route's."""
    case, flow, frame = _advance_case()
    flow[:, 600:, 0] = flow[:, :254, 0]                                            # (nobody leaves the frame here)
    fresh = _fresh_dicts(case)
    a = _tracker(case)
    want = []
    for _ in range(10):
        want.append(a.step(fresh, flow, frame)["idmap"].cpu().numpy())
    dev = a.device
    fm, rows, sc = _fresh_arrays(case, dev)
    flow_d, frame_d = torch.from_numpy(flow).to(dev), torch.from_numpy(frame).to(dev)
    warm = _tracker(case)
    for _ in range(2):
        warm.step_resident(fm, rows, sc, flow_d, frame_d)["idmap"].release()
    b = _tracker(case)
    torch.cuda.synchronize()
    calls, me = [], threading.get_ident()

    def counted(owner, name):
        orig = getattr(owner, name)

        def wrapper(*args, **kw):
            if threading.get_ident() == me:
                calls.append(f"{getattr(owner, '__name__', owner)}.{name}")
            return orig(*args, **kw)
        monkeypatch.setattr(owner, name, wrapper)
    counted(torch.cuda, "synchronize")
    counted(torch.cuda.Stream, "synchronize")
    counted(torch.cuda.Event, "synchronize")
    for name in ("cpu", "item", "numpy", "tolist"):
        counted(torch.Tensor, name)
    slots = [b.step_resident(fm, rows, sc, flow_d, frame_d)["idmap"] for _ in range(10)]
    assert calls == [], calls
    monkeypatch.undo()
    torch.ones(1).item()
    for t, (slot, ref) in enumerate(zip(slots, want)):
        assert slot.wait().tobytes() == ref.tobytes(), t
        slot.release()


# ------------------------------------------------------------------------------------------------ the feed's layout, directly
def test_three_frames_over_a_chunk_store_equal_the_dict_route():
    """``ChunkStore`` as the refinement lane fills it (frames of 1, 0 and 1 fresh proposals behind T free slots each), then
    ``step_resident`` with ``stack`` / ``next_slots`` as the tracker thread passes them: frame 0 copies the templates into its free
    slots, its refined candidates land in frame 1's slots (no copy at frame 1: the stack's first T entries ARE the candidates), frame
    1 has no fresh proposal, and after frame 2 -- the end of the chunk, ``next_slots`` None -- the tracker owns its candidates.
    Every frame's scores, selection, id map and carried state equal the dict route's."""
    from premvos_amd.stream_track import ChunkStore
    case, flow, frame = _advance_case()
    flow[:, 600:, 0] = flow[:, :254, 0]
    fresh = _fresh_dicts(case)
    a, b = _tracker(case, record=True), _tracker(case)
    dev, T = b.device, 3
    st = torch.cuda.current_stream(dev)
    store = ChunkStore([1, 0, 1], T, H, W, dev, st)
    fm, rows, sc = _fresh_arrays(case, dev)
    store.masks.fill_(7)                                                            # whatever the allocator left there must not matter
    store.put(0, 0, fm, rows)
    store.put(2, 0, fm, rows)
    store.close([[float(case["fscore"][0])], [], [float(case["fscore"][0])]], st)
    st.wait_event(store.event)
    flow_d, frame_d = torch.from_numpy(flow).to(dev), torch.from_numpy(frame).to(dev)
    for k, props in enumerate((fresh, [], fresh)):
        want = a.step(props, flow, frame)
        stack, fr, rw, s, nxt = store.frame(k)
        assert (fr is None) == (k == 1) and (nxt is None) == (k == 2) and stack.shape[0] == T + len(props)
        before = b.cand_masks.data_ptr()
        got = b.step_resident(fr, rw, s, flow_d, frame_d, stack=stack, next_slots=nxt)
        assert (before == stack.data_ptr()) == (k > 0)                              # from frame 1 on the candidates are in place
        for key in ("selected", "weighted", "planes", "final_score", "labels"):
            assert got[key].cpu().numpy().tobytes() == np.ascontiguousarray(want[key]).tobytes(), (k, key)
        assert got["idmap"].wait().tobytes() == want["idmap"].cpu().numpy().tobytes(), k
        got["idmap"].release()
        assert b.cand_masks.cpu().numpy().tobytes() == a.cand_masks.cpu().numpy().tobytes(), k
        assert b.cand_emb.cpu().numpy().tobytes() == a.cand_emb.cpu().numpy().tobytes(), k
        assert b.cand_score.cpu().numpy().tobytes() == a.cand_score.cpu().numpy().tobytes(), k
        if nxt is not None:
            assert b.cand_masks.data_ptr() == nxt.data_ptr()
    assert b.cand_masks.data_ptr() not in (store.masks.data_ptr(),) and b.cand_masks.shape == (T, H, W)


def test_the_id_map_ring_can_be_page_locked_ahead_of_the_video():
    case = crafted_case(3, 1)
    b = _tracker(case)
    b.pin_idmap_ring(H, W)
    assert b._ring_made == b.ring_slots == b._ring.qsize()
    fm, rows, sc = _fresh_arrays(case, b.device)
    slot = b.step_resident(fm, rows, sc)["idmap"]
    assert b._ring_made == b.ring_slots and b._ring.qsize() == b.ring_slots - 1     # taken from the ring, none made
    slot.wait()
    slot.release()
