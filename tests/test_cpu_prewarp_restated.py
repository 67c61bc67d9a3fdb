"""tests/prewarp_restated.py against what MergeTrack/oldmerge.py itself computed (tests/golden/prewarp_ref.npz, written by
tools/make_golden_prewarp.py): planes within 1e-12 (numpy's dot order), selections, id maps and eval_video's scores exactly."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prewarp_restated as R  # noqa: E402

REF = np.load(os.path.join(HERE, "golden", "prewarp_ref.npz"), allow_pickle=False)
G = json.load(open(os.path.join(HERE, "golden", "prewarp_host_refs.json")))


def test_fixture_is_data_under_the_margin_condition():
    assert os.path.getsize(os.path.join(HERE, "golden", "prewarp_ref.npz")) < 300 * 1000
    assert min(G["min_margin_column"], G["min_margin_row"], G["min_margin_paint"]) >= 1e-6
    assert G["videos"]["alpha"]["zero_score_rows"] >= 1 and G["videos"]["alpha"]["no_reid"]
    assert [o["start"] for o in G["videos"]["alpha"]["objects"]] == [0, 0, 2] and len(G["videos"]["beta"]["objects"]) == 1
    t, p = G["videos"]["alpha"]["no_reid"][0]
    assert np.isinf(REF["v_alpha_emb"][t, p]).all()
    assert np.allclose(R.normalised(), G["normalised_weights"], rtol=0, atol=0) and R.WEIGHTS.tolist() == G["weights"]


@pytest.mark.parametrize("tag,n", (("reid3", 3), ("reid1", 2)))
def test_reid_planes(tag, n):
    emb_t = REF[f"{tag}_emb_t"]
    frames = [{"reid": REF[f"{tag}_emb_p_{f}"], "ann": [{"id": k + 1, "reid": e} for k, e in enumerate(emb_t)] if f == 0 else []} for f in range(n)]
    reid, oreid = R.reid_planes(frames)
    for f in range(n):
        assert reid[f].shape == REF[f"{tag}_reid_{f}"].shape
        assert np.abs(reid[f] - REF[f"{tag}_reid_{f}"]).max(initial=0) <= 1e-12 and np.abs(oreid[f] - REF[f"{tag}_oreid_{f}"]).max(initial=0) <= 1e-12
    if tag == "reid3":
        assert (reid[0][:, 2] == 0).all() and (oreid[0][:, 2] == 1).all()            # the proposal without ReID
    else:
        assert all((o == 1).all() for o in oreid)                                    # a single template


@pytest.mark.parametrize("tag", ("planes3", "planes1"))
def test_warp_planes(tag):
    w = G["w"]
    masks, cur = np.unpackbits(REF[f"{tag}_masks"], axis=-1)[..., :w], np.unpackbits(REF[f"{tag}_current"], axis=-1)[..., :w]
    want = REF[f"{tag}_out"]
    warp = np.array([[R.mask_iou(m, c) for m in masks] for c in cur])
    assert np.array_equal(want[0], np.repeat(REF[f"{tag}_score"][None], len(cur), 0))
    assert np.array_equal(want[1], REF[f"{tag}_reid"]) and np.array_equal(want[2], REF[f"{tag}_oreid"])
    assert np.abs(warp - want[3]).max() <= 1e-12 and np.abs(R.other_max_plane(warp) - want[4]).max() <= 1e-12
    if tag == "planes3":
        assert (want[3][1] == 0).all()                                               # the empty current mask


@pytest.mark.parametrize("name", ("alpha", "beta"))
def test_do_video(name):
    frames = R.fixture_video(REF, G, name)
    out = R.merge_video(frames, G["h"], G["w"])
    for t in range(len(frames)):
        assert np.abs(out["planes"][t] - REF[f"v_{name}_planes_{t}"]).max() <= 1e-12
        assert np.abs(out["weighted"][t] - REF[f"v_{name}_weighted_{t}"]).max() <= 1e-12
    assert np.array_equal(out["chosen"], REF[f"v_{name}_chosen"])
    assert np.abs(out["best"] - REF[f"v_{name}_best"]).max() <= 1e-12
    assert np.array_equal(out["idmap"], REF[f"v_{name}_png"])
    T0 = R.check_first_frame_ids(frames)
    assert np.array_equal(R.eval_video(out["index"], REF[f"v_{name}_gt"], T0), REF[f"v_{name}_eval"])
    if name == "alpha":
        assert (out["best"][:2, 2] == 0).any() and (out["idmap"][2:] == 3).any() and not (out["idmap"][:2] == 3).any()
        off = R.merge_video(R.fixture_video(REF, G, name, late=False), G["h"], G["w"])
        assert not (off["idmap"] == 3).any() and off["chosen"].shape == (5, 2)


def test_rules_of_our_own():
    h, w = 4, 8
    m = np.zeros((3, h, w), np.uint8)
    m[0, :, :4], m[1, :, 2:6], m[2, 0, 7] = 1, 1, 1
    e = np.zeros((3, R.EMB))
    e[1, 0], e[2, 1] = 1.0, 2.0
    ann = [{"id": 1, "mask": m[0], "fwd": m[0], "reid": e[0]}]
    f0 = {"score": np.array([0.5, 0.5, 0.5]), "mask": m, "fwd": m, "reid": e, "ann": ann}
    f1 = {"score": np.zeros(0), "mask": np.zeros((0, h, w), np.uint8), "fwd": np.zeros((0, h, w), np.uint8), "reid": np.zeros((0, R.EMB)), "ann": []}
    out = R.merge_video([f0, f1, f0], h, w)
    assert out["chosen"][1, 0] == -1 and out["best"][1, 0] == 0 and not out["idmap"][1].any()      # a frame without proposals
    assert out["planes"][2][3].max() == 0                                                            # ... carries the empty mask
    assert R.paint_order(np.array([0.5, np.nan, 0.5, 0.1])) == [3, 0, 2, 1]                          # equal: the higher index last; NaN last
    assert R.first_max(np.array([1.0, np.nan, 3.0, np.nan]))[1] == 1
    assert R.mask_iou(m[0], m[2]) == 0.0
    with pytest.raises(ValueError, match="ids 1 .. T0"):
        R.check_first_frame_ids([{"ann": [{"id": 2}]}])
    ws = R.search_weights(4, 3)
    assert ws.shape == (4, 5) and np.array_equal(ws[0], R.normalised()) and np.allclose(ws.sum(1), 1)
    assert np.array_equal(ws[1:], R.search_weights(4, 3)[1:]) and not np.array_equal(ws[1], R.search_weights(4, 4)[1])
