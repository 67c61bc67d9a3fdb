"""Host side of `premvos_amd.stream --reid` (no GPU): the command line and its two refusals, the JSON the writer emits, the C-ABI
entries of the device path and their build."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flags_and_defaults(monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    a = stream.parse_args([])
    assert a.reid is False and a.reid_config == "code/ReID_net/configs/run" and a.gather is False
    a = stream.parse_args(["--reid", "--reid_config", "code/ReID_net/configs/other", "--gpus", "2"])
    assert a.reid is True and a.reid_config == "code/ReID_net/configs/other" and a.gpus == 2
    assert stream.parse_args(["--gather"]).gather is True                    # alone, both stay what they were
    monkeypatch.setenv("PREMVOS_SIDECAR", "1")
    assert stream.parse_args(["--batch", "4"]).batch == 4


def test_reid_with_gather_or_sidecar_is_refused_at_argument_time(tmp_path, monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    with pytest.raises(SystemExit) as e:
        stream.main(["--root", str(tmp_path / "nowhere"), "--reid", "--gather"])
    assert "--reid" in str(e.value) and "--gather" in str(e.value) and str(e.value).count(". ") == 0      # one sentence
    monkeypatch.setenv("PREMVOS_SIDECAR", "1")
    with pytest.raises(SystemExit) as e:
        stream.main(["--root", str(tmp_path / "nowhere"), "--reid"])
    assert "--reid" in str(e.value) and "PREMVOS_SIDECAR=1" in str(e.value) and str(e.value).count(". ") == 0
    monkeypatch.setenv("PREMVOS_SIDECAR", "0")
    assert stream.parse_args(["--reid"]).reid is True
    assert not (tmp_path / "nowhere").exists()
    with pytest.raises(SystemExit):                                          # the library entry refuses the pair as well
        stream.run(str(tmp_path), "seq_to_run.txt", "a", "b", "c", "d", gather=True, reid_config="code/ReID_net/configs/run")


def _refined(n, rng):
    from premvos_amd import rle
    out = []
    for i in range(n):
        m = np.zeros((12, 20), np.uint8)
        if i % 3:
            m[2:7 + i % 4, 3 + i:9 + i] = 1
        out.append({"bbox": [round(float(rng.uniform(0, 9)), 1) for _ in range(4)], "score": round(float(rng.uniform(0, 1)), 2),
                    "segmentation": rle.encode(m), "conf_score": str(np.float32(rng.uniform(-1, 1)))})
    return out


def test_emitted_json_round_trips_and_equals_the_stage_drivers_form(tmp_path):
    """``stream.reid_lists`` on packed rows (128 float32 + the box as int32 bits): "ReID" exactly where w > 0 and h > 0, last in
    the dict, floats as forward_directory emits them (np.array(float32 row).tolist()); the refined dicts are not touched."""
    from premvos_amd import rle, stream
    rng = np.random.default_rng(0)
    frames = [_refined(4, rng), [], _refined(3, rng)]
    before = json.dumps(frames)
    flat = [q for fr in frames for q in fr]
    emb = rng.standard_normal((len(flat), 128)).astype(np.float32)
    emb[1, 0], emb[1, 1], emb[1, 2] = np.float32(1e-8), np.float32(-3.0), np.float32(0.1)
    boxes = np.array([rle.to_bbox(q["segmentation"]) for q in flat]).astype(np.int32)
    rows = np.concatenate([emb, boxes.view(np.float32)], axis=1)
    assert rows.shape == (7, 132)
    # two launches: slots 0..4 and 5..6 (a launch may end inside a frame)
    lists = stream.reid_lists(frames, [(flat[:5], rows[:5]), (flat[5:], rows[5:])])
    assert json.dumps(frames) == before
    assert [len(x) for x in lists] == [4, 0, 3]
    k = 0
    for fr, out in zip(frames, lists):
        for q, p in zip(fr, out):
            has = boxes[k][2] > 0 and boxes[k][3] > 0
            assert ("ReID" in p) == bool(has) == bool(k % 3 if k < 4 else (k - 4) % 3)
            assert {a: b for a, b in p.items() if a != "ReID"} == q
            if has:
                assert list(p)[-1] == "ReID" and p["ReID"] == np.array(emb[k]).tolist()
                assert np.array_equal(np.array(p["ReID"], np.float32), emb[k])         # nothing lost in the text
            k += 1
    for i, out in enumerate(lists):
        fn = tmp_path / f"{i}.json"
        stream._dump_json(str(fn), out)
        text = fn.read_text()
        assert json.dumps(json.load(open(fn))) == text
        stripped = [{a: b for a, b in p.items() if a != "ReID"} for p in json.loads(text)]
        assert json.dumps(stripped) == json.dumps(frames[i])


def test_header_table_and_counts_name_the_new_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    for name in ("premvos_mask_bbox_u8", "premvos_reid_context_boxes_i32", "premvos_reid_input_frames_u8"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["premvos_mask_bbox_u8"]) == 11 and len(_lib.SIGNATURES["premvos_reid_input_frames_u8"]) == 11
    assert _lib.ABI_VERSION == 21
    assert int(re.search(r"#define PREMVOS_MASK_BBOX_SLABS (\d+)", hdr).group(1)) == _lib.MASK_BBOX_SLABS
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert f"{len(declared)} entry points, ABI v{_lib.ABI_VERSION}" in text, doc
    for cite in ("ReIDForwarding.py:68-74", "Similarity.py:264-298", "maskApi.c rleToBbox"):
        assert cite in hdr


def test_library_builds_for_gfx950_and_validates_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21
    assert lib.premvos_mask_bbox_u8(None, 1, 4, 4, 16, 4, 0, None, None, None, None) == -1 and b"null" in lib.premvos_last_error()
    assert lib.premvos_reid_context_boxes_i32(None, 1, 4, 4, 0, None, None) == -1
    assert lib.premvos_reid_input_frames_u8(None, 1, 4, 4, None, None, 1, 128, 0, None, None) == -1
    buf = (np.zeros(64, np.int32)).ctypes.data
    assert lib.premvos_mask_bbox_u8(buf, 1, 4, 4, 8, 4, 0, buf, None, buf, None) == -1      # mask_stride smaller than a mask
    assert b"strides" in lib.premvos_last_error()
