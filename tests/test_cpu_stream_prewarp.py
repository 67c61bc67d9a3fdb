"""The host side of `stream --track --prewarp` (no GPU): header / binding / document agreement of premvos_mask_warp_pack_bits_u8, its
argument checks (before any HIP call, so they run here), the streaming driver's command line, and `prewarp.VideoIngest`'s tables."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "premvos_mask_warp_pack_bits_u8", 15


def test_header_binding_source_and_documents_name_the_entry():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "prewarp_ingest_ops.hip")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.premvos_abi_version() == 21                           # additive: the version stays
    assert NAME in declared and len(_lib.SIGNATURES[NAME]) == NARGS and hasattr(lib, NAME)
    decl = re.search(r"\bint " + NAME + r"\(([^;]*)\);", hdr).group(1)
    assert decl.count(",") + 1 == NARGS
    defn = re.search(r'extern "C" int ' + NAME + r"\(([^)]*)\)", src).group(1)
    assert defn.count(",") + 1 == NARGS
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    before = hdr[:hdr.index("int " + NAME)]
    comment = before[before.rindex("/*"):]
    assert "merge_functions.py:209-217" in comment and "oldmerge.py" in comment
    # the tap arithmetic is shared, not copied: one statement of it, included by both files; integer work only, no preprocessor branches
    merge = open(os.path.join(ROOT, "premvos_amd", "csrc", "merge_ops.hip")).read()
    for text in (src, merge):
        assert '#include "mask_warp_taps.h"' in text and "__float2int_rn" not in text
    assert "__float2int_rn" in open(os.path.join(ROOT, "premvos_amd", "csrc", "mask_warp_taps.h")).read()
    assert "#if" not in src and "atomic" not in src


def test_the_entry_refuses_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(1 << 16, np.int64)
    masks, cur, fwd, dev = buf.ctypes.data, buf.ctypes.data + (1 << 17), buf.ctypes.data + (1 << 18), buf.ctypes.data     # never dereferenced
    first, fof = np.array([0, 2, 2, 3], np.int32), np.array([0, 0, -1], np.int32)

    def call(masks=masks, n=3, h=5, w=13, fh=first, fd=dev, oh=fof, od=dev, flows=dev, nflows=1, V=3, cur=cur, fwd=fwd, rb=16):
        return lib.premvos_mask_warp_pack_bits_u8(masks, n, h, w, None if fh is None else fh.ctypes.data, fd, None if oh is None else oh.ctypes.data,
                                                  od, flows, nflows, V, cur, fwd, rb, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    for kw in ("masks", "fh", "fd", "oh", "od", "flows", "cur", "fwd"):
        refused(call(**{kw: None}), b"null")
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(h=1 << 16, w=1 << 15, rb=(1 << 31) // 8)):
        refused(call(**kw), b"bad dims")
    refused(call(V=0), b"1 to 4096")
    refused(call(V=4097), b"1 to 4096")
    refused(call(rb=9), b"row_bytes")                                                           # 65 pixels are two words
    refused(call(rb=8), b"row_bytes")
    refused(call(rb=24), b"row_bytes")
    refused(call(cur=cur + 4), b"8-byte aligned")
    refused(call(fh=np.array([1, 2, 2, 3], np.int32)), b"frame_first runs")
    refused(call(fh=np.array([0, 2, 2, 4], np.int32)), b"frame_first runs")
    refused(call(fh=np.array([0, 2, 1, 3], np.int32)), b"descends")
    refused(call(oh=np.array([0, 1, -1], np.int32)), b"outside [-1, 1)")
    refused(call(oh=np.array([0, -2, -1], np.int32)), b"outside [-1, 1)")
    refused(call(cur=masks + 64), b"overlap an output")
    refused(call(fwd=masks + 3 * 65 - 1), b"8-byte aligned")                                    # (alignment is asked first)
    refused(call(fwd=masks + 192), b"overlap an output")                                        # the masks' last 3 bytes
    refused(call(fwd=cur + 40), b"overlap each other")
    refused(call(n=3, h=8, w=8, rb=8, cur=masks + 192, fwd=masks + 192 + 16), b"overlap each other")     # rows 8 bytes: 24 per output


def test_the_streaming_driver_command_line(monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    new = ("prewarp", "weights", "late_annotations")
    a = stream.parse_args(["--track"])
    assert (a.prewarp, a.weights, a.late_annotations) == (False, None, False)                   # --track alone: no new key set
    old = {k: v for k, v in vars(a).items() if k not in new}
    assert old["track"] and old["reid"] and not old["eval"] and not old["overlay"] and not old["gather"]
    assert set(old) == {"root", "seq_file", "flow_weights", "general_weights", "specific_weights", "refinement_weights", "batch", "gpus", "shard",
                        "gather", "merge_share", "reid", "reid_config", "track", "track_refinement_config", "track_reid_config", "eval", "overlay"}
    plain = stream.parse_args([])
    assert not plain.track and not plain.reid and (plain.prewarp, plain.weights) == (False, None)
    a = stream.parse_args(["--track", "--prewarp"])
    assert a.track and a.reid and a.prewarp and a.weights is None
    assert {k: v for k, v in vars(a).items() if k not in new} == old                            # the flag changes nothing else
    a = stream.parse_args(["--track", "--prewarp", "--weights", "1,2,3,4,0", "--eval", "--overlay"])
    assert a.weights == [1.0, 2.0, 3.0, 4.0, 0.0] and a.eval and a.overlay
    opts = stream._prewarp_options(a.weights)
    assert opts["prewarp"] is True and opts["raw_weights"] == a.weights and np.allclose(opts["weights"], [0.1, 0.2, 0.3, 0.4, 0.0])
    from premvos_amd import prewarp as pw
    assert stream._prewarp_options(None)["weights"] == pw.normalised().tolist()

    def refused(argv, *words):
        with pytest.raises(SystemExit) as e:
            stream.parse_args(argv)
        for word in words:
            assert word in str(e.value), (argv, word, str(e.value))

    refused(["--prewarp"], "--prewarp", "needs --track", "premvos_amd.track --prewarp")
    refused(["--reid", "--prewarp"], "needs --track")
    refused(["--track", "--weights", "1,2,3,4,5"], "--weights", "only with --track --prewarp")
    refused(["--weights", "1,2,3,4,5"], "--weights")
    for bad in ("1,2,3", "1,2,x,4,5", "0,0,0,0,0", "1,2,3,4,-5", "1,2,3,4,nan"):
        refused(["--track", "--prewarp", "--weights", bad], "--weights", "invalid value", repr(bad))
    refused(["--track", "--prewarp", "--gather"], "--gather")
    refused(["--track", "--prewarp", "--late-annotations"], "--late-annotations", "premvos_amd.track --prewarp")
    refused(["--track", "--late-annotations"], "--late-annotations")
    monkeypatch.setenv("PREMVOS_SIDECAR", "1")
    refused(["--track", "--prewarp"], "PREMVOS_SIDECAR")


def test_the_mode_needs_no_refinement_config_and_refuses_videos_it_cannot_pool(tmp_path):
    from premvos_amd import prewarp as pw, stream
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "code/ReID_net/configs"))
    open(os.path.join(root, "code/ReID_net/configs/live"), "w").write("{}")
    cfgs = ("code/refinement_net/configs/live", "code/ReID_net/configs/live")
    assert len(stream.check_track_inputs(root, *cfgs)) == 1 and "refinement_net" in stream.check_track_inputs(root, *cfgs)[0]
    assert stream.check_track_inputs(root, *cfgs, prewarp=True) == []
    os.remove(os.path.join(root, "code/ReID_net/configs/live"))
    assert len(stream.check_track_inputs(root, *cfgs, prewarp=True)) == 1
    cap = 4 << 30
    assert stream.check_prewarp_video(104, [(480, 854)], 10, 40, cap) is None
    assert "differ in size" in stream.check_prewarp_video(5, [(8, 12), (8, 16)], 2, 40, cap)
    assert "LDS" in stream.check_prewarp_video(5, [(480, 854)], 65, 40, cap)                   # more templates than the chain kernel holds
    assert "LDS" in stream.check_prewarp_video(5, [(480, 854)], 40, 201, cap)                  # 40 x 201 scores
    need = pw.ingest_bytes(104, 40, 10, 480, 854)
    assert stream.check_prewarp_video(104, [(480, 854)], 10, 40, need) is None
    assert "PREMVOS_PREWARP_POOL_BYTES" in stream.check_prewarp_video(104, [(480, 854)], 10, 40, need - 1)
    assert 0.85e9 < need < 0.87e9                                                               # twice the 0.43 GB pool (see ingest_bytes)


def test_video_ingest_host_side_builds_upload_s_tables():
    from premvos_amd import prewarp as pw
    rng = np.random.default_rng(5)
    fields = ("N", "sumP", "T", "S", "cur0", "fwd0", "ann0", "annfwd0", "n_inter", "n_areas")
    for trial in range(40):
        N = int(rng.integers(1, 12))
        P = [int(x) for x in rng.integers(0, 7, N)]
        T = int(rng.integers(0, 4))
        ing = pw.VideoIngest(9, 11)
        ing.note_annotations(list(range(1, T + 1)))
        k, firsts = 0, []
        while k < N:                                                                            # a random chunking of the frames
            n = int(rng.integers(1, 5))
            firsts.append(ing.note_chunk(P[k:k + n]))
            k += n
        tab, ref = ing.tables(), pw.Tables(P, [T] + [0] * (N - 1))
        for f in fields:
            assert getattr(tab, f) == getattr(ref, f), (trial, f)
        for f in ("poff", "first", "blocks"):
            assert np.array_equal(getattr(tab, f), getattr(ref, f)) and getattr(tab, f).dtype == np.int32, (trial, f)
        assert firsts[0] == 0 and all(int(ref.poff[i]) >= 0 for i in range(N)) and set(firsts) <= set(ref.poff.tolist())
        h, w = 9, 11
        implied = (ref.S * pw.row_bytes(h * w) + ref.sumP * (8 + 128 * 8) + ref.T * 128 * 8
                   + (ref.blocks.size + ref.poff.size + ref.first.size + ref.T) * 4)
        assert implied <= pw.ingest_bytes(N, max(P), T, h, w), trial
    assert pw.ingest_bytes(104, 40, 0, 480, 854) >= 2 * 2 * 104 * 40 * pw.row_bytes(480 * 854)
    with pytest.raises(AssertionError):
        ing.note_annotations([1])                                                               # the objects are frame 0's: before any chunk
