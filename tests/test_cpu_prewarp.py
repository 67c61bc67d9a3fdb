"""The host side of the pre-warp merge (no GPU): header / binding / document agreement of the four entries of prewarp_ops.hip, their
argument checks (before any HIP call, so they run here), the bit layout of the host helpers, the tables and the command line."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ENTRIES = (("premvos_bits_overlap_i32", 12), ("premvos_prewarp_reid_f64", 12), ("premvos_prewarp_chain_f64", 21), ("premvos_prewarp_paint_bits_u8", 20))


def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "prewarp_ops.hip")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.premvos_abi_version() == 21                           # additive: the version stays
    for name, nargs in ENTRIES:
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert decl.count(",") + 1 == nargs, name
        assert f'extern "C" int {name}(' in src
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for cite in ("oldmerge.py:87-110", "oldmerge.py:112-127", "oldmerge.py:114-116", "oldmerge.py:176-208", "merge_functions.py:613-634"):
        assert cite in hdr, cite
    assert src.startswith("// hipcc-flags: -ffp-contract=off\n") and "#if" not in src and "atomicAdd(dst" in src
    assert not re.search(r"atomicAdd\([^)]*(float|double)", src)


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.int64)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused
    blocks = np.array([[0, 2, 4, 1, 0, 0, 0, 0], [2, 2, 6, 2, 5, 1, 2, 3]], np.int32)           # a 2-frame video: P = 2, 2; one object, in frame 0
    poff, first = np.array([0, 2, 4], np.int32), np.array([0, 1, 1], np.int32)

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    def overlap(bits=one, S=10, stride=8, hw=60, bh=blocks, bd=one, B=2, inter=one, ni=8, areas=one, na=8):
        return lib.premvos_bits_overlap_i32(bits, S, stride, hw, None if bh is None else bh.ctypes.data, bd, B, inter, ni, areas, na, None)

    def reid(ep=one, et=one, sumP=4, T=1, ph=poff, pd=one, N=2, flat=one, maxd=one):
        return lib.premvos_prewarp_reid_f64(ep, et, sumP, T, None if ph is None else ph.ctypes.data, pd, N, flat, maxd, one, one, None)

    def chain(inter=one, ni=8, na=8, bh=blocks, ph=poff, fh=first, N=2, T=1, wts=one, W=1, chosen=one, weighted=None):
        return lib.premvos_prewarp_chain_f64(inter, ni, one, na, None if bh is None else bh.ctypes.data, one, ph.ctypes.data, one, fh.ctypes.data, one,
                                             N, T, one, one, one, wts, W, chosen, one, weighted, None)

    def paint(bits=one, S=10, stride=8, hw=60, bh=blocks, fh=first, ids=one, ann0=4, N=2, T=1, W=1, idmap=one, gt=None, T0=0, counts=None):
        return lib.premvos_prewarp_paint_bits_u8(bits, S, stride, hw, bh.ctypes.data, one, fh.ctypes.data, one, ids, ann0, one, one, N, T, W, idmap, gt,
                                                 T0, counts, None)

    for f in (overlap, paint):
        refused(f(bits=None), b"null")
        refused(f(S=0), b"bad dims")
        refused(f(hw=0), b"bad dims")
        refused(f(stride=12), b"multiple of 8")
        refused(f(stride=8, hw=65), b"multiple of 8")                                           # 65 bits do not fit 8 bytes
        refused(f(bits=one + 4), b"8-byte aligned")
    refused(overlap(bh=None), b"null")
    refused(overlap(bd=None), b"null")
    refused(overlap(inter=None), b"null")
    refused(overlap(B=-1), b"bad dims")
    refused(overlap(S=7), b"outside the pool")                                                  # block 1's columns 6, 7
    refused(overlap(ni=7), b"do not fit")
    refused(overlap(na=7), b"do not fit")
    bad = blocks.copy()
    bad[1, 1] = -1
    refused(overlap(bh=bad), b"outside the pool")
    assert overlap(B=0) == 0                                                                    # nothing to do, nothing launched
    refused(reid(et=None), b"null")
    refused(reid(ep=None), b"null")
    refused(reid(T=0), b"bad dims")
    refused(reid(T=65), b"at most 64")
    refused(reid(sumP=5), b"poff")
    refused(reid(ph=np.array([0, 3, 2], np.int32), sumP=2), b"descends")
    refused(chain(wts=None), b"null")
    refused(chain(chosen=None), b"null")
    refused(chain(inter=None), b"null")
    refused(chain(T=65), b"at most 64")
    refused(chain(W=0), b"bad dims")
    refused(chain(W=2, weighted=one), b"one weight set")
    refused(chain(fh=np.array([0, 1, 2], np.int32)), b"first")                                  # first runs to 2, T is 1
    refused(chain(bh=bad), b"the video's tables ask")
    refused(chain(ni=7), b"do not fit")
    big = np.array([[0, 257, 300, 1, 0, 0, 0, 0]], np.int32)
    refused(chain(bh=big, ph=np.array([0, 257], np.int32), fh=np.array([0, 1], np.int32), N=1, ni=257, na=258), b"LDS")
    wide = np.array([[0, 201, 300, 40, 0, 0, 0, 0]], np.int32)                                  # 201 x 40 = 8040 scores
    refused(chain(bh=wide, ph=np.array([0, 201], np.int32), fh=np.array([0, 40], np.int32), N=1, T=40, ni=201 * 40, na=241), b"LDS")
    refused(paint(ids=None), b"null")
    refused(paint(idmap=None), b"neither")
    refused(paint(W=2), b"one weight set")
    refused(paint(T=65), b"at most 64")
    refused(paint(counts=one), b"bit planes")
    refused(paint(counts=one, gt=one, T0=2), b"bit planes")                                     # T0 > T
    refused(paint(ann0=10), b"annotation masks")
    refused(paint(S=3), b"outside the pool")


def test_bit_layout_of_the_host_helpers():
    from premvos_amd import prewarp as pw
    assert [pw.row_bytes(n) for n in (1, 64, 65, 1551, 2240, 409920)] == [8, 8, 16, 200, 280, 51240]
    rng = np.random.default_rng(0)
    for h, w in ((3, 5), (33, 47), (8, 8)):
        m = (rng.random((4, h, w)) < 0.4).astype(np.uint8) * rng.integers(1, 255, (4, h, w)).astype(np.uint8)
        bits = pw.pack_bits_host(m)
        assert bits.shape == (4, pw.row_bytes(h * w)) and bits.dtype == np.uint8
        flat = m.reshape(4, -1) != 0
        for i in (0, 7, 8, h * w - 1):
            assert np.array_equal((bits[:, i // 8] >> (i % 8)) & 1, flat[:, i])                 # bit k of byte i = pixel 8 i + k
        assert not np.unpackbits(bits, axis=1, bitorder="little")[:, h * w:].any()              # zero beyond h*w
        assert np.array_equal(pw.unpack_bits_host(bits, h, w), (m != 0).astype(np.uint8))
        words = bits.view(np.uint64)
        assert np.array_equal(np.array([[bin(int(x)).count("1") for x in r] for r in words]).sum(1), flat.sum(1))


def test_tables_weights_and_scores():
    import prewarp_restated as R
    from premvos_amd import _lib, prewarp as pw
    tab = pw.Tables([3, 0, 2], [2, 0, 1])
    assert (tab.N, tab.sumP, tab.T, tab.S) == (3, 5, 3, 16) and tab.poff.tolist() == [0, 3, 3, 5] and tab.first.tolist() == [0, 2, 2, 3]
    assert tab.blocks.tolist() == [[0, 3, 10, 2, 0, 0, 0, 0], [3, 0, 5, 3, 13, 2, 6, 5], [3, 2, 8, 0, 15, 0, 6, 10]]
    assert (tab.n_inter, tab.n_areas) == (6, 12) and tab.blocks.dtype == np.int32
    tab.check_caps()
    for P, A in (([257], [1]), ([4], [65]), ([201], [40])):
        with pytest.raises(_lib.PremvosError, match="LDS"):
            pw.Tables(P, A).check_caps()
    pw.Tables([200], [40]).check_caps()                                                         # T = 40, P = 128 and more fit
    assert np.array_equal(pw.WEIGHTS, R.WEIGHTS) and np.array_equal(pw.normalised(), R.normalised())
    assert np.array_equal(pw.search_weights(7, 3), R.search_weights(7, 3))
    rng = np.random.default_rng(2)
    idx, gt = rng.integers(0, 4, (6, 9, 11)), rng.integers(0, 4, (6, 9, 11))
    gt[2][gt[2] == 1] = 0
    idx[2][idx[2] == 1] = 0                                                                     # absent and not painted: 1
    gt[3][gt[3] == 2] = 0                                                                       # absent but painted: 0
    c = R.region_counts(idx, gt, 3)
    assert np.array_equal(pw.scores_from_counts(c[None])[0], R.scores_from_counts(c))
    with pytest.raises(_lib.PremvosError, match="ids 1 .. T0"):
        pw.first_frame_ids([{"ann": [{"id": 1}, {"id": 3}]}])
    assert pw.first_frame_ids([{"ann": [{"id": 1}, {"id": 2}]}]) == 2
    assert pw.first_frame_ids([{"ann": []}]) == 0 == R.check_first_frame_ids([{"ann": []}])   # no object in frame 0: nothing scored, as the restatement


def test_command_line(tmp_path, capsys):
    from PIL import Image
    from premvos_amd import track
    for argv, word in ((["--prewarp", "--lockstep", "2"], "--lockstep"), (["--prewarp", "--weights", "1,2,3"], "--weights"),
                       (["--prewarp", "--weights", "1,2,x,4,5"], "--weights"), (["--prewarp", "--weights", "0,0,0,0,0"], "--weights"),
                       (["--weights", "1,2,3,4,5"], "only with --prewarp"), (["--late-annotations"], "only with --prewarp"),
                       (["--prewarp-search", "-2"], "--prewarp-search"), (["--prewarp-search", "two"], "--prewarp-search")):
        with pytest.raises(SystemExit) as e:
            track.main(["--root", "/nonexistent"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert track.main(["--root", "/nonexistent", "--prewarp", "--check-only"]) == 2             # accepted; the inputs are what is missing
    assert "refinement_net" not in capsys.readouterr().out
    assert track.main(["--root", "/nonexistent", "--check-only"]) == 2
    assert "refinement_net" in capsys.readouterr().out                                          # without the flag: as it always was
    with pytest.raises(SystemExit):
        track.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--prewarp", "--weights", "--late-annotations", "--prewarp-search", "--seed", "oldmerge.py:220-221", "output/final_prewarp", "merge.py:78"):
        assert word in text, word
    root = str(tmp_path)                                                                        # a video whose frames differ in size
    for sub in ("data/DAVIS/JPEGImages/480p/v", "output/intermediate/ReID_proposals/v", "output/intermediate/flow/v", "code/ReID_net/configs"):
        os.makedirs(os.path.join(root, sub))
    open(os.path.join(root, "code/ReID_net/configs/live"), "w").write("{}")
    Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(os.path.join(root, "data/DAVIS/JPEGImages/480p/v/00000.jpg"))
    Image.fromarray(np.zeros((8, 16, 3), np.uint8)).save(os.path.join(root, "data/DAVIS/JPEGImages/480p/v/00001.jpg"))
    with pytest.raises(SystemExit) as e:
        track.main(["--root", root, "--prewarp"])
    assert e.value.code == 2 and "differ in size" in capsys.readouterr().err
    for flag in ("--eval", "--overlay"):                                                        # the search writes no id maps
        with pytest.raises(SystemExit) as e:
            track.main(["--root", "/nonexistent", "--prewarp-search", "3", flag])
        assert e.value.code == 2 and "not with --eval / --overlay" in capsys.readouterr().err
    assert track.main(["--root", "/nonexistent", "--prewarp", "--eval", "--overlay", "--check-only"]) == 2     # accepted with --prewarp
