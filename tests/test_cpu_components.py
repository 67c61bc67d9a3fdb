"""The host side of the largest-component clean-up (no GPU): the restatement (tests/components_restated.py) on hand-made cases with a
known answer, the conditions the synthetic fixtures of the GPU tests must meet, header / binding / symbol / document agreement of the
three premvos_cc_* entries against include/premvos_post_hip.h (premvos_hip.h stays at 89 declarations, ABI v21), their argument checks
(before any HIP call, null stream, no device touched), the refusals of ``python -m premvos_amd.components`` at argument time and
``--check-only`` on a small tree."""
import os
import re

import numpy as np
import pytest

import components_restated as X
import track_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"premvos_cc_dilate_u8": 8, "premvos_cc_label_i32": 6, "premvos_cc_keep_largest_u8": 11}


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", list(X.hand_cases()))
def test_the_restatement_on_hand_made_cases(name):
    M, D, want, removed, ncomp = X.hand_cases()[name]
    r = X.keep_largest(M, 2, D)
    assert np.array_equal(r["idmap"], want) and r["removed"].tolist() == [removed] and r["components"].tolist() == [ncomp]


def test_the_dilation_is_a_clipped_box():
    rng = np.random.default_rng(0)
    for (H, W), D in (((7, 9), 1), ((7, 9), 2), ((12, 5), 3), ((12, 15), 4), ((20, 31), 7), ((6, 8), 16), ((30, 40), 100)):
        res = rng.random((H, W)) < 0.05
        res[rng.integers(H), rng.integers(W)] = True
        want = np.zeros((H, W), np.uint8)
        for y, x in zip(*np.nonzero(res)):
            want[max(0, y - D // 2):y + (D - 1) // 2 + 1, max(0, x - D // 2):x + (D - 1) // 2 + 1] = 1
        assert np.array_equal(X.dilate(res, D), want), (H, W, D)


def test_min_index_labels_and_raster_numbering():
    m = np.zeros((5, 7), np.uint8)
    m[0, 3] = m[1, 2] = m[4, 6] = m[3, 0] = 1
    lab = X.min_index_labels(m)
    assert lab[0, 3] == lab[1, 2] == 3 and lab[3, 0] == 21 and lab[4, 6] == 34 and (lab[m == 0] == -1).all()     # a diagonal joins
    comp, n = X.components(m)
    assert n == 3 and comp[0, 3] == comp[1, 2] == 1 and comp[3, 0] == 2 and comp[4, 6] == 3
    assert X.min_index_labels(np.zeros((3, 4), np.uint8)).tolist() == [[-1] * 4] * 3
    assert (X.min_index_labels(np.ones((3, 4), np.uint8)) == 0).all()


def test_absent_ids_and_ids_beyond_L_are_left_alone():
    M = np.zeros((12, 20), np.uint8)
    M[1:4, 1:4], M[8, 15], M[5:7, 5:9], M[10, 1] = 1, 1, 3, 7
    r = X.keep_largest(M, 4, 1)
    assert r["removed"].tolist() == [1, 0, 0] and r["components"].tolist() == [2, 0, 1]
    assert r["idmap"][8, 15] == 0 and r["idmap"][10, 1] == 7 and (r["idmap"][5:7, 5:9] == 3).all()
    assert X.keep_largest(M)["removed"].shape == (7,)


@pytest.mark.parametrize("H, W, L, D", X.SYNTHETIC)
def test_the_synthetic_fixtures_meet_their_conditions(H, W, L, D):
    M = X.synthetic(H, W, L, X.SEED)
    assert M.dtype == np.uint8 and M.shape == (H, W) and int(M.max()) == L - 1
    r, r1 = X.keep_largest(M, L, D), X.keep_largest(M, L, 1)
    fg = int((M > 0).sum())
    assert r["removed"].sum() >= 0.05 * fg, (int(r["removed"].sum()), fg)
    assert int((r["idmap"] != M).sum()) == int(r["removed"].sum()) and set(np.unique(r["idmap"][r["idmap"] != M])) <= {0}
    if D > 1:
        assert (r["idmap"] != r1["idmap"]).any()
    assert np.array_equal(X.synthetic(H, W, L, X.SEED), M)


# ----------------------------------------------------------------------------------------------------- header, binding, documents
def test_header_signatures_symbols_and_documents_agree():
    from premvos_amd import _lib
    old = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "premvos_post_hip.h")).read()
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "components_ops.hip")).read()
    assert _lib.ABI_VERSION == 21 and len(set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", old))) == 89
    assert "premvos_cc_" not in old and not set(ENTRIES) & set(_lib.SIGNATURES)
    assert set(re.findall(r"^int (premvos_\w+)\(", hdr, re.M)) == set(ENTRIES) == set(_lib.POST_SIGNATURES)
    for name, nargs in ENTRIES.items():
        assert len(_lib.POST_SIGNATURES[name]) == nargs, name
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(([^;]*)\);", hdr, re.S)
        assert m and m.group(2).count(",") + 1 == nargs and "postproc.py:41-63" in m.group(1), name      # each declaration cites the reference
        assert f'extern "C" int {name}(' in src, name
    assert set(re.findall(r'extern "C" int (premvos_\w+)\(', src)) == set(ENTRIES)
    assert not re.search(r"\b(float|double|half)\b", re.sub(r"//[^\n]*", "", src))              # integers only
    for bounds in re.findall(r"__launch_bounds__\((\w+)\)", src):
        n = int(bounds) if bounds.isdigit() else int(re.search(r"constexpr int %s = (\d+)" % bounds, src).group(1))
        assert n % 64 == 0, bounds
    for doc in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "89 entry points, ABI v21" in text and "premvos_post_hip.h" in text, doc
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(name in text for name in ENTRIES), doc
    assert "8.12" in open(os.path.join(ROOT, "DESIGN.md")).read() and "premvos_amd.components" in open(os.path.join(ROOT, "README.md")).read()


def test_library_built_for_gfx950_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21 and all(hasattr(lib, name) for name in ENTRIES)
    buf = np.zeros(1 << 16, np.uint8)
    p = [buf.ctypes.data + 4096 * i for i in range(8)]                                          # never dereferenced: every call is refused

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    def dilate(idmaps=p[0], n=1, h=4, w=4, L=3, D=3, dil=p[1]):
        return lib.premvos_cc_dilate_u8(idmaps, n, h, w, L, D, dil, None)

    def label(masks=p[0], planes=1, h=4, w=4, labels=p[1]):
        return lib.premvos_cc_label_i32(masks, planes, h, w, labels, None)

    def keep(idmaps=p[0], labels=p[1], n=1, h=4, w=4, L=3, counts_ws=p[2], out_idmaps=p[3], removed=p[4], ncomp=p[5]):
        return lib.premvos_cc_keep_largest_u8(idmaps, labels, n, h, w, L, counts_ws, out_idmaps, removed, ncomp, None)

    for call, pointers, dims in ((dilate, ("idmaps", "dil"), ("n", "h", "w")), (label, ("masks", "labels"), ("planes", "h", "w")),
                                 (keep, ("idmaps", "labels", "counts_ws", "out_idmaps", "removed", "ncomp"), ("n", "h", "w"))):
        for name in pointers:
            refused(call(**{name: None}), b"null pointer")
        for dim in dims:
            for bad in (0, -3):
                refused(call(**{dim: bad}), b">= 1")
                assert dim.encode() in lib.premvos_last_error()
        refused(call(h=1 << 13, w=(1 << 13) + 1), b"h * w at most 2^26")
        refused(call(h=1 << 30, w=1 << 30), b"h * w at most 2^26")
    for call in (dilate, keep):
        for L in (1, 0, 257, -2):
            refused(call(L=L), b"L from 2 to 256")
    for D in (0, 256, -1):
        refused(dilate(D=D), b"D from 1 to 255")


# -------------------------------------------------------------------------------------------------------------------- the command
def _refused(capsys, parse, argv, *words):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    err = " ".join(capsys.readouterr().err.split())
    assert e.value.code == 2 and all(w in err for w in words), (argv, err)


def test_the_commands_refusals(capsys):
    from premvos_amd import components
    p = components.parse_args
    _refused(capsys, p, ["--root", "r"], "--input")
    _refused(capsys, p, ["--input", "final", "--out", "final"], "argument --out", "is the input")
    _refused(capsys, p, ["--input", "final_crf", "--out", "final"], "argument --out: not final")
    _refused(capsys, p, ["--input", "../x"], "invalid value")
    _refused(capsys, p, ["--input", "final", "--out", "a/b"], "invalid value")
    _refused(capsys, p, ["--input", "final", "--out", ""], "invalid value")
    for bad in ("0", "256", "-4"):
        _refused(capsys, p, ["--input", "final", f"--dilate={bad}"], "argument --dilate", "1 to 255")
    _refused(capsys, p, ["--input", "final", "--dilate", "3.5"], "argument --dilate")
    a = p(["--input", "final"])
    assert a.out == "final_cc" and a.dilate == 100 == components.DILATE == X.DILATE and not (a.eval or a.overlay or a.check_only) and a.videos is None
    a = p(["--input", "final_crf", "--out", "clean", "--dilate", "31", "--eval", "--overlay", "--videos", "a,b"])
    assert a.out == "clean" and a.dilate == 31 and a.eval and a.overlay and a.videos == "a,b"
    with pytest.raises(SystemExit):
        p(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--input", "--dilate D", "postproc.py:41-63", "output/<out>.json", "--check-only", "background"):
        assert word in text, word


def _listing(d):
    return sorted(os.path.join(b, f) for b, _, fs in os.walk(d) for f in fs)


def test_check_only_names_what_is_missing(tmp_path, capsys):
    from premvos_amd import components
    root = str(tmp_path)
    for video, (n, h, w) in {"a": (3, 6, 9), "b": (2, 5, 7)}.items():
        os.makedirs(os.path.join(root, "output", "final", video))
        for t in range(n):
            m = np.zeros((h, w), np.uint8)
            m[1:3, 1 + t:4 + t] = 1 + t
            R.write_index_png(os.path.join(root, "output", "final", video, f"{t:05d}.png"), m)
    assert components.check_tree(root, "final", ["a", "b"]) == []
    assert components.main(["--root", root, "--input", "final", "--check-only"]) == 0          # no frames under JPEGImages: not needed
    assert "2 videos" in capsys.readouterr().out
    assert components.main(["--root", root, "--input", "final", "--overlay", "--check-only"]) == 2      # ... but the overlay needs them
    assert "a/00000.png: no frame" in capsys.readouterr().out
    R.write_index_png(os.path.join(root, "output", "final", "a", "00001.png"), np.zeros((6, 10), np.uint8))      # a size differs
    os.makedirs(os.path.join(root, "output", "final", "c"))                                    # a video without PNGs
    before = _listing(root)
    assert components.main(["--root", root, "--input", "final", "--check-only"]) == 2
    text = capsys.readouterr().out
    assert "a: its PNGs differ in size ([(6, 9), (6, 10)])" in text and "c: no PNGs under" in text and "b:" not in text
    assert len(components.check_tree(root, "final", ["a", "b", "c"])) == 2
    assert components.main(["--root", root, "--input", "final", "--videos", "b", "--check-only"]) == 0
    capsys.readouterr()
    assert components.main(["--root", root, "--input", "other", "--check-only"]) == 2
    assert "other is missing" in capsys.readouterr().out
    os.makedirs(os.path.join(root, "output", "empty"))
    assert components.main(["--root", root, "--input", "empty", "--check-only"]) == 2
    assert "no video folders" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        components.main(["--root", root, "--input", "final", "--out", "final", "--check-only"])
    capsys.readouterr()
    assert _listing(root) == before                                                            # nothing was written
