"""The host side of the CRF boundary refinement (no GPU): the restatement (tests/crf_restated.py) on cases with a known answer, the
``Params`` parser and every refusal, header / binding / symbol / document agreement of the four premvos_crf_* entries, their argument
checks (before any HIP call, null stream, no device touched), the refusals of ``python -m premvos_amd.crf`` at argument time and
``--check-only`` on a small tree."""
import math
import os
import re

import numpy as np
import pytest
import torch

import crf_restated as X
import track_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"premvos_crf_unary_labels_f32": 10, "premvos_crf_norm_f32": 9, "premvos_crf_step_f32": 18, "premvos_crf_argmax_u8": 9}
TEXT = "sxy=22.4,srgb=7.7,compat=1.4,gsxy=0.22,gcompat=1.25,r=56,gr=1,iters=12,gt_prob=0.7"


# ------------------------------------------------------------------------------------------------------------- the restatement
def test_without_compatibility_the_map_stays():
    frame, idmap = X.synthetic(13, 17, 3, seed=1)
    r = X.refine(frame, idmap, 3, X.params(compat=0.0, gcompat=0.0, sxy=3.0, r=4, iters=3))
    assert torch.equal(r["labels"], idmap) and r["changed"] == 0
    assert torch.allclose(r["Q"], r["Q0"], rtol=0, atol=1e-15)


def test_a_constant_field_passes_through_an_interior_pixel():
    frame = torch.full((21, 23, 3), 97, dtype=torch.uint8)
    Q = torch.full((2, 21 * 23), 0.5, dtype=torch.float64)
    Q[1] = 0.25
    for sxy, srgb, Rw in ((2.0, None, 3), (3.0, 5.0, 4)):
        K = X.pair_weights(frame, sxy, srgb, Rw)
        m = X.message(K, X.normaliser(K), Q).reshape(2, 21, 23)
        inner = m[:, 2 * Rw:21 - 2 * Rw, 2 * Rw:23 - 2 * Rw]             # the pixel's window and its neighbours' windows are whole
        assert inner.numel() and (inner[0] - 0.5).abs().max() < 1e-12 and (inner[1] - 0.25).abs().max() < 1e-12


def test_the_normaliser_of_a_corner_is_the_hand_sum():
    rng = np.random.default_rng(0)
    frame = torch.from_numpy(rng.integers(0, 256, (6, 7, 3)).astype(np.uint8))
    sxy, srgb, Rw = 1.5, 20.0, 2
    n = X.normaliser(X.pair_weights(frame, sxy, srgb, Rw)).reshape(6, 7)
    f = frame.numpy().astype(np.float64)
    total = 0.0
    for y in range(0, 3):                                                # the window of (0, 0) clipped to the frame: 3 x 3 pixels
        for x in range(0, 3):
            total += math.exp(-(y * y + x * x) / (2 * sxy * sxy) - float(((f[y, x] - f[0, 0]) ** 2).sum()) / (2 * srgb * srgb))
    assert abs(float(n[0, 0]) - 1.0 / math.sqrt(total + 1e-20)) < 1e-14
    g = X.normaliser(X.pair_weights(frame, sxy, None, Rw)).reshape(6, 7)
    hand = sum(math.exp(-(y * y + x * x) / (2 * sxy * sxy)) for y in range(-2, 1) for x in range(-2, 1))      # the corner (5, 6)
    assert abs(float(g[5, 6]) - 1.0 / math.sqrt(hand + 1e-20)) < 1e-14


def test_the_unary_the_argmax_and_the_defaults():
    idmap = torch.tensor([[0, 2], [1, 1]], dtype=torch.uint8)
    U = X.unary_from_labels(idmap, 3, 0.7)
    assert U.shape == (3, 2, 2) and abs(float(U[0, 0, 0]) + math.log(0.7)) < 1e-15 and abs(float(U[1, 0, 0]) + math.log(0.15)) < 1e-15
    assert torch.equal(U.argmin(0).to(torch.uint8), idmap)
    assert torch.allclose(torch.softmax(-U, 0)[:, 0, 1], torch.tensor([0.15, 0.15, 0.7], dtype=torch.float64))
    Q = torch.tensor([[[0.4, 0.2]], [[0.4, 0.5]], [[0.2, 0.5]]])
    assert X.labels_of(Q).tolist() == [[0, 1]] and torch.allclose(X.margin_of(Q), torch.tensor([[0.0, 0.0]]))
    p = X.params()
    assert p["r"] == math.ceil(2.5 * p["sxy"]) == 56 and p["gr"] == max(1, math.ceil(2.5 * p["gsxy"])) == 1 and p["iters"] == 12
    assert X.params(sxy=3.0)["r"] == 8 and X.params(sxy=3.0, r=6)["r"] == 6


# --------------------------------------------------------------------------------------------------------------------- Params
def test_params_defaults_text_and_subsets():
    from premvos_amd import crf
    d = crf.Params()
    assert d.as_dict() == X.DEFAULTS                                                            # crf_davis.py:43-60's numbers, r = 56, gr = 1
    assert crf.Params.parse(None) == d and crf.Params.parse("") == d and crf.Params.parse(str(d)) == d
    p = crf.Params.parse(TEXT)
    assert p.as_dict() == {"sxy": 22.4, "srgb": 7.7, "compat": 1.4, "gsxy": 0.22, "gcompat": 1.25, "r": 56, "gr": 1, "iters": 12, "gt_prob": 0.7}
    p = crf.Params.parse(" sxy = 3 , gt_prob=0.5 ")
    assert (p.sxy, p.r, p.gt_prob, p.srgb, p.gr) == (3.0, 8, 0.5, d.srgb, 1)                    # the radius follows the sigma given
    assert crf.Params.parse("gsxy=0.8").gr == 2 and crf.Params.parse("gsxy=0.8,gr=0").gr == 0 and crf.Params.parse("sxy=30,r=64").r == 64
    assert crf.Params.parse("compat=0,gcompat=0,iters=0").iters == 0


@pytest.mark.parametrize("text, key", [
    ("sigma=3", "sigma"), ("sxy=0", "sxy"), ("sxy=-1", "sxy"), ("srgb=0", "srgb"), ("gsxy=nan", "gsxy"), ("sxy=abc", "sxy"), ("sxy", "sxy"),
    ("compat=-0.1", "compat"), ("gcompat=inf", "gcompat"), ("r=65", "r"), ("r=-1", "r"), ("gr=65", "gr"), ("r=5.5", "r"), ("sxy=30", "r"),
    ("iters=-1", "iters"), ("iters=1001", "iters"), ("iters=2.5", "iters"), ("gt_prob=0", "gt_prob"), ("gt_prob=1", "gt_prob"),
    ("gt_prob=1.5", "gt_prob"), ("sxy=3,sxy=4", "sxy"), ("x=3", "x")])
def test_params_refusals_name_the_key(text, key):
    from premvos_amd import crf
    with pytest.raises(ValueError, match="crf parameter '?" + re.escape(key) + r"\b"):
        crf.Params.parse(text)
    with pytest.raises(ValueError, match="an empty item"):
        crf.Params.parse("sxy=3,,r=2")


def test_params_constructor_refuses_like_the_parser():
    from premvos_amd import crf
    for kw, key in (({"r": 65}, "r"), ({"gr": -1}, "gr"), ({"sxy": 0.0}, "sxy"), ({"gt_prob": 1.0}, "gt_prob"), ({"iters": 1.5}, "iters"),
                    ({"compat": float("nan")}, "compat")):
        with pytest.raises(ValueError, match="crf parameter " + key):
            crf.Params(**kw)


# ----------------------------------------------------------------------------------------------------- header, binding, documents
def test_header_signatures_symbols_and_documents_agree():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "crf_ops.hip")).read()
    assert _lib.ABI_VERSION == 21 and len(declared) == 89
    for name, nargs in ENTRIES.items():
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs, name
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(([^;]*)\);", hdr, re.S)
        assert m and m.group(2).count(",") + 1 == nargs and "crf_davis.py:43-60" in m.group(1), name     # each declaration cites the reference
        assert f'extern "C" int {name}(' in src, name
    assert set(re.findall(r'extern "C" int (premvos_\w+)\(', src)) == set(ENTRIES)
    for bounds in re.findall(r"__launch_bounds__\((\w+)\)", src):
        n = int(bounds) if bounds.isdigit() else int(re.search(r"constexpr int %s = (\d+)" % bounds, src).group(1))
        assert n % 64 == 0, bounds
    for doc in ("README.md", "DESIGN.md"):
        assert "89 entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(name in text for name in ENTRIES), doc
    assert "8.11" in open(os.path.join(ROOT, "DESIGN.md")).read() and "premvos_amd.crf" in open(os.path.join(ROOT, "README.md")).read()


def test_library_built_for_gfx950_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21 and all(hasattr(lib, name) for name in ENTRIES)
    buf = np.zeros(1 << 16, np.uint8)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused
    p = [one + 4096 * i for i in range(8)]

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, word, lib.premvos_last_error())

    def unary(idmaps=p[0], n=1, h=4, w=4, L=3, prob=0.5, u=p[1], q0=p[2], flag=p[3]):
        return lib.premvos_crf_unary_labels_f32(idmaps, n, h, w, L, prob, u, q0, flag, None)

    def norm(frames=p[0], n=1, h=4, w=4, sxy=2.0, srgb=5.0, Rw=3, out=p[1]):
        return lib.premvos_crf_norm_f32(frames, n, h, w, sxy, srgb, Rw, out, None)

    def step(frames=p[0], u=p[1], q_in=p[2], n_g=p[3], n_b=p[4], n=1, h=4, w=4, L=3, gsxy=0.5, gR=1, gcompat=1.0, sxy=2.0, srgb=5.0, Rw=3,
             compat=1.0, q_out=p[5]):
        return lib.premvos_crf_step_f32(frames, u, q_in, n_g, n_b, n, h, w, L, gsxy, gR, gcompat, sxy, srgb, Rw, compat, q_out, None)

    def argmax(q=p[0], n=1, h=4, w=4, L=3, before=p[1], idmap=p[2], changed=p[3]):
        return lib.premvos_crf_argmax_u8(q, n, h, w, L, before, idmap, changed, None)

    for call, pointers in ((unary, ("idmaps", "u", "q0", "flag")), (norm, ("frames", "out")), (step, ("frames", "u", "n_g", "n_b", "q_out")),
                           (argmax, ("q", "before", "idmap", "changed"))):
        for name in pointers:
            refused(call(**{name: None}), b"null pointer")
        for dim in ("n", "h", "w"):
            refused(call(**{dim: 0}), b">= 1")
            refused(call(**{dim: -3}), b">= 1")
        refused(call(n=65536), b"bad dims")
        refused(call(h=1 << 14, w=(1 << 12) + 1), b"bad dims")
    for call in (unary, step, argmax):
        for L in (1, 0, 17, -2):
            refused(call(L=L), b"2 to 16 labels")
    for prob in (0.0, 1.0, -0.5, 1.5, float("nan")):
        refused(unary(prob=prob), b"gt_prob")
    for Rw in (-1, 65):
        refused(norm(Rw=Rw), b"radius 0 to 64")
        refused(step(Rw=Rw), b"radius 0 to 64")
        refused(step(gR=Rw), b"radius 0 to 64")
    for bad in (0.0, -1.0, float("nan")):
        refused(norm(sxy=bad), b"sxy > 0")
        refused(step(sxy=bad), b"> 0")
        refused(step(gsxy=bad), b"> 0")
        refused(step(srgb=bad), b"> 0")
    refused(norm(srgb=-1.0), b"srgb")
    refused(step(compat=float("inf")), b"finite")
    refused(step(gcompat=float("nan")), b"finite")
    refused(step(q_out=p[2]), b"q_out overlaps q_in")
    refused(step(q_out=p[2] + 4 * 3 * 16 - 4), b"q_out overlaps q_in")                          # the last float of q_in
    refused(step(q_out=p[2] - 4 * 3 * 16 + 4), b"q_out overlaps q_in")


# -------------------------------------------------------------------------------------------------------------------- the command
def _refused(capsys, parse, argv, *words):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    err = " ".join(capsys.readouterr().err.split())
    assert e.value.code == 2 and all(w in err for w in words), (argv, err)


def test_the_commands_refusals(capsys):
    from premvos_amd import crf
    p = crf.parse_args
    _refused(capsys, p, ["--root", "r"], "--input")
    _refused(capsys, p, ["--input", "final", "--out", "final"], "argument --out", "is the input")
    _refused(capsys, p, ["--input", "final_prewarp", "--out", "final"], "argument --out: not final")
    _refused(capsys, p, ["--input", "../x"], "invalid value")
    _refused(capsys, p, ["--input", "final", "--out", "a/b"], "invalid value")
    _refused(capsys, p, ["--input", "final", "--out", ""], "invalid value")
    _refused(capsys, p, ["--input", "final", "--params", "r=65"], "argument --params", "r=65")
    _refused(capsys, p, ["--input", "final", "--params", "colour=3"], "argument --params", "'colour'")
    _refused(capsys, p, ["--input", "final", "--params", "gt_prob=1"], "argument --params", "gt_prob")
    a = p(["--input", "final"])
    assert a.out == "final_crf" and a.crf == crf.Params() and not (a.eval or a.overlay or a.check_only) and a.videos is None
    a = p(["--input", "final_vote", "--out", "sharp", "--params", TEXT, "--eval", "--overlay", "--videos", "a,b"])
    assert a.out == "sharp" and a.crf == crf.Params.parse(TEXT) and a.eval and a.overlay and a.videos == "a,b"
    with pytest.raises(SystemExit):
        p(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--input", "--params TEXT", "crf_davis.py:43-60", "output/<out>.json", "--check-only"):
        assert word in text, word


def _tree(root, name, videos):
    from PIL import Image
    rng = np.random.default_rng(0)
    for video, (n, h, w) in videos.items():
        os.makedirs(os.path.join(root, "output", name, video))
        os.makedirs(os.path.join(root, "data/DAVIS/JPEGImages/480p", video))
        for t in range(n):
            a = np.zeros((h, w), np.uint8)
            a[1:3, 1 + t:4 + t] = 1 + t
            R.write_index_png(os.path.join(root, "output", name, video, f"{t:05d}.png"), a)
            Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "data/DAVIS/JPEGImages/480p", video, f"{t:05d}.jpg"))


def test_check_only_names_what_is_missing(tmp_path, capsys):
    from PIL import Image
    from premvos_amd import crf
    root = str(tmp_path)
    _tree(root, "final", {"a": (3, 6, 9), "b": (2, 5, 7)})
    images = os.path.join(root, "data/DAVIS/JPEGImages/480p")
    assert crf.check_tree(root, "final", ["a", "b"], images) == []
    assert crf.main(["--root", root, "--input", "final", "--check-only"]) == 0
    assert "2 videos" in capsys.readouterr().out and not os.path.exists(os.path.join(root, "output", "final_crf"))
    os.remove(os.path.join(images, "a", "00001.jpg"))                                          # a frame is missing
    os.remove(os.path.join(root, "output", "final", "b", "00000.png"))                         # a PNG is missing
    Image.fromarray(np.zeros((6, 10, 3), np.uint8)).save(os.path.join(images, "a", "00002.jpg"))      # a size differs
    assert crf.main(["--root", root, "--input", "final", "--check-only"]) == 2
    text = capsys.readouterr().out
    assert "a/00001.png: no frame" in text and "b/00000.jpg: no PNG" in text and "a/00002.png: its size (6, 9) is not the frame's (6, 10)" in text
    assert len(crf.check_tree(root, "final", ["a", "b"], images)) == 3
    assert crf.main(["--root", root, "--input", "final", "--videos", "b", "--check-only"]) == 2
    assert "a/00001" not in capsys.readouterr().out
    assert crf.main(["--root", root, "--input", "other", "--check-only"]) == 2
    assert "other is missing" in capsys.readouterr().out
    os.makedirs(os.path.join(root, "output", "empty"))
    assert crf.main(["--root", root, "--input", "empty", "--check-only"]) == 2
    assert "no video folders" in capsys.readouterr().out
