"""The CRF boundary refinement on the GPU (csrc/crf_ops.hip's four premvos_crf_* entries through ctypes, ``crf.meanfield``,
``crf.refine_idmaps`` and ``python -m premvos_amd.crf``) against the fp64 brute-force restatement of the rule (tests/crf_restated.py).

Inputs: ``crf_restated.synthetic`` -- piecewise-constant colour regions, label boundaries 2 px off the colour boundaries, pixel noise of
sigma 5, 3 % label noise.  The fixture asserts on the restatement alone that at least 1 % of the pixels change label in the first two
cases and that at most 2 % of a case's pixels have an fp64 top-two margin below the exemption threshold.

Bars.  U, Q^0 and both normalisers: relative 1e-6 (one log, exp or rsqrt and an fp32 sum).  Q after round 1 and after the last round:
32 x d32, where d32 is the largest deviation of the restatement evaluated in fp32 on the CPU from the same in fp64 on that case (the
factor is for another summation order over up to 12 769 taps and the hardware's exponential); both figures are printed.  Labels: equal
wherever the fp64 margin exceeds twice the Q bar (a Q within the bar cannot flip such a pixel); ``changed``: the count recomputed
from the kernel's own labels, exactly."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crf_restated as X  # noqa: E402
import track_restated as R  # noqa: E402

REL = 1e-6
CASES = {                                                                                       # name -> (H, W, L, parameters, must flip)
    "37x53_L3": (37, 53, 3, dict(gsxy=0.8, gr=2, sxy=3.0, srgb=10.0, r=6, gt_prob=0.5), True),  # odd sizes, tile tails, window < frame
    "24x40_L4_r30": (24, 40, 4, dict(r=30, gt_prob=0.5), True),                                 # the window covers the frame from every pixel
    "33x70_L16": (33, 70, 16, dict(r=6), False),                                                # the label loop's ends
    "33x70_L2": (33, 70, 2, dict(r=6), False),
    "70x150_L3_default": (70, 150, 3, dict(), False),                                           # r = 56: several tiles and bands, whole and clipped windows
}
SEED = 11


def _dev():
    from premvos_amd import _lib
    _lib.require_gpu()
    return _lib.resolve_device(None)


def _params(p):
    from premvos_amd import crf
    return crf.Params(**p)


@functools.lru_cache(maxsize=None)
def _case(name, seed=SEED):
    """The inputs and the restatement's results of a case, computed once: "frame", "idmap", "p", "r64" (``crf_restated.refine`` in fp64),
    "d32", "bar" = 32 d32."""
    H, W, L, kw, must_flip = CASES[name]
    frame, idmap = X.synthetic(H, W, L, seed)
    p = X.params(**kw)
    r64, r32 = X.refine(frame, idmap, L, p), X.refine(frame, idmap, L, p, torch.float32)
    d32 = max(float((r32[k].double() - r64[k]).abs().max()) for k in ("Q1", "Q"))
    bar = 32 * d32
    changed, exempt = r64["changed"] / (H * W), float((r64["margin"] <= 2 * bar).double().mean())
    print(f"{name}: restatement: {changed:.4f} of the pixels change, d32 {d32:.3e}, Q bar {bar:.3e}, smallest margin {float(r64['margin'].min()):.3e}, "
          f"exempt {exempt:.4f}")
    assert not must_flip or changed >= 0.01, (name, changed)
    assert exempt <= 0.02, (name, exempt)
    assert 1e-8 < d32 < 1e-5, (name, d32)                                                       # (an fp32 evaluation: neither exact nor broken)
    return {"frame": frame, "idmap": idmap, "L": L, "p": p, "r64": r64, "d32": d32, "bar": bar}


def _rel(got, want):
    return float(((got.double().cpu() - want) / want).abs().max())


def _raw(frame, idmap, L, p):
    """One frame through the four entries themselves -> U, Q0, n_g, n_b, Q1 (device tensors without the frame axis)."""
    from premvos_amd import _lib
    dev = _dev()
    lib, s = _lib.load(), _lib.current_stream()
    f, m = frame[None].contiguous().to(dev), idmap[None].contiguous().to(dev)
    H, W = idmap.shape
    U, Q0, Q1 = (torch.full((1, L, H, W), float("nan"), device=dev) for _ in range(3))
    n_g, n_b = (torch.full((1, H, W), float("nan"), device=dev) for _ in range(2))
    flag = torch.full((1,), 7, dtype=torch.int32, device=dev)
    _lib.check(lib.premvos_crf_unary_labels_f32(m.data_ptr(), 1, H, W, L, p["gt_prob"], U.data_ptr(), Q0.data_ptr(), flag.data_ptr(), s), "unary")
    assert int(flag) == 0
    _lib.check(lib.premvos_crf_norm_f32(f.data_ptr(), 1, H, W, p["gsxy"], 0.0, p["gr"], n_g.data_ptr(), s), "norm g")
    _lib.check(lib.premvos_crf_norm_f32(f.data_ptr(), 1, H, W, p["sxy"], p["srgb"], p["r"], n_b.data_ptr(), s), "norm b")
    _lib.check(lib.premvos_crf_step_f32(f.data_ptr(), U.data_ptr(), Q0.data_ptr(), n_g.data_ptr(), n_b.data_ptr(), 1, H, W, L, p["gsxy"], p["gr"],
                                        p["gcompat"], p["sxy"], p["srgb"], p["r"], p["compat"], Q1.data_ptr(), s), "step")
    return U[0], Q0[0], n_g[0], n_b[0], Q1[0]


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernels_against_the_restatement(name):
    from premvos_amd import _lib, crf
    c = _case(name)
    dev, r64, p, L = _dev(), c["r64"], c["p"], c["L"]
    U, Q0, n_g, n_b, Q1 = _raw(c["frame"], c["idmap"], L, p)
    errs = {"U": _rel(U, r64["U"]), "Q0": _rel(Q0, r64["Q0"]), "n_g": _rel(n_g, r64["n_g"]), "n_b": _rel(n_b, r64["n_b"])}
    d1 = float((Q1.double().cpu() - r64["Q1"]).abs().max())
    frame, idmap = c["frame"].to(dev), c["idmap"].to(dev)
    Q = crf.meanfield(frame, U, _params(p))                                                     # the library path, from the kernel's own U
    dq = float((Q.double().cpu() - r64["Q"]).abs().max())
    print(f"{name}: relative errors {errs}; Q after round 1 off by {d1:.3e}, after round {p['iters']} by {dq:.3e}; d32 {c['d32']:.3e}, bar {c['bar']:.3e}")
    assert all(e <= REL for e in errs.values()), errs
    assert d1 <= c["bar"] and dq <= c["bar"], (d1, dq, c["bar"])
    assert float((Q.sum(0) - 1).abs().max()) < 1e-5
    out = crf.refine_idmaps(frame[None], idmap[None], L, _params(p))
    labels, changed = out["idmap"][0].cpu(), out["changed"].cpu()
    assert labels.dtype == torch.uint8 and changed.dtype == torch.int32 and changed.shape == (1,)
    sure = r64["margin"] > 2 * c["bar"]
    assert torch.equal(labels[sure], r64["labels"][sure]) and float((~sure).double().mean()) <= 0.02
    assert int(changed[0]) == int((labels != c["idmap"]).sum())                                 # from the kernel's own labels
    Qm = crf.meanfield(frame, -torch.log(Q0), _params(p))                                       # a unary that is not from labels: Q^0 by the step
    assert float((Qm.double().cpu() - r64["Q"]).abs().max()) <= c["bar"]
    lab2 = torch.empty_like(out["idmap"])                                                       # the argmax entry on its own: ties and counts
    ch2 = torch.full((1,), -5, dtype=torch.int32, device=dev)
    tie = Q.clone()[None]
    tie[0, :, 0, 0] = 0.25                                                                      # all equal: the lowest label
    tie[0, L - 1, 0, 1] = tie[0, 0, 0, 1] = 2.0                                                 # first and last equal and largest: the first
    _lib.check(_lib.load().premvos_crf_argmax_u8(tie.data_ptr(), 1, *idmap.shape, L, idmap[None].contiguous().data_ptr(), lab2.data_ptr(),
                                                 ch2.data_ptr(), _lib.current_stream()), "argmax")
    assert int(lab2[0, 0, 0]) == 0 and int(lab2[0, 0, 1]) == 0 and int(ch2[0]) == int((lab2[0] != idmap).sum())


def test_a_stack_equals_its_frames_and_chunks_do_not_show():
    """N = 3 frames of 37 x 53 in one call against three single calls, and ``refine_idmaps`` in chunks of 3, 2 + 1 and 1: equal bytes."""
    from premvos_amd import crf
    dev = _dev()
    H, W, L, kw, _ = CASES["37x53_L3"]
    pairs = [X.synthetic(H, W, L, seed) for seed in (SEED, SEED + 1, SEED + 2)]
    frames, maps = torch.stack([f for f, _ in pairs]).to(dev), torch.stack([m for _, m in pairs]).to(dev)
    p = _params(X.params(**kw))
    U, Q0 = crf.unary_from_labels(maps, L, p.gt_prob)
    Q = crf.meanfield(frames, U, p)
    assert Q.shape == (3, L, H, W)
    for t in range(3):
        assert torch.equal(crf.meanfield(frames[t], U[t], p), Q[t]), t
        ng, nb = crf.normalisers(frames[t:t + 1], p)
        ng3, nb3 = crf.normalisers(frames, p)
        assert torch.equal(ng[0], ng3[t]) and torch.equal(nb[0], nb3[t]), t
    whole = crf.refine_idmaps(frames, maps, L, p)
    per_frame = 3 * L * 4 * H * W
    for budget in (2 * per_frame, per_frame, 1):
        part = crf.refine_idmaps(frames, maps, L, p, chunk_bytes=budget)
        assert torch.equal(part["idmap"], whole["idmap"]) and torch.equal(part["changed"], whole["changed"]), budget
    assert torch.equal(whole["idmap"], Q.argmax(1).to(torch.uint8)) and not torch.equal(whole["idmap"], maps)
    assert whole["changed"].tolist() == (whole["idmap"] != maps).flatten(1).sum(1).tolist()


def test_meanfield_with_a_soft_unary():
    """Random probabilities, L = 3, 37 x 53: ``meanfield(frame, -log(clamp(p)))`` against the restatement of the same unary."""
    from premvos_amd import crf
    dev = _dev()
    H, W, L, kw, _ = CASES["37x53_L3"]
    frame, _ = X.synthetic(H, W, L, SEED)
    g = torch.Generator().manual_seed(5)
    prob = torch.softmax(2.0 * torch.randn((L, H, W), generator=g, dtype=torch.float64), 0)
    U32 = -torch.log(prob.clamp(1e-5, 1.0)).float()
    p = X.params(**kw)
    r64, r32 = X.meanfield(frame, U32.double(), p), X.meanfield(frame, U32, p, torch.float32)
    d32 = max(float((r32[k].double() - r64[k]).abs().max()) for k in ("Q0", "Q1", "Q"))
    assert 1e-8 < d32 < 1e-5
    Q = crf.meanfield(frame.to(dev), U32.to(dev), _params(p))
    Q1 = crf.meanfield(frame.to(dev), U32.to(dev), _params(dict(p, iters=1)))
    Q0 = crf.meanfield(frame.to(dev), U32.to(dev), _params(dict(p, iters=0)))
    errs = [float((a.double().cpu() - r64[k]).abs().max()) for a, k in ((Q0, "Q0"), (Q1, "Q1"), (Q, "Q"))]
    print(f"soft unary: Q0, Q1, Q off by {errs}; d32 {d32:.3e}, bar {32 * d32:.3e}")
    assert max(errs) <= 32 * d32, (errs, d32)
    assert float((Q.double().cpu() - r64["Q0"]).abs().max()) > 1e-3                             # the rounds did something


def test_a_label_beyond_L_is_reported_and_nothing_is_written():
    from premvos_amd import _lib, crf
    dev = _dev()
    H, W, L = 37, 53, 3
    frame, idmap = X.synthetic(H, W, L, SEED)
    bad = idmap.clone()
    bad[H - 1, W - 1] = L                                                                       # one pixel, the last
    m = torch.stack([idmap, bad]).to(dev)
    U, Q0 = (torch.full((2, L, H, W), -123.0, device=dev) for _ in range(2))
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    rc = lib.premvos_crf_unary_labels_f32(m.data_ptr(), 2, H, W, L, 0.5, U.data_ptr(), Q0.data_ptr(), flag.data_ptr(), _lib.current_stream())
    assert rc == -1 and b"label >= L" in lib.premvos_last_error()
    torch.cuda.synchronize()
    assert int(flag) != 0 and bool((U == -123.0).all()) and bool((Q0 == -123.0).all())
    with pytest.raises(_lib.PremvosError, match="label >= L"):
        crf.refine_idmaps(torch.stack([frame, frame]).to(dev), m, L, crf.Params(r=6))
    rc = lib.premvos_crf_unary_labels_f32(m.data_ptr(), 1, H, W, L, 0.5, U.data_ptr(), Q0.data_ptr(), flag.data_ptr(), _lib.current_stream())
    assert rc == 0 and int(flag) == 0 and bool((U[0] > 0).all()) and bool((U[1] == -123.0).all())      # the good frame alone is taken


# -------------------------------------------------------------------------------------------------------------------- the command
def _listing(d):
    return {os.path.join(b, f): (os.path.getsize(os.path.join(b, f)), os.path.getmtime(os.path.join(b, f))) for b, _, fs in os.walk(d) for f in fs}


def test_the_command_on_a_tree(tmp_path, capsys):
    """Two videos of 3 frames of 37 x 53 under output/final, the frames written as JPEGs, one video of background alone: the PNGs under
    output/final_sharp decode to the restatement's maps for the frames as ``jpeg.imread`` returns them; the json, the eval and the
    overlay files stand where the other tree tools put theirs; output/final is left as it was."""
    from PIL import Image
    from premvos_amd import crf, jpeg, track
    dev = _dev()
    root = str(tmp_path)
    H, W, L, kw, _ = CASES["37x53_L3"]
    text = "gsxy=0.8,gr=2,sxy=3,srgb=10,r=6,gt_prob=0.5"
    images, anns = os.path.join(root, "data/DAVIS/JPEGImages/480p"), os.path.join(root, "data/DAVIS/Annotations/480p")
    maps = {}
    for video in ("clip", "void"):
        for d in (os.path.join(root, "output", "final", video), os.path.join(images, video), os.path.join(anns, video)):
            os.makedirs(d)
        for t in range(3):
            frame, idmap = X.synthetic(H, W, L, SEED + t)
            if video == "void":
                idmap = torch.zeros_like(idmap)
            maps[video, t] = idmap
            Image.fromarray(frame.numpy()).save(os.path.join(images, video, f"{t:05d}.jpg"), quality=95)
            R.write_index_png(os.path.join(root, "output", "final", video, f"{t:05d}.png"), idmap.numpy())
            R.write_index_png(os.path.join(anns, video, f"{t:05d}.png"), idmap.numpy())
    before = _listing(os.path.join(root, "output", "final"))
    assert crf.main(["--root", root, "--input", "final", "--out", "final_sharp", "--params", text, "--eval", "--overlay"]) == 0
    said = capsys.readouterr().out
    out = os.path.join(root, "output")
    assert "final_sharp" in said and _listing(os.path.join(out, "final")) == before
    assert sorted(os.listdir(out)) == ["eval_final_sharp", "final", "final_sharp", "final_sharp.json", "overlay_final_sharp",
                                       "premvos_amd_davis_eval_final_sharp.json"]
    p = X.params(**kw)
    pal = track.voc_palette().reshape(-1)
    changed = []
    for t in range(3):
        im = Image.open(os.path.join(out, "final_sharp", "void", f"{t:05d}.png"))
        assert im.mode == "P" and not np.array(im).any() and np.array(im).shape == (H, W)
        im = Image.open(os.path.join(out, "final_sharp", "clip", f"{t:05d}.png"))
        got = torch.from_numpy(np.array(im))
        assert im.mode == "P" and np.array_equal(np.array(im.getpalette(), np.uint8), pal)
        frame = jpeg.imread(os.path.join(images, "clip", f"{t:05d}.jpg"), dev).cpu()
        r64, r32 = X.refine(frame, maps["clip", t], L, p), X.refine(frame, maps["clip", t], L, p, torch.float32)
        bar = 32 * max(float((r32[k].double() - r64[k]).abs().max()) for k in ("Q1", "Q"))
        sure = r64["margin"] > 2 * bar
        assert torch.equal(got[sure], r64["labels"][sure]) and float((~sure).double().mean()) <= 0.02, t
        assert r64["changed"] > 0
        changed.append(int((got != maps["clip", t]).sum()))
        for video in ("clip", "void"):
            assert os.path.getsize(os.path.join(out, "overlay_final_sharp", video, f"{t:05d}.jpg")) > 0
    res = json.load(open(os.path.join(out, "final_sharp.json")))
    assert set(res) == {"videos", "frames", "params", "source"} and res["frames"] == 6 and res["source"] == "output/final"
    assert res["params"] == crf.Params.parse(text).as_dict() and res["params"]["iters"] == 12
    assert res["videos"] == {"clip": {"frames": 3, "L": L, "changed": changed}, "void": {"frames": 3, "L": 1, "changed": [0, 0, 0]}}
    assert os.listdir(os.path.join(out, "eval_final_sharp")) == ["clip.json"]                   # (a video without objects is not scored)
    assert json.load(open(os.path.join(out, "premvos_amd_davis_eval_final_sharp.json")))
    high = maps["clip", 0].clone()                                                              # an id the CRF does not take: refused by name
    high[0, 0] = 16
    R.write_index_png(os.path.join(root, "output", "final", "clip", "00000.png"), high.numpy())
    from premvos_amd import _lib
    with pytest.raises(_lib.PremvosError, match="clip: id 16"):
        crf.main(["--root", root, "--input", "final", "--videos", "clip"])
