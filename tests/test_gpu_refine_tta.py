"""Test-time augmentation of the refinement net on the GPU (csrc/refine_ops.hip: premvos_refine_tta_input_f32,
premvos_refine_tta_output_f32; refinement/model.py: the member bodies of a plan; ``track --refine-tta``) against the restatement
(tests/refine_tta_restated.py, anchored on the oracle in tests/test_cpu_refine_tta.py).

Bounds.  The input kernel does the oracle's align-corners arithmetic operation for operation (no contraction): 1e-6, and bit equality
where the rule is a copy.  The output kernel alone: the bars of test_gpu_refinement.py::test_refine_output_matches_oracle (posterior and
conf 1e-5: expf against torch's softmax, a few ulp; masks may differ only where the restated mean probability is within 1e-4 of 0.5).  The net
end to end: the bars of test_gpu_refinement.py::test_refinement_net_end_to_end (logits 1e-3 relative to their largest value, posterior
1e-3, masks away from 2e-3 around 0.5, conf 1e-3), for the same reasons: fp32 convs in another summation order over ~70 layers.
Group / packed against per-frame calls: the bars of the existing group / packed tests (another batch size may pick another k-split)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import refine_tta_restated as T  # noqa: E402
from oracle import refinement_oracle as R  # noqa: E402


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _libops():
    from premvos_amd import _lib, ops
    return _lib, ops


def _nhwc(x_nchw, ps=None):
    """[N,C,h,w] host tensor -> ops.NHWC on the GPU (pixel stride 4 for two logits, as the net's own)."""
    _, ops = _libops()
    n, c, h, w = x_nchw.shape
    t = ops.NHWC.alloc(n, h, w, c, ps=ps)
    t.buf[..., :c] = x_nchw.permute(0, 2, 3, 1).to(_dev())
    return t


# ----------------------------------------------------------------------------------------------------------------- the input kernel
def test_input_kernel_resizes_and_mirrors():
    _lib, _ = _libops()
    lib, dev = _lib.load(), _dev()
    P, S = 2, 33
    x = torch.randn((P, 4, S, S), generator=torch.Generator().manual_seed(5))
    xin = x.permute(0, 2, 3, 1).contiguous().to(dev)
    for scale, So in ((0.75, 25), (1.0, 33), (1.25, 41)):
        assert R.scale_dimension(S, scale) == So
        out = torch.full((2 * P + 1, So, So, 4), 7.0, device=dev)                              # (one crop of sentinel behind the batch)
        _lib.check(lib.premvos_refine_tta_input_f32(xin.data_ptr(), P, S, out.data_ptr(), So, 1, _lib.current_stream()), "refine_tta_input")
        ref = R.resize_bilinear_tf(x, So, So, True)
        got = out.cpu().permute(0, 3, 1, 2)
        d0, d1 = float((got[:P] - ref).abs().max()), float((got[P:2 * P] - torch.flip(ref, [3])).abs().max())
        print(f"scale {scale}: {So}x{So}  max |d| unmirrored {d0:.2e}  mirrored {d1:.2e}")
        assert d0 <= 1e-6 and d1 <= 1e-6 and bool((got[2 * P] == 7.0).all())
        assert torch.equal(got[P:2 * P], torch.flip(got[:P], [3]))                            # the same arithmetic on both halves
        if So == S:
            assert torch.equal(got[:P], x)                                                     # scale 1: a copy plus a mirrored copy
        half = torch.full((2 * P, So, So, 4), 7.0, device=dev)
        _lib.check(lib.premvos_refine_tta_input_f32(xin.data_ptr(), P, S, half.data_ptr(), So, 0, _lib.current_stream()), "refine_tta_input")
        assert torch.equal(half[:P], out[:P]) and bool((half[P:] == 7.0).all())                # flip off: one half, nothing behind it


# ---------------------------------------------------------------------------------------------------------------- the output kernel
S_OUT, H_OUT, W_OUT, BOXES_OUT, COUNT_OUT = 33, 40, 56, 3, 2
CROPS_OUT = [(0, 30, 25, 56), (5, 8, 33, 40), (0, 0, 0, 0)]                                    # clipped at the frame's top / right border; interior


def _output_buffers():
    dev = _dev()
    _lib, _ = _libops()
    lib = _lib.load()
    ws = torch.zeros((int(lib.premvos_refine_output_workspace_bytes(BOXES_OUT, S_OUT, H_OUT, W_OUT)) + 3) // 4, device=dev)
    return {"crops": torch.tensor(CROPS_OUT, dtype=torch.int32, device=dev), "count": torch.tensor([COUNT_OUT], dtype=torch.int32, device=dev),
            "mask": torch.full((BOXES_OUT, H_OUT, W_OUT), 9, dtype=torch.uint8, device=dev), "post": torch.full((BOXES_OUT, H_OUT, W_OUT), 9.0, device=dev),
            "conf": torch.full((BOXES_OUT,), 9.0, device=dev), "ws": ws}


def _tta_output(members, b):
    _lib, _ = _libops()
    lib = _lib.load()
    mem = _lib.tta_members([(t.ptr, t.h, t.ps, mirrored) for t, mirrored in members])
    _lib.check(lib.premvos_refine_tta_output_f32(mem, b["crops"].data_ptr(), b["count"].data_ptr(), BOXES_OUT, S_OUT, H_OUT, W_OUT, b["mask"].data_ptr(),
                                                 b["post"].data_ptr(), b["conf"].data_ptr(), b["ws"].data_ptr(), _lib.current_stream()), "refine_tta_output")
    torch.cuda.synchronize()
    return b["mask"].cpu().numpy().copy(), b["post"].cpu().numpy().copy(), b["conf"].cpu().numpy().copy()


def _random_logits():
    g = torch.Generator().manual_seed(11)
    return [torch.randn((BOXES_OUT, 2, L, L), generator=g) * 2 for L in (9, 9, 11, 11)]


def test_output_kernel_merges_the_members():
    spec = "1,1.25+flip"
    table = T.member_table(spec, S_OUT)
    assert [(m[2], m[3]) for m in table] == [(9, False), (9, True), (11, False), (11, True)]
    lgs = _random_logits()
    members = [(_nhwc(lg), m[3]) for lg, m in zip(lgs, table)]
    b = _output_buffers()
    mask, post, conf = _tta_output(members, b)
    prob, cls = T.restated_merge(lgs, spec, S_OUT)
    near = ((prob - 0.5).abs() < 1e-4).to(torch.uint8)
    for i in range(COUNT_OUT):
        rm, rp = T.uncrop(prob[i], cls[i], CROPS_OUT[i], H_OUT, W_OUT)
        rn, _ = T.uncrop(prob[i], near[i], CROPS_OUT[i], H_OUT, W_OUT)                          # where a mask pixel's source sits at the boundary
        dp, dc = float(np.abs(post[i] - rp).max()), abs(float(conf[i]) - float(R.conf_score(rm, rp)))
        diff = mask[i] != rm
        print(f"box {i}: posterior max |d| {dp:.2e}  conf |d| {dc:.2e}  mask pixels that differ {int(diff.sum())}  foreground {int(rm.sum())}")
        assert dp <= 1e-5 and dc <= 1e-5 and not (diff & (rn == 0)).any()
        assert 0 < rm.sum() < rm.size                                                          # (non-vacuous)
    assert not mask[COUNT_OUT:].any() and not post[COUNT_OUT:].any() and not conf[COUNT_OUT:].any()      # the slot beyond ``count``
    again = _tta_output(members, b)                                                             # twice on the same buffers: the same bits
    for x, y in zip((mask, post, conf), again):
        assert x.tobytes() == y.tobytes()


def test_output_kernel_reads_the_mirror_flag():
    lgs = _random_logits()[:2]
    t = [_nhwc(lg) for lg in lgs]
    a = _tta_output([(t[0], False), (t[1], True)], _output_buffers())
    c = _tta_output([(t[0], True), (t[1], False)], _output_buffers())
    assert float(np.abs(a[1] - c[1]).max()) > 1e-2
    prob, cls = T.restated_merge(lgs, "1+flip", S_OUT)
    rm, rp = T.uncrop(prob[1], cls[1], CROPS_OUT[1], H_OUT, W_OUT)
    assert float(np.abs(a[1][1] - rp).max()) <= 1e-5


def test_one_unmirrored_member_is_the_plain_output_layer_bit_for_bit():
    _lib, _ = _libops()
    lib = _lib.load()
    lg = _nhwc(_random_logits()[0])
    got = _tta_output([(lg, False)], _output_buffers())
    b = _output_buffers()
    _lib.check(lib.premvos_refine_output_f32(lg.ptr, lg.ps, 9, 9, b["crops"].data_ptr(), b["count"].data_ptr(), BOXES_OUT, S_OUT, H_OUT, W_OUT,
                                             b["mask"].data_ptr(), b["post"].data_ptr(), b["conf"].data_ptr(), b["ws"].data_ptr(), _lib.current_stream()), "refine_output")
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(got[0]), b["mask"].cpu()) and torch.equal(torch.from_numpy(got[1]), b["post"].cpu())
    assert torch.equal(torch.from_numpy(got[2]), b["conf"].cpu()) and got[0][:COUNT_OUT].any()


# ------------------------------------------------------------------------------------------------------------------ the net, end to end
NM, SEED = 2, 1
IMG = (np.random.default_rng(1).random((120, 200, 3)) * 255).astype(np.uint8)
NET_BOXES = [[20.0, 30.0, 90.0, 150.0], [0.0, 0.0, 60.0, 80.0]]
NET_SPEC = "0.75,1+flip"
_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        _CACHE["w"] = R.synth_weights(SEED, NM)
    return _CACHE["w"]


def _restated():
    """Per box: (member logits, mask, posterior, conf) under NET_SPEC -- computed once, shared, left unchanged."""
    if "ref" not in _CACHE:
        out = []
        for b in NET_BOXES:
            x, crop = R.make_input(IMG, b)
            lgs = T.restated_member_logits(_weights(), x, NET_SPEC, NM)
            prob, cls = T.restated_merge(lgs, NET_SPEC, x.shape[2])
            mask, post = T.uncrop(prob[0], cls[0], crop, 120, 200)
            out.append((lgs, mask, post, R.conf_score(mask, post)))
        _CACHE["ref"] = out
    return _CACHE["ref"]


def _plain_net():
    from premvos_amd.refinement import RefinementNet
    if "plain" not in _CACHE:
        _CACHE["plain"] = RefinementNet(_weights(), NM)
    return _CACHE["plain"]


@pytest.mark.parametrize("use_graph", [False, True])
def test_net_end_to_end(use_graph):
    from premvos_amd.refinement import RefinementNet
    net = RefinementNet(_weights(), NM, use_graph=use_graph, tta=NET_SPEC)
    frame, boxes = torch.from_numpy(IMG).to(_dev()), torch.tensor(NET_BOXES).to(_dev())
    p = net.refine(frame, boxes, max_boxes=3, with_posterior=True)
    assert (p.graph is not None) == use_graph
    names = [n for n, _ in p.steps]
    assert names[0] == "refine_input" and names[-1] == "tta_output" and "refine_output" not in names
    assert [n for n in names if n.startswith(("tta_input", "tta_logits"))] == ["tta_input:289", "tta_logits:289", "tta_input:385"]
    assert [(m.n, m.h, m.w, m.c) for m in p.member_logits] == [(3, 97, 97, 2)] * 4
    assert names.count("conv:tta289/entry_flow/conv1_1") == 1 and names.count("conv:tta385/entry_flow/conv1_1") == 1 and len(set(names)) == len(names)
    d289 = [d for n, d in zip([n for n in names if n.startswith("conv:")], p.descs) if n == "conv:tta289/entry_flow/conv1_1"][0]
    assert (d289.n, d289.h, d289.w) == (6, 289, 289)                                            # the mirrored crops share the batch
    mem = [m.torch().cpu() for m in p.member_logits]
    for i, (lgs, rm, rp, rc) in enumerate(_restated()):
        for m, ref in enumerate(lgs):
            e = float((mem[m][i:i + 1] - ref).abs().max())
            print(f"box {i} member {m}: logits max |d| {e:.2e} (|ref| max {float(ref.abs().max()):.2f})")
            assert e < 1e-3 * max(1.0, float(ref.abs().max())), (i, m)
        gp, gm = p.posterior[i].cpu().numpy(), p.mask[i].cpu().numpy()
        diff = gm != rm
        print(f"box {i}: posterior max |d| {float(np.abs(gp - rp).max()):.2e}  conf |d| {abs(float(p.conf[i]) - float(rc)):.2e}  mask diff {int(diff.sum())}")
        assert np.abs(gp - rp).max() < 1e-3
        assert not diff.any() or np.abs(rp[diff] - 0.5).max() < 2e-3
        assert abs(float(p.conf[i]) - float(rc)) < 1e-3
    assert int(p.mask[len(NET_BOXES):].sum()) == 0 and not bool(p.posterior[len(NET_BOXES):].any())
    tta_post = p.posterior[:2].clone()
    q = _plain_net().refine(frame, boxes, max_boxes=3, with_posterior=True)
    assert float((q.posterior[:2] - tta_post).abs().max()) > 1e-2                               # not a pass-through of the plain net


def test_a_plain_net_is_untouched_by_a_tta_net_on_the_same_weights():
    from premvos_amd.refinement import RefinementNet
    plain = _plain_net()
    frame, boxes = torch.from_numpy(IMG).to(_dev()), torch.tensor(NET_BOXES).to(_dev())
    p = plain.refine(frame, boxes, max_boxes=3, with_posterior=True)
    before = [t.clone() for t in (p.mask, p.posterior, p.conf, p.logits.buf)]
    names = [n for n, _ in p.steps]
    assert not [n for n in names if "tta" in n] and names[0] == "refine_input" and names[-1] == "refine_output" and plain.tta is None
    assert all(len(k) == 7 for k in plain._plans)                                               # the plain plan key, as it always was
    other = RefinementNet(_weights(), NM, tta="1+flip")
    o = other.refine(frame, boxes, max_boxes=3, with_posterior=True)
    assert all(k[-1] == "1+flip" for k in other._plans) and float((o.posterior - before[1]).abs().max()) > 1e-3
    p = plain.refine(frame, boxes, max_boxes=3, with_posterior=True)
    for x, y in zip(before, (p.mask, p.posterior, p.conf, p.logits.buf)):
        assert torch.equal(x, y)
    assert RefinementNet(_weights(), NM, tta="1").tta is None                                   # "1" is off


def test_group_and_packed_equal_per_frame_calls():
    from premvos_amd.refinement import RefinementNet
    nm = 1
    net = RefinementNet(R.synth_weights(3, nm), nm, tta="1+flip")
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 100, 160, 3), dtype=np.uint8)).to(_dev())
    boxes = torch.zeros((2, 3, 4))
    counts = [3, 1]
    for g in range(2):
        for i in range(counts[g]):
            y0, x0 = rng.uniform(0, 50), rng.uniform(0, 90)
            boxes[g, i] = torch.tensor([y0, x0, y0 + rng.uniform(10, 45), x0 + rng.uniform(10, 65)])
    boxes = boxes.to(_dev())
    pg = net.refine_group(frames, boxes, torch.tensor(counts, dtype=torch.int32).to(_dev()), with_posterior=True)
    assert [n for n, _ in pg.steps][-1] == "tta_output" and pg.graph is not None
    mg, cg, qg = pg.mask_g.clone(), pg.conf_g.clone(), pg.posterior_g.clone()
    pk = net.refine_packed(frames, [boxes[g, :counts[g]] for g in range(2)], slots=4, max_frames=2)
    mk, ck = pk.mask_g[0].clone(), pk.conf_g[0].clone()
    off = 0
    for g in range(2):
        n = counts[g]
        p1 = net.refine(frames[g], boxes[g, :n], max_boxes=3, with_posterior=True)
        dq, dc, dk = float((qg[g, :n] - p1.posterior[:n]).abs().max()), float((cg[g, :n] - p1.conf[:n]).abs().max()), float((ck[off:off + n] - p1.conf[:n]).abs().max())
        print(f"frame {g}: group posterior {dq:.2e} conf {dc:.2e}; packed conf {dk:.2e}")
        assert dq < 1e-5 and dc < 1e-5 and dk < 1e-5
        for got in (mg[g], torch.cat([mk[off:off + n], torch.zeros_like(mg[g, n:])])):
            diff = got != p1.mask
            assert not bool(diff.any()) or (p1.posterior[diff] - 0.5).abs().max().item() < 1e-4
        assert int(mg[g, n:].sum()) == 0 and bool(p1.mask[:n].any())
        off += n


def test_the_bf16_modes_are_refused_with_a_spec():
    from premvos_amd.refinement import RefinementNet
    with pytest.raises(ValueError) as e:
        RefinementNet(_weights(), NM, precision="bf16x3", tta=NET_SPEC)
    assert "fp32 only" in str(e.value) and "bf16x3" in str(e.value) and "unvalidated" in str(e.value)
    assert RefinementNet(_weights(), NM, precision="bf16x3", tta="1").tta is None                 # plain inference is not a spec


# ------------------------------------------------------------------------------------------------------------------ the stage C driver
def test_the_stage_driver_honours_the_config_keys(tmp_path, monkeypatch, capsys):
    """``python -m premvos_amd.refinement.driver <config> <update>`` with "tta_scales" / "tta_flip" in the update string: one line naming
    the members, the JSON of an engine built with the same spec, in the update string's output directory."""
    from PIL import Image
    from premvos_amd.refinement import RefinementEngine, RefinementNet
    from premvos_amd.refinement import driver as rd
    nm = 1
    w = R.synth_weights(3, nm)
    monkeypatch.setattr(rd, "load_weights", lambda path: w)
    img = (np.random.default_rng(4).random((96, 144, 3)) * 255).astype(np.uint8)
    os.makedirs(tmp_path / "images" / "clip")
    os.makedirs(tmp_path / "bb" / "clip")
    Image.fromarray(img).save(str(tmp_path / "images" / "clip" / "00000.jpg"), quality=95)
    props = [{"bbox": [20.0, 10.0, 70.0, 60.0], "score": 0.9}, {"bbox": [60.0, 30.0, 50.0, 40.0], "score": 0.8}]
    (tmp_path / "bb" / "clip" / "00000.json").write_text(json.dumps(props))
    cfg = tmp_path / "run"
    cfg.write_text(json.dumps({"load": "unused", "image_input_dir": str(tmp_path / "images"), "bb_input_dir": str(tmp_path / "bb"),
                               "output_dir": str(tmp_path / "refined")}))
    update = json.dumps({"tta_scales": [1.0, 0.75], "tta_flip": True, "output_dir": str(tmp_path / "refined_tta")})
    assert rd.main([str(cfg), update]) == 0
    line = " ".join(capsys.readouterr().out.split())
    assert "test-time augmentation 1,0.75+flip" in line and "1@385 1m@385 0.75@289 0.75m@289" in line and "refined_tta" in line
    assert not os.path.exists(tmp_path / "refined")
    got = json.loads((tmp_path / "refined_tta" / "clip" / "00000.json").read_text())
    frame = np.asarray(Image.open(str(tmp_path / "images" / "clip" / "00000.jpg")).convert("RGB"))
    want = RefinementEngine(RefinementNet(w, nm, tta="1,0.75+flip")).refine_frame(frame, [dict(p) for p in props])
    plain = RefinementEngine(RefinementNet(w, nm)).refine_frame(frame, [dict(p) for p in props])
    assert [p["segmentation"] for p in got] == [p["segmentation"] for p in want] and [p["conf_score"] for p in got] == [p["conf_score"] for p in want]
    assert [p["conf_score"] for p in got] != [p["conf_score"] for p in plain]                   # (not the plain net's)


# ------------------------------------------------------------------------------------------------------------------------- the loop
def test_the_loop_runs_with_the_augmented_engine(tmp_path, monkeypatch, capsys):
    """``track --refine-tta 1+flip`` on a 3-frame tree (test_gpu_track_lockstep's ``_video``): output/final_tta/, never output/final/;
    the PNGs of ``do_video`` with an engine of the same spec, byte for byte; and a recorded run's candidate masks are ``net.refine``'s
    under the spec on the same boxes."""
    from test_gpu_plumbing import MIDDLE
    from test_gpu_track_lockstep import _engines, _video
    from premvos_amd import jpeg, track
    from premvos_amd.refinement import RefinementNet, tta
    from premvos_amd.refinement import driver as rd
    from premvos_amd.refinement.driver import RefinementEngine, _bucket
    from premvos_amd.reid import driver as qd
    root = str(tmp_path)
    lay = track._layout(root)
    _video(lay, "clip", 3, 2, seed=5)
    for netdir in ("refinement_net", "ReID_net"):
        os.makedirs(os.path.join(root, "code", netdir, "configs"))
        open(os.path.join(root, "code", netdir, "configs", "live"), "w").write("{}")
    _, reid_eng = _engines()
    made = []

    def init(config_path="refinement_net/configs/live", tta=None):
        made.append(tta)
        return RefinementEngine(RefinementNet(R.synth_weights(0, MIDDLE), MIDDLE, tta=tta))
    monkeypatch.setattr(rd, "refinement_net_init", init)
    monkeypatch.setattr(qd, "ReID_net_init", lambda: reid_eng)
    assert track.main(["--root", root, "--refine-tta", "1+flip"]) == 0
    text = capsys.readouterr().out
    assert made == [tta.parse("1+flip")] and "final_tta" in text and "1@385 1m@385" in " ".join(text.split())
    out = os.path.join(root, "output")
    assert sorted(os.listdir(os.path.join(out, "final_tta", "clip"))) == [f"{t:05d}.png" for t in range(3)]
    assert not os.path.exists(os.path.join(out, "final")) and sorted(d for d in os.listdir(out) if d != "intermediate") == ["final_tta"]
    eng = RefinementEngine(RefinementNet(R.synth_weights(0, MIDDLE), MIDDLE, tta="1+flip"))
    tracker = track.Tracker(eng, reid_eng, record=True)
    log = track.do_video(os.path.join(lay["images"], "clip") + "/", lay["images"], lay["anns"], lay["props"], lay["flows"],
                         os.path.join(root, "again") + "/", eng, reid_eng, record=True, tracker=tracker)
    assert len(log) == 3 and log[-1]["png"].any()
    for t in range(3):
        assert open(os.path.join(out, "final_tta", "clip", f"{t:05d}.png"), "rb").read() == open(os.path.join(root, "again", "clip", f"{t:05d}.png"), "rb").read(), t
    calls = [c for c in tracker.engine_log if c["call"] == "refine"]
    assert len(calls) == 2
    plain = RefinementNet(R.synth_weights(0, MIDDLE), MIDDLE)
    moved = 0
    for c in calls:
        frame = jpeg.to_device(track._frame_array(c["image_fn"]), eng.net.device)
        yx = torch.from_numpy(np.array([[b[1], b[0], b[1] + b[3], b[0] + b[2]] for b in c["bbox"]], np.float32)).to(eng.net.device)
        n = len(c["bbox"])
        p = eng.net.refine(frame, yx, max_boxes=_bucket(n))
        assert [s for s, _ in p.steps][-1] == "tta_output" and np.array_equal(p.mask[:n].cpu().numpy(), c["mask"])
        moved += int((plain.refine(frame, yx, max_boxes=_bucket(n)).mask[:n].cpu().numpy() != c["mask"]).sum())
    print(f"candidate mask pixels the augmentation changed against the plain net: {moved}")
    assert json.dumps(made[0].members())
