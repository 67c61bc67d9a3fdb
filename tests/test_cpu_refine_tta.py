"""The host side of the refinement net's test-time augmentation (no GPU): the spec parser and its refusals, the member table, the
restatement (tests/refine_tta_restated.py) anchored on plain inference and shown to move the posterior, header / binding / document
agreement of the two entries, their argument checks (before any HIP call), the places of ``track --refine-tta``'s outputs, its
refusals at argument time and the driver's config keys."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import refine_tta_restated as T
from oracle import refinement_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"premvos_refine_tta_input_f32": 7, "premvos_refine_tta_output_f32": 12}


# --------------------------------------------------------------------------------------------------------------------- the spec
def test_spec_parsing_round_trip_and_refusals():
    from premvos_amd.refinement import tta
    t = tta.parse("0.75,1,1.25+flip")
    assert t.scales == (0.75, 1.0, 1.25) and t.flip and str(t) == "0.75,1,1.25+flip" and tta.parse(str(t)) == t
    u = tta.parse(" 1.5, 0.5 ")
    assert u.scales == (1.5, 0.5) and not u.flip and str(u) == "1.5,0.5" and tta.parse(str(u)) == u           # the order given is kept
    assert tta.TTA([0.75, 1.0], True) == tta.parse("0.75,1.0+flip") and len({tta.parse("1+flip"), tta.parse("1.0+flip")}) == 1
    full = tta.parse("0.5,0.75,1,1.25,1.5,1.75+flip")
    assert len(full.members()) == 12 == tta.MAX_MEMBERS
    for bad, word in (("0.6", "'0.6'"), ("0.75,2", "'2'"), ("1,abc", "'abc'"), ("0.75,1,0.75", "'0.75'"), ("1,1.0", "'1.0'"),
                      ("0.5,0.75,1,1.25,1.5,1.75,0.5+flip", "14 members"), ("0.5,0.75,1,1.25,1.5,1.75,1,1.5,0.5,0.75,1.25,1.75,1", "13 members"),
                      ("", "empty"), ("   ", "empty"), ("1+flop", "'+flop'"), ("1,", "''"), ("+flip", "''")):
        with pytest.raises(ValueError) as e:
            tta.parse(bad)
        assert word in str(e.value), (bad, str(e.value))
    for bad in ([], [0.6], [1.0, 1.0], [0.5] * 13):
        with pytest.raises(ValueError):
            tta.TTA(bad)


def test_the_member_table():
    from premvos_amd.refinement import tta
    m = tta.parse("0.5,0.75,1,1.25,1.5,1.75").members()
    assert [x[1] for x in m] == [193, 289, 385, 481, 577, 673] and [x[2] for x in m] == [97, 97, 97, 121, 145, 169]
    assert not any(x[3] for x in m)
    m = tta.parse("1.25,0.75+flip").members()
    assert m == [(1.25, 481, 121, False), (1.25, 481, 121, True), (0.75, 289, 97, False), (0.75, 289, 97, True)]      # unmirrored before mirrored
    assert m == T.member_table("1.25,0.75+flip")                                                                     # the restatement's own table
    assert [x[1:3] for x in tta.parse("1,1.25").members(33)] == [(33, 9), (41, 11)] and tta.parse("0.75").members(33)[0][1:3] == (25, 9)
    assert tta.parse("0.75,1+flip").describe() == "0.75@289  0.75m@289  1@385  1m@385"


def test_scale_one_alone_is_off():
    from premvos_amd import track
    from premvos_amd.refinement import tta
    assert tta.parse("1").plain and tta.resolve("1") is None and tta.resolve("1.0") is None and tta.resolve(None) is None
    assert tta.resolve([1.0], False) is None and tta.resolve(tta.TTA([1.0])) is None
    assert tta.resolve("1+flip") == tta.TTA([1.0], True) and tta.resolve([0.75, 1.0], True) == tta.parse("0.75,1+flip")
    assert track.refine_tta(track.parse_args(["--refine-tta", "1"])) is None
    assert track.refine_tta(track.parse_args([])) is None and "refine_tta" not in vars(track.parse_args([]))
    assert str(track.refine_tta(track.parse_args(["--refine-tta", "0.75,1+flip"]))) == "0.75,1+flip"


def test_the_net_refuses_the_bf16_modes_before_it_needs_a_gpu():
    from premvos_amd.refinement import RefinementNet
    for prec in ("bf16", "bf16x3"):
        with pytest.raises(ValueError) as e:
            RefinementNet({}, 1, precision=prec, tta="1+flip")
        assert "fp32 only" in str(e.value) and "unvalidated" in str(e.value) and prec in str(e.value)


# ------------------------------------------------------------------------------------------------------------- the restatement
IMG = (np.random.default_rng(1).random((120, 200, 3)) * 255).astype(np.uint8)
BOX = [20, 30, 90, 150]
NM = 2


@pytest.fixture(scope="module")
def weights():
    return R.synth_weights(1, NM)


def test_the_restatements_anchor_is_plain_inference(weights):
    """The single member (1.0, unmirrored): ``restated_refine`` IS the oracle's output layer + conf_score, exactly."""
    x, crop = R.make_input(IMG, BOX)
    with torch.no_grad():
        lg = R.deeplab_logits(weights, x, NM)
    rm, rp = R.output_layer(lg, crop, 120, 200)
    mask, post, conf = T.restated_refine(weights, IMG, BOX, "1", NM)
    assert np.array_equal(mask, rm) and np.array_equal(post, rp) and conf == R.conf_score(rm, rp) and mask.any() and not mask.all()
    members = T.restated_members(x, "1")
    assert len(members) == 1 and members[0] is x
    got = T.restated_member_logits(weights, x, "1", NM)
    assert len(got) == 1 and torch.equal(got[0], lg)


def test_the_restated_merge_on_hand_written_logits():
    """Two members on a 1 x 1 grid (every resize is a broadcast): the mean of the probabilities, not of the logits; a tie is class 0;
    a mirrored member's logits are reversed along the width before the resize."""
    a = torch.tensor([0.0, 4.0]).view(1, 2, 1, 1)                 # p1 = 0.982
    b = torch.tensor([1.0, 0.0]).view(1, 2, 1, 1)                 # p1 = 0.269
    prob, cls = T.restated_merge([a, b], "1,1.25", 3)
    want = (torch.softmax(a[0, :, 0, 0], 0)[1] + torch.softmax(b[0, :, 0, 0], 0)[1]) / 2
    assert prob.shape == (1, 3, 3) and torch.allclose(prob, want.expand(1, 3, 3), atol=1e-7) and bool((cls == 1).all())
    assert abs(float(want) - 0.6255) < 1e-3 and float(torch.softmax((a + b)[0, :, 0, 0] / 2, 0)[1]) > 0.8          # (the logit mean would say 0.82)
    prob, cls = T.restated_merge([torch.zeros(1, 2, 1, 1), torch.zeros(1, 2, 1, 1)], "1+flip", 3)
    assert bool((prob == 0.5).all()) and not bool(cls.any())                                                       # a tie: class 0
    lg = torch.zeros(1, 2, 2, 2)
    lg[0, 1, :, 0] = 8.0                                           # foreground in the LEFT column
    plain, _ = T.restated_merge([lg], "1", 2)
    both, _ = T.restated_merge([lg, lg], "1+flip", 2)              # the second member's map is reversed: foreground right
    assert plain[0, 0, 0] > 0.99 and plain[0, 0, 1] == 0.5 and torch.allclose(both[0, :, 0], both[0, :, 1]) and abs(float(both[0, 0, 0]) - 0.75) < 1e-3


def test_the_augmentation_moves_the_posterior_and_is_decisive(weights):
    """synth_weights(1, 2), frame 120x200, box [20, 30, 90, 150], spec 0.75,1,1.25+flip: the merged posterior is not the plain one (a
    pass-through would be caught), and few crop pixels sit at the decision boundary (masks are compared away from it)."""
    spec = "0.75,1,1.25+flip"
    x, crop = R.make_input(IMG, BOX)
    members = T.restated_members(x, spec)
    assert [tuple(m.shape) for m in members] == [(1, 4, s, s) for s in (289, 289, 385, 385, 481, 481)]
    assert members[2] is x and torch.equal(members[3], torch.flip(x, [3])) and torch.equal(members[1], torch.flip(members[0], [3]))
    lgs = T.restated_member_logits(weights, x, spec, NM)
    assert [tuple(l.shape) for l in lgs] == [(1, 2, L, L) for L in (97, 97, 97, 97, 121, 121)]
    prob, cls = T.restated_merge(lgs, spec, 385)
    plain, pcls = T.restated_merge(lgs[2:3], "1", 385)
    per = [T.restated_merge([torch.flip(l, [3]) if m[3] else l], "1", 385)[0] for l, m in zip(lgs, T.member_table(spec))]   # each member's own p1
    spread = max(float((p - plain).abs().max()) for p in per)
    near = int(((prob - 0.5).abs() < 1e-3).sum())
    print(f"merged vs plain posterior: max |d| {float((prob - plain).abs().max()):.3f}; members vs plain: up to {spread:.3f}; "
          f"crop pixels within 1e-3 of 0.5: {near} of {prob.numel()}; class changes: {int((cls != pcls).sum())}")
    assert float((prob - plain).abs().max()) > 1e-2
    assert near <= 0.01 * prob.numel()
    mask, post, conf = T.restated_refine(weights, IMG, BOX, spec, NM)
    m0, p0, c0 = T.restated_refine(weights, IMG, BOX, "1", NM)
    assert float(np.abs(post - p0).max()) > 1e-2 and mask.shape == (120, 200) and np.isfinite(conf)


# ----------------------------------------------------------------------------------------------------- header, binding, documents
def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    src = open(os.path.join(ROOT, "premvos_amd", "csrc", "refine_ops.hip")).read()
    assert _lib.ABI_VERSION == 21
    for name, nargs in ENTRIES.items():
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert decl.count(",") + 1 == nargs and f'extern "C" int {name}(' in src
    for line in ("model.py:84-160", "model.py:272-277", "model.py:118", "model.py:137", "model.py:143-147", "model.py:258-297"):
        assert line in hdr, line
    # the descriptor: the header's struct and the ctypes mirror, field by field
    body = re.search(r"typedef struct premvos_tta_members \{(.*?)\} premvos_tta_members;", hdr, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[PREMVOS_TTA_MAX_MEMBERS\])?;", body)
    assert fields == [f[0] for f in _lib.TTAMembers._fields_] == ["count", "size", "pixel_stride", "mirrored", "logits"]
    assert int(re.search(r"#define PREMVOS_TTA_MAX_MEMBERS (\d+)", hdr).group(1)) == _lib.TTA_MAX_MEMBERS == 12
    assert C.sizeof(_lib.TTAMembers) == 4 * (1 + 3 * 12) + 4 + 8 * 12                                  # (the pointers are 8-byte aligned)
    assert _lib.SIGNATURES["premvos_refine_tta_output_f32"][0] is _lib.TTAMembers                      # by value
    for bounds in re.findall(r"__launch_bounds__\((\w+)\)", src):
        assert int(bounds) % 64 == 0
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(name in text for name in ENTRIES), doc
    assert "--refine-tta" in open(os.path.join(ROOT, "README.md")).read() and "tta_scales" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8.10" in design and "--refine-tta" in design and "unmeasured" in design


def test_library_built_for_gfx950_refuses_bad_arguments_without_a_gpu():
    import __graft_entry__ as G
    from premvos_amd import _lib
    G.build()
    lib = _lib.load()
    assert lib.premvos_abi_version() == 21 and all(hasattr(lib, n) for n in ENTRIES)
    buf = np.zeros(4096, np.uint8)
    one = buf.ctypes.data + (-buf.ctypes.data) % 16                                             # never dereferenced: every call is refused

    def refused(rc, *words):
        err = lib.premvos_last_error()
        assert rc == -1 and all(w in err for w in words), (rc, err)

    def tin(net_in=one, boxes=2, size=33, out=one + 1024, out_size=25, flip=1):
        return lib.premvos_refine_tta_input_f32(net_in, boxes, size, out, out_size, flip, None)

    refused(tin(net_in=None), b"refine_tta_input", b"null")
    refused(tin(out=None), b"null")
    refused(tin(boxes=0), b"bad dims")
    refused(tin(size=1), b"bad dims")
    refused(tin(out_size=0), b"bad dims")
    refused(tin(out_size=-5), b"bad dims")
    refused(tin(flip=2), b"flip is 0 or 1")
    refused(tin(flip=-1), b"flip is 0 or 1")
    refused(tin(out=one + 1028), b"16-byte aligned")
    refused(tin(net_in=one + 8), b"16-byte aligned")

    def members(n=2, size=9, ps=4, mirrored=(0, 1), ptr=one):
        return _lib.tta_members([(ptr, size, ps, mirrored[m % 2]) for m in range(n)])

    def tout(mem=None, crops=one, count=one + 64, max_boxes=3, size=33, h=40, w=56, mask=one + 128, post=None, conf=one + 256, ws=one + 512):
        return lib.premvos_refine_tta_output_f32(members() if mem is None else mem, crops, count, max_boxes, size, h, w, mask, post, conf, ws, None)

    zero, many = members(), members()
    zero.count, many.count = 0, 13
    refused(tout(mem=zero), b"refine_tta_output", b"1 to 12 members, not 0")
    refused(tout(mem=many), b"1 to 12 members, not 13")
    neg = members()
    neg.count = -1
    refused(tout(mem=neg), b"1 to 12 members")
    refused(tout(mem=members(ptr=None)), b"null pointer (logits of member 0)")
    hole = members(3)
    hole.logits[2] = None
    refused(tout(mem=hole), b"logits of member 2")
    refused(tout(mem=members(size=0)), b"member 0 has a grid of 0")
    refused(tout(mem=members(size=-3)), b"grid of -3")
    refused(tout(mem=members(ps=1)), b"pixel stride of 1")
    refused(tout(mem=members(mirrored=(0, 2))), b"member 1: mirrored is 0 or 1")
    for k in ("crops", "count", "mask", "conf", "ws"):
        refused(tout(**{k: None}), b"null pointer")
    for k in ("max_boxes", "h", "w"):
        refused(tout(**{k: 0}), b"bad dims")
    refused(tout(size=1), b"bad dims")
    refused(tout(ws=one + 516), b"workspace must be 16-byte aligned")
    refused(tout(mem=members(1, mirrored=(0, 0)), ws=one + 516), b"16-byte aligned")            # the single plain member too: before it dispatches
    d = _lib.tta_members([(one + 16 * m, 9 + m, 4, m % 2) for m in range(12)])                   # the mirror carries twelve members
    assert d.count == 12 and [d.size[m] for m in range(12)] == list(range(9, 21)) and d.logits[11] == one + 176 and d.mirrored[11] == 1


# --------------------------------------------------------------------------------------------------------------------- the places
def test_the_mode_never_writes_the_live_loops_places():
    from premvos_amd import track
    assert track.mode_suffix() == "" and track.mode_suffix("argmax", False, False, False) == "" and track.mode_suffix(tta=False) == ""
    assert track.mode_suffix("argmax", False, False, False, True) == "tta" and track.mode_suffix(tta=True) == "tta"
    assert track.mode_suffix(live_weights=True, tta=True) == "weights_tta" and track.mode_suffix("probabilistic", tta=True) == "prob_tta"
    assert track.mode_suffix("probabilistic", True, tta=True) == "oracle_prob_tta" and track.mode_suffix(ensemble=True, tta=True) == "ensemble_tta"
    plain = track.mode_layout("/r")
    assert plain == track.mode_layout("/r", "argmax", False, False, False, False) and plain["out"] == "/r/output/final/"
    lay = track.mode_layout("/r", "argmax", False, False, False, True)
    assert lay == track.mode_layout("/r", tta=True)
    assert lay["out"] == "/r/output/final_tta/" and lay["eval"] == "/r/output/eval_tta" and lay["overlay"] == "/r/output/overlay_tta/"
    assert lay["viz"] == "/r/output/viz_tta/" and lay["summary"] == "/r/output/premvos_amd_davis_eval_tta.json"
    assert track.mode_layout("/r", live_weights=True, tta=True)["out"] == "/r/output/final_weights_tta/"
    assert track.mode_layout("/r", "probabilistic", tta=True)["out"] == "/r/output/final_prob_tta/"
    for k in ("images", "anns", "props", "flows"):
        assert lay[k] == plain[k]
    for kw in ({}, {"live_weights": True}, {"combine": "probabilistic"}, {"oracle": True}, {"ensemble": True}):
        out = track.mode_layout("/r", tta=True, **kw)
        assert all(not out[k].rstrip("/").endswith(("/final", "/eval", "/overlay", "/viz")) for k in ("out", "eval", "overlay", "viz")), out


def _refused(capsys, parse, argv, *words):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    err = " ".join(capsys.readouterr().err.split())
    assert e.value.code == 2 and all(w in err for w in words), (argv, err)


def test_the_track_commands_refusals(capsys):
    from premvos_amd import track
    p = track.parse_args
    _refused(capsys, p, ["--refine-tta", "1+flip", "--prewarp"], "argument --refine-tta: not with --prewarp", "no refinement net")
    _refused(capsys, p, ["--refine-tta", "1+flip", "--prewarp-search", "3"], "argument --refine-tta: not with --prewarp")
    _refused(capsys, p, ["--refine-tta", "1+flip", "--max-reid-distance"], "argument --refine-tta: not with --max-reid-distance")
    _refused(capsys, p, ["--refine-tta", "1", "--prewarp"], "argument --refine-tta: not with --prewarp")                  # the flag, whatever it says
    for bad, word in (("0.6", "'0.6'"), ("1,1", "'1'"), ("", "empty"), ("1+flop", "'+flop'"), ("0.5,0.75,1,1.25,1.5,1.75,1+flip", "14 members")):
        _refused(capsys, p, ["--refine-tta", bad], "argument --refine-tta: invalid value", word)
    _refused(capsys, p, ["--refine-tta"], "expected one argument")
    # accepted next to every flag of the live loop; no file was looked at
    for extra in ([], ["--eval", "--overlay"], ["--lockstep", "3"], ["--search", "4"], ["--live-weights", "1,1,1,1,1"], ["--ensemble", "1,1,1,1,1;1,0,0,0,0"],
                  ["--combine", "probabilistic", "--oracle", "--viz"]):
        a = p(["--refine-tta", "0.75,1,1.25+flip"] + extra)
        assert str(track.refine_tta(a)) == "0.75,1,1.25+flip" and a.refine_tta == "0.75,1,1.25+flip"
    assert track.main(["--root", "/nonexistent", "--refine-tta", "1+flip", "--check-only"]) == 2      # accepted; the inputs are what is missing
    capsys.readouterr()
    with pytest.raises(SystemExit):
        p(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--refine-tta SPEC", "model.py:84-160", "output/final_tta/", "never output/final/", "0.75,1,1.25+flip"):
        assert word in text, word


# ----------------------------------------------------------------------------------------------------------------- the config
def test_the_config_keys(tmp_path):
    from premvos_amd.refinement import driver, tta
    cfg = tmp_path / "run"
    cfg.write_text('{\n# a comment\n"load": "x", "output_dir": "out"}')
    assert driver.config_tta(driver.Config(str(cfg))) is None
    update = json.dumps({"tta_scales": [0.75, 1.0, 1.25], "tta_flip": True, "output_dir": "refined_proposals_tta/"})
    c = driver.Config(str(cfg), update)
    assert driver.config_tta(c) == tta.parse("0.75,1,1.25+flip") and c.dir("output_dir") == "refined_proposals_tta/"
    assert driver.config_tta(driver.Config(str(cfg), '{"tta_scales": [1.0]}')) is None                                # plain
    assert driver.config_tta(driver.Config(str(cfg), '{"tta_scales": [1.0], "tta_flip": false}')) is None
    assert driver.config_tta(driver.Config(str(cfg), '{"tta_flip": true}')) == tta.parse("1+flip")
    assert driver.config_tta(driver.Config(str(cfg), '{"tta_scales": [1.25, 0.75]}')) == tta.parse("1.25,0.75")
    with pytest.raises(ValueError):
        driver.config_tta(driver.Config(str(cfg), '{"tta_scales": [0.6]}'))
    with pytest.raises(AssertionError):
        driver.config_tta(driver.Config(str(cfg), '{"tta_scales": "0.75,1"}'))                                         # a float list, as Config's getters insist
    with pytest.raises(TypeError):
        driver.config_tta(driver.Config(str(cfg), '{"tta_scales": [0.75], "tta_flip": 1}'))
    import inspect
    sig = inspect.signature(driver.refinement_net_init)
    assert list(sig.parameters) == ["config_path", "tta"] and sig.parameters["tta"].default is None
