"""Without a GPU: the case table of the depthwise kernel tests (tests/dwconv_cases.py) reaches every kernel instance that
premvos_dwconv3x3_f32's dispatcher can pick.  The dispatcher's decision is read through the host-only premvos_dwconv3x3_variant, which
the launcher itself consults, so a new branch of the rule without a case in the table fails here."""
import json
import os

import pytest

import dwconv_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from premvos_amd import _lib
    return _lib.load()


def _covered():
    out = set()
    for c in D.CASES:
        out |= D.launched_codes(c)
    return out


def test_table_is_well_formed_and_the_query_agrees_with_it(lib):
    assert len(D.BY_ID) == len(D.CASES)
    for c in D.CASES:
        ho, wo = D.out_extent(c)
        assert ho >= 1 and wo >= 1 and c.act & ~(D.S8 | D.RELU) == 0, c.id
        for win in (c.win_in, c.win_out):
            assert win is None or (win[0] % 4 == 0 and win[1] % 4 == 0 and win[1] + D.c_pad(c) <= win[0] and win[0] > D.c_pad(c)), c.id
        for act in {c.act, c.act & ~D.S8}:
            got = D.query(lib, c, act)
            assert got == D.expected_code(c, act), (c.id, D.describe(got), D.describe(D.expected_code(c, act)))
    # the table holds what the issue of this test names: a window on both sides, a c that is not a multiple of 4, 1-pixel maps, ...
    assert any(c.c % 4 for c in D.CASES) and any(c.h == 1 and c.w == 1 for c in D.CASES)
    assert any(c.win_in and c.win_out for c in D.CASES) and any(c.pt == 0 and c.ho is not None for c in D.CASES)
    assert any(c.h % c.rate and c.w % c.rate and c.rate > 1 for c in D.CASES)


def test_query_validates_like_the_launcher(lib):
    ok = (2, 25, 25, 64, 25, 25, 1, 1, 0, 0)
    assert lib.premvos_dwconv3x3_variant(*ok) == D.code(D.TILE, 5, 5, 1, 0, 1, D.F32)
    for pos, bad in ((0, 0), (1, 0), (2, -1), (3, 0), (3, 62), (4, 0), (5, 0), (6, 0), (7, 0), (9, 2), (9, 0x100), (9, 0x400)):
        args = list(ok)
        args[pos] = bad
        assert lib.premvos_dwconv3x3_variant(*args) == -1, (pos, bad)
        assert b"dwconv3x3" in lib.premvos_last_error()


def test_every_reachable_variant_has_a_case(lib):
    """A sweep of the query over extents 1..60 plus the wide production maps, every dilation the nets use and the ones between them,
    strides 1-3, small and large batches, even and odd numbers of 4-channel units, both pre-ReLU values, plain and S8 store."""
    covered = _covered()
    extents = list(range(1, 61)) + [97, 193, 385]
    q = lib.premvos_dwconv3x3_variant
    full = {}
    for n, cp in ((1, 4), (16, 64), (7, 60), (320, 2044), (96, 2048)):                 # c_pad / 4 = 1, 16, 15, 511, 512
        for dil in (1, 2, 3, 4, 5, 6, 12, 18):
            for stride in (1, 2, 3):
                for pre, act in ((0, 0), (1, D.RELU), (0, D.S8 | D.RELU), (1, D.S8)):
                    for ho in extents:
                        for wo in extents:
                            v = q(n, ho, wo, cp, ho, wo, stride, dil, pre, act)
                            if v not in full:
                                full[v] = (n, cp, ho, wo, stride, dil, pre, act)
    assert -1 not in full
    missing = {D.describe(v): at for v, at in full.items() if v not in covered}
    assert not missing, f"dispatcher variants without a case in tests/dwconv_cases.py: {missing}"
    assert len(full) >= 42            # 4 tile instances + 2 row + 1 per-pixel, x PRE_RELU x 3 store forms


def _production_layers():
    from premvos_amd.refinement.model import module_plan
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "deeplab_host_refs.json")))
    relu_inside = {prefix: relu_in for prefix, _, _, _, relu_in, _, _ in module_plan(ref["num_middle"])}
    layers = []

    def walk(o):
        if isinstance(o, dict):
            if o.get("op") == "depthwise":
                layers.append(o)
            for v in o.values():
                walk(v)
        elif isinstance(o, list):
            for v in o:
                walk(v)
    walk(ref)
    out = []
    for l in layers:
        scope = l["scope"]
        if scope.startswith("xception_65/"):        # _Plan._build: pre_relu = not relu_inside, act = RELU if relu_inside
            prefix = scope[len("xception_65/"):].rsplit("/", 1)[0]
            pre, act = (0, D.RELU) if relu_inside[prefix] else (1, 0)
        else:                                       # ASPP and decoder: dwconv(..., act=ACT_RELU)
            assert scope.startswith("aspp") or scope.startswith("decoder/"), scope
            pre, act = 0, D.RELU
        out.append((scope, l["cin"], l["in_hw"], l["out_hw"], l["stride"], l["rate"], pre, act))
    return out


def test_every_production_layer_variant_has_a_case(lib):
    covered = _covered()
    layers = _production_layers()
    assert len(layers) >= 26
    assert {(c, tuple(hw), s, r) for _, c, _, hw, s, r, _, _ in layers} >= {(64, (193, 193), 1, 1), (728, (25, 25), 1, 1), (2048, (25, 25), 1, 18),
                                                                         (128, (97, 97), 2, 1), (304, (97, 97), 1, 1)}
    missing = {}
    for scope, c, in_hw, (ho, wo), stride, rate, pre, act in layers:
        # the map the launcher is handed: the golden in_hw, except that a strided layer's in_hw counts the ring of zeros that
        # fixed_padding puts around it (one pixel on each side of a 3x3 kernel), which the launcher takes as pt = pl = 1
        h, w = (in_hw[0], in_hw[1]) if stride == 1 else (in_hw[0] - 2, in_hw[1] - 2)
        assert (h, w) == ((ho - 1) * stride + 1, (wo - 1) * stride + 1), (scope, in_hw, ho, wo, stride)
        for n in (1, 4, 20, 96, 320):
            for store in (0, D.S8):
                v = lib.premvos_dwconv3x3_variant(n, h, w, (c + 3) // 4 * 4, ho, wo, stride, rate, pre, act | store)
                assert v >= 0, lib.premvos_last_error()
                if v not in covered:
                    missing[D.describe(v)] = (scope, n)
    assert not missing, missing


def test_every_threshold_of_the_rule_has_a_case_on_each_side(lib):
    assert len(D.THRESHOLDS) == 6
    for what, a, b in D.THRESHOLDS:
        ca, cb = D.BY_ID[a], D.BY_ID[b]
        va, vb = D.query(lib, ca), D.query(lib, cb)
        assert va == D.expected_code(ca) and vb == D.expected_code(cb), what
        assert va != vb, f"{what}: {a} and {b} both launch {D.describe(va)}"
    # the two sides differ in nothing but the quantity the threshold is about
    t = D.BY_ID
    assert t["t48-9x9x2048-n86"]._replace(id="", n=85, launches=None) == t["t44-9x9x2048-n85"]._replace(id="", launches=None)
    assert t["t44-13x14x8-r4"]._replace(id="", rate=5, pt=5, pl=5, launches=None) == t["t44n-13x14x8-r5"]._replace(id="", launches=None)
    assert t["t44n-13x13x8-r6"]._replace(id="", h=12, launches=None) == t["pix-12x13x8-r6"]._replace(id="", launches=None)
    assert t["t44-8x8x8"]._replace(id="", h=7, launches=None) == t["row1-7x8x8"]._replace(id="", launches=None)
    assert t["row1-7x8x8"]._replace(id="", w=7, launches=None) == t["pix-7x7x8"]._replace(id="", launches=None)
    assert t["t55-50x50x8"]._replace(id="", h=55, w=55, launches=None) == t["t44-55x55x8"]._replace(id="", launches=None)
