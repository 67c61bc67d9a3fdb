"""Without a GPU: the premises of tests/test_gpu_conv_f32_special.py.  The lattice inputs of tests/conv_f32_special_cases.py make every
product a multiple of 2^-8 and every case keeps S_abs below 2^16 -- so a float32 evaluation of the sums in any order is exact, which is
why the GPU test may ask for equality --, the table reaches every instance of the streaming pointwise kernel and of the direct small-N
kernel and, by its shapes alone, every mechanism its comments name, and the tuner offers the two kernels to no kind of layer that the
table does not hold."""
import itertools

import pytest
import torch

import conv_f32_special_cases as T
from conv_exact_device import shape_desc

IDS = [c.id for c in T.CASES]


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_lattice_inputs_make_every_sum_exact(case):
    data, fin = T.inputs(case), T.finite_inputs(case)
    for t in (fin.x, data.w):
        t = t[t != 0] if case.inf else t                                            # (the zeros stand in for the +Inf pixels)
        q = t * 16
        assert torch.equal(q, q.round()) and t.abs().min().item() >= 1 - 3 / 16 and t.abs().max().item() <= case.hmax + 3 / 16
        assert t.numel() < 1000 or t.abs().max().item() == case.hmax + 3 / 16
        assert set(((t.abs() + 0.25).floor()).unique().tolist()) == set(range(1, case.hmax + 1))          # every |h| occurs
        assert not case.inf or t.min().item() > 0
    for t in (data.b, data.res):
        assert t is None or (t.abs().max().item() <= 8 and torch.equal(t / T.QUANTUM, (t / T.QUANTUM).round()))
    assert (data.res is not None) == case.res and (case.bias or not data.b.any())
    ref, s_abs = T.expected(case)
    assert ref.shape == (case.n, case.cout) + T.gemm_extent(case) == s_abs.shape
    print(f"{case.id}: max S_abs = {s_abs.max().item():.1f}")
    assert s_abs.max().item() < T.S_ABS_LIMIT == 2.0 ** 24 * T.QUANTUM              # the exactness condition
    pre64 = T.B.pre_activation(case, fin)
    pre32 = T.B.pre_activation(case, fin, torch.float32)
    assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)      # a float32 evaluation rounds nowhere
    assert torch.equal(pre64.float().double(), pre64)
    assert torch.equal(pre64 / T.QUANTUM, (pre64 / T.QUANTUM).round()) and pre64.abs().max().item() <= s_abs.max().item()
    if not case.inf:
        assert torch.equal(ref.float().double(), ref) and torch.equal(T.activate(case, pre32).double(), ref)
        # the data tells a dropped or doubled product from the right sum: no product is zero, and most outputs are not
        assert (ref != 0).float().mean().item() > (0.4 if case.act == "relu" else 0.9)
        return
    # +Inf in every channel of the four corner pixels and nowhere else; the reference is +Inf exactly where a window covers a corner
    # and, everywhere else, the finite sum that does not read the corners at all
    assert case.act == "none" and not case.res and case.cin == T.cin_pad(case)      # (no pad channel: +Inf would meet a zero weight)
    inf = torch.isinf(data.x)
    assert inf[:, :, ::case.h - 1, ::case.w - 1].all() and inf.sum().item() == 4 * case.n * case.cin and (data.x > 0).all()
    corners = T.corner_outputs(case)
    assert corners.sum().item() == 16
    assert not torch.isnan(ref).any() and torch.equal(torch.isinf(ref), corners.expand_as(ref)) and (ref > 0).all()
    assert torch.equal(ref[..., ~corners], pre64[..., ~corners])


def test_table_reaches_every_instance_and_every_mechanism():
    assert len(T.BY_ID) == len(T.CASES) and all(i in T.BY_ID for i in T.GAUSSIAN)
    inst = T.instances()
    assert len(T.STREAM_INSTANCES) == 12 and set(inst) == set(T.STREAM_INSTANCES) | set(T.SMALLN_KERNELS) and all(inst.values())
    for c in T.CASES:
        assert c.act in T.ACTS and all(T.gemm_extent(c)) and not c.deconv and T.k_pad(c) - T.k_real(c) < 16
        if c.win_in:
            assert c.win_in[0] % 4 == 0 and c.win_in[1] % 4 == 0 and c.win_in[1] + T.cin_pad(c) <= c.win_in[0]
        if c.win_out:
            assert c.win_out[1] + c.cout <= c.win_out[0] and c.win_out[0] > c.cout
        if c.win_res:
            assert c.res and c.win_res[1] + c.cout <= c.win_res[0]

    # --- the streaming kernel ---
    st = T.STREAM_CASES
    assert all(c.kernel == "stream" and c.hints == ((5, 0),) for c in st)
    assert {T.stream_instance(c) for c in st} == set(T.STREAM_INSTANCES)
    gauss = {T.stream_instance(T.BY_ID[i]) for i in T.GAUSSIAN if T.BY_ID[i].kernel == "stream"}
    assert gauss == set(T.STREAM_UNTESTED_BEFORE)                  # the Gaussian tests run the six instances no test ran before
    assert {c.cout for c in st} == {128, 256, 384, 512}
    rows = {T.gemm_rows(c) for c in st}
    assert {35, 256, 257} <= rows
    walk = {c.id: T.stream_walk(c) for c in st}
    assert walk["k64-relu-res-walk"] == (64, 67) and walk["k128-none-res-walk"] == (80, 83)
    assert walk["k64-relu"] == (8, 2) and walk["k64-none"] == (8, 1)
    multi = {i for i, (wgs, steps) in walk.items() if steps > wgs}
    assert multi == {"k64-relu-res-walk", "k128-none-res-walk"}
    assert {T.BY_ID[i].cout for i in multi} == {384, 512} and {T.k_pad(T.BY_ID[i]) for i in multi} == {64, 128}
    assert all(steps < 8 for i, (wgs, steps) in walk.items() if i not in multi)
    assert {s for i, (w, s) in walk.items() if i not in multi} >= {1, 2}
    # walkers x column tiles is a multiple of 8 * column tiles (the kernel's (XCD, column tile, walker) mapping is a bijection) and fits 256 CUs
    for c in st:
        wgs, steps = T.stream_walk(c)
        assert wgs % 8 == 0 and wgs * (c.cout // 128) <= 256
    # windows: input (in_ps 72 and 136, offset 4), output (cout + 8, offset 4), residual with a pixel stride of its own; pad channels; no bias
    assert {c.win_in for c in st if c.win_in} == {(72, 4), (136, 4)}
    assert {(c.cin, T.cin_pad(c)) for c in st if c.cin < T.cin_pad(c)} == {(62, 64), (126, 128)}
    assert all(c.win_in for c in st if c.cin < T.cin_pad(c))
    assert any(c.win_out == (c.cout + 8, 4) for c in st)
    assert any(c.win_res and c.win_res[0] != (c.win_out or (c.cout, 0))[0] for c in st)
    assert [c.id for c in st if not c.bias] == ["k128-none-nobias"]

    # --- the direct small-N kernel ---
    sn = T.SMALLN_CASES
    assert all(c.kernel == "smalln" and T.smalln_applicable(c) and c.hints[0] == (1, 0) for c in sn)
    kern = {c.id: [k for _, _, k in T.launches_of(c)] for c in sn}
    pp1, pp2, tile = T.SMALLN_KERNELS
    tiled = [c for c in sn if kern[c.id][0] == tile]
    assert [c.id for c in tiled] == ["tile-37x43-n3", "tile-40x40", "tile-c568", "tile-900", "tile-inf-corners"]
    for c in tiled:                                                # every tiled case also runs the per-pixel form on the same layer
        assert (1, 1) in c.hints and T.smalln_kernel(c, 1) == pp2 and T.tiles(c) >= T.TILED_MIN_TILES
    for c in sn:
        if c not in tiled:
            assert set(kern[c.id]) == {T.SMALLN_KERNELS[c.cout - 1]}
    per_pixel = {nout: [c for c in sn if c not in tiled and c.cout == nout] for nout in (1, 2)}
    for nout, cs in per_pixel.items():
        assert any(c.k == 1 and T.k_real(c) == 32 for c in cs), nout                                 # the applicability floor
        assert any(c.k == 3 and T.cin_pad(c) == 4 and T.idle_lanes(c) == 15 for c in cs), nout       # only lane 0 has channels
        assert any(T.cin_pad(c) == 68 for c in cs) and any(T.cin_pad(c) == 260 and T.c_trips(c) == 2 for c in cs), nout
        assert any(c.k == 7 and c.stride == 2 and c.pad == (2, 2, 3, 3) and c.cin == 3 for c in cs), nout
        assert any(c.dil == 2 and c.n == 3 and c.pad == (2, 2, 2, 2) and (T.gemm_rows(c) // c.n) % 16 for c in cs), nout
        assert any(T.gemm_rows(c) == 3 and c.win_out == (5, 3) and c.res for c in cs), nout
        assert {c.act for c in cs} == set(T.ACTS), nout
        assert any(h == (0, 0) for c in cs for h in c.hints), nout                                   # hint 0 (auto) takes the kernel too
    assert any(T.k_real(c) == 32 for c in sn) and not any(T.k_real(c) < 32 for c in sn)
    # dilated taps fall outside the map on all four sides: first / last output row and column
    a = T.BY_ID["pp2-atrous"]
    assert T.gemm_extent(a) == (a.h, a.w) and a.pad[0] == a.dil and a.h > 2 * a.dil and a.w > 2 * a.dil
    # the grid-stride loops: a second trip per pixel and per tile; every other case fits one trip
    assert T.gemm_rows(T.BY_ID["pp1-pw-c32-230"]) == 52900 > 49152 and T.grid_trips(T.BY_ID["pp1-pw-c32-230"]) == 2
    big = T.BY_ID["tile-900"]
    assert T.tiles(big) == 50625 > 49152 and T.grid_trips(big, 0) == 2 and T.grid_trips(big, 1) == 17
    assert all(T.grid_trips(c, stg) == 1 for c in sn for _, stg, _ in T.launches_of(c) if c.id not in ("pp1-pw-c32-230", "tile-900"))
    # LDS: the attribute branch (> 48 KB) once; the largest head any earlier test ran (661 channels) stays under it
    assert {c.id: T.lds_bytes(c) for c in sn if T.lds_bytes(c) > T.LDS_ATTR} == {"pp2-c700-lds": 50432}
    assert 2 * T.B._r(9 * 664, 16) * 4 < T.LDS_ATTR
    # tile counts on either side of the threshold; a ragged last tile in both directions; one output on a map of >= 100 tiles
    assert T.tiles(T.BY_ID["tile-40x40"]) == 100 and T.tiles(T.BY_ID["pp2-same-36x44"]) == 99 and kern["pp2-same-36x44"] == [pp2, pp2]
    r = T.BY_ID["tile-37x43-n3"]
    assert r.h % 4 and r.w % 4 and r.n == 3 and T.tiles(r) == 110
    one = T.BY_ID["pp1-same-40x40"]
    assert one.cout == 1 and T.tiles(one) >= 100 and kern[one.id] == [pp1, pp1]
    # channel steps of the tiled form: fewer channels than one step (idle lanes), a second step, nine steps; with and without residual
    assert {T.c_trips(c) for c in tiled} >= {1, 2, 9} and {T.idle_lanes(c) for c in tiled} >= {0, 7, 15}
    assert {c.res for c in tiled} == {False, True} and {T.cin_pad(c) for c in tiled} >= {4, 36, 568}
    inf = [c for c in sn if c.inf]
    assert [c.id for c in inf] == ["tile-inf-corners"] and (inf[0].h, inf[0].w) == (37, 43) and inf[0].hints == T.BOTH


ACT = {"none": "ACT_NONE", "relu": "ACT_RELU", "leaky": "ACT_LEAKY", "sigmoid": "ACT_SIGMOID"}


def _desc(case, ops):
    """The shape fields of the case's descriptor as tests/test_cpu_conv_f32_cases.py builds them, plus what the two applicability rules
    read besides: the activation and a residual's pixel stride (behind a made-up, aligned, never dereferenced address)."""
    d = shape_desc(T.B, case)
    d.act = getattr(ops, ACT[case.act])
    if case.res:
        d.res, d.res_ps = 0x1000, (case.win_res or ((case.cout + 3) // 4 * 4, 0))[0]
    return d


def _smalln_rule(d, ops):
    """The condition under which ops._candidates offers hint 1 (= premvos::conv_smalln_applicable)."""
    return d.precision == ops._lib.PREC_F32 and d.cout <= 2 and d.out_mode == ops.OUT_NHWC and d.kh * d.kw * d.cin_pad >= 32 \
        and d.cout * d.k_pad * 4 <= 150 * 1024


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_descriptors_satisfy_the_applicability_rules(case):
    from premvos_amd import ops
    d = _desc(case, ops)
    assert (d.k_pad, d.cin_pad) == (T.k_pad(case), T.cin_pad(case))
    cands = ops._candidates(d)
    if case.kernel == "stream":
        assert ops.stream_applicable(d) and not _smalln_rule(d, ops)
        assert (5, 0, -1, 0, 0) in cands and not any(c[0] == 1 for c in cands)
        # the promise under test: the tuner times hint 5 against the GEMM tiles as an order-neutral choice
        tile = next(c for c in cands if c[0] > 6 and c[2] == -1)
        assert ops.numerics_key(d, (5, 0, -1, 0, 0)) == ops.numerics_key(d, tile)
    else:
        assert _smalln_rule(d, ops) and T.smalln_applicable(case) and not ops.stream_applicable(d)
        assert (1, 0, -1, 0, 0) in cands and ops.rule_choice(d) == (1, 0, -1, 0, 0) and not any(c[0] == 5 for c in cands)
    for hint, stage in case.hints:
        d.tile_hint, d.stage_k = hint, stage
        assert ops.workspace_bytes(d) == 0


def test_the_tuner_offers_hint_5_and_1_only_to_layers_the_table_covers():
    """ops._candidates reads only the shape fields, the activation and the residual.  A sweep over layers on and around the two
    kernels' domains: wherever the tuner offers hint 5 the table holds a case of that <KG, ACT, HAS_RES> and of that many column
    tiles; wherever it offers hint 1 the layer is in the family the table's direct cases span.  A K, an activation or an output width
    later added to a candidate rule without a case fails here."""
    from premvos_amd import ops
    stream_inst = {T.stream_instance(c) for c in T.STREAM_CASES}
    stream_cout = {c.cout for c in T.STREAM_CASES}
    direct_cout = {c.cout for c in T.SMALLN_CASES}
    k_floor = min(T.k_real(c) for c in T.SMALLN_CASES)
    lds_top = max(T.lds_bytes(c) for c in T.SMALLN_CASES)
    offered5, offered1 = set(), set()
    for cin, cout, k, stride, act, res in itertools.product(
            (4, 16, 28, 32, 48, 62, 64, 96, 126, 128, 192, 256, 512, 700), (1, 2, 3, 4, 64, 96, 128, 256, 384, 512, 640, 768, 1024),
            (1, 3), (1, 2), ("none", "relu", "leaky", "sigmoid"), (False, True)):
        pad = (k // 2,) * 4
        c = T.Case("sweep", "?", 2, 12, 14, cin, cout, k, stride, 1, pad, act, res, 3, None, None, None, True, False, (), False)
        d = _desc(c, ops)
        hints = {cand[0] for cand in ops._candidates(d)} | {ops.rule_choice(d)[0]}
        if 5 in hints:
            assert (k, stride) == (1, 1) and T.stream_instance(c) in stream_inst and cout in stream_cout, (cin, cout, k, stride, act, res)
            offered5.add(T.stream_instance(c))
        if 1 in hints:
            assert cout in direct_cout and k_floor <= T.k_real(c) and T.lds_bytes(c) <= lds_top, (cin, cout, k, stride)
            offered1.add(cout)
        assert (1 in hints) == T.smalln_applicable(c)
    assert offered5 == stream_inst and offered1 == {1, 2}
