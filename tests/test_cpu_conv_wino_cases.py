"""Without a GPU: the premises of tests/test_gpu_conv_wino_exact.py.  The lattice inputs of tests/conv_wino_cases.py make both filter
transforms whole multiples of one quantum (asserted on what ops.pack_winograd / ops.pack_winograd4 return), every case keeps M_abs and
Y_abs below 2^24 quanta for every family that takes it -- so a float32 evaluation of either Winograd algorithm in any order is exact,
which is why the GPU test may ask for equality --, the restated algorithms equal the direct convolution, and the table reaches, by its
shapes alone, each of the 24 kernels and every mechanism its comments name."""
import pytest
import torch

import conv_wino_cases as B

ALL = B.CASES + B.DENSE
IDS = [c.id for c in ALL]
Q = B.QUANTUM


def _whole(t, q=Q):
    return torch.equal(t / q, (t / q).round())


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_lattice_inputs_make_every_winograd_sum_exact(case):
    data = B.inputs(case)
    assert set(data.x.unique().tolist()) == {-1.0, 0.0, 1.0} and set((data.w / B.WEIGHT).unique().tolist()) == {-1.0, 0.0, 1.0}
    for t in (data.x, data.w):
        assert abs((t != 0).float().mean().item() - case.density) < 0.06
    for t in (data.b, data.res):
        assert t is None or (t.abs().max().item() <= 8 and _whole(t))
    assert (data.res is not None) == case.res
    ref = B.expected(case)
    assert ref.shape == (case.n, case.cout) + B.out_extent(case)
    assert torch.equal(ref.float().double(), ref)                                   # representable in float32
    pre64 = B.pre_activation(case, data)
    assert torch.equal(pre64.float().double(), pre64) and _whole(pre64)             # expected(case).float() loses nothing
    assert torch.equal(B.activate(case, pre64.float()).double(), ref)
    assert (ref != 0).float().mean().item() > (0.4 if case.act == "relu" else 0.9)  # the data tells a wrong sum from the right one
    direct = B.conv(case, data.x.double(), data.w.double())
    for m in sorted({B.FAMILY[h] for h in B.HINTS if B.takes(case, h)}):
        # the filter transform is a whole number of quanta, the input transform an integer of at most 100 x the data
        u = B.filter_transform(data.w, m)
        v = B.input_transform(case, data.x, m)
        assert _whole(u) and _whole(v, 1.0) and v.abs().max().item() <= (100 if m == 4 else 4)
        # the exactness condition, in quanta
        m_abs, y_abs, y_tiles = B.magnitudes(case, data, m)
        assert m_abs.shape[1:3] == (case.cout, case.dil ** 2) and m_abs.shape[0] * m_abs.shape[2] * m_abs.shape[3] * m_abs.shape[4] == B.tiles(case, m)
        print(f"{case.id} F({m}x{m}): max M_abs = {m_abs.max().item() / Q:.3g}, max Y_abs = {y_abs.max().item() / Q:.3g} quanta")
        assert m_abs.max().item() / Q < B.LIMIT
        assert y_abs.max().item() / Q < B.LIMIT and (y_tiles + 16) / Q < B.LIMIT
        # the restated algorithm is the convolution, exactly
        assert torch.equal(B.winograd(case, data.x, data.w, m), direct)
        assert (y_abs >= pre64.abs()).all() and (B.bound_scale(case, data, m) >= y_abs).all()


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_packed_filter_transforms_are_whole_quanta(case):
    """What the library multiplies by: ops.pack_winograd / pack_winograd4 evaluate G g G^T their own way (element-wise float64 sums and
    divisions by 6 and 24, rounded once to float32).  On the lattice they must return the restated transform, rounded nowhere."""
    from premvos_amd import ops
    data = B.inputs(case)
    cp, op, kp = B.cin_pad(case), B.cout_pad(case), B.kp(case)
    for m, pack in ((2, ops.pack_winograd), (4, ops.pack_winograd4)):
        u = pack(data.w, cp, op)
        p = (m + 2) ** 2
        assert u.dtype == torch.float32 and tuple(u.shape) == (p, op, kp)
        assert _whole(u.double())
        want = B.filter_transform(data.w, m).permute(2, 3, 0, 1).reshape(p, case.cout, case.cin)
        assert torch.equal(u[:, :case.cout, :case.cin].double(), want)
        assert not u[:, case.cout:].any() and not u[:, :, case.cin:].any()


def test_gaussian_restatement_is_the_convolution():
    """On full-mantissa data the restated algorithms agree with the direct float64 convolution to float64 rounding, and the scale of the
    derived bound dominates the conv's own."""
    for cid in B.GAUSSIAN:
        case = B.BY_ID[cid]
        data = B.gaussian_inputs(case)
        direct = B.conv(case, data.x.double(), data.w.double())
        plain = B.conv(case, data.x.double().abs(), data.w.double().abs())
        for m in (2, 4):
            s_w = B.bound_scale(case, data, m)
            assert ((B.winograd(case, data.x, data.w, m) - direct).abs() <= 1e-12 * s_w).all()
            assert (s_w * (1 + 1e-12) >= plain).all() and s_w.min().item() > 0


def _one(case_id, hint, stage_k):
    return B.kernels(B.BY_ID[case_id], hint, stage_k)


def test_table_reaches_every_kernel_and_every_mechanism():
    assert len(B.BY_ID) == len(B.CASES) == 8 and all(i in B.BY_ID for i in B.GAUSSIAN)
    assert len(B.BLOCKS) == 12 and len(B.ALL_KERNELS) == len(set(B.ALL_KERNELS)) == 24 and len(B.WINO4_GEMM) == 9
    inst = B.instances()
    assert set(inst) == set(B.ALL_KERNELS) | {B.SLAB_ENTRY} and all(inst.values()), [k for k, v in inst.items() if not v]
    assert all(c.cout >= B.WINO4_MIN_COUT and c.cin >= B.WINO4_MIN_C and c.cout % 4 == 0 for c in B.CASES + B.DENSE)
    geo = {c.id: (B.cin_pad(c), B.kp(c), B.tiles(c, 2), B.tiles(c, 4)) for c in B.CASES}
    assert geo == {"c20-n136": (20, 32, 60, 18), "ragged-m": (48, 48, 585, 168), "c64-n32": (64, 64, 572, 168),
                   "long-k": (536, 544, 35, 12), "atrous-2": (36, 48, 96, 32), "atrous-4-small": (16, 16, 32, 16),
                   "pad-2-0": (32, 32, 36, 9), "scalar-store": (24, 32, 12, 4)}
    # which family takes what: hint 2 no atrous case, hints 3 and 4 all of them
    assert [c.id for c in B.CASES if not B.takes(c, 2)] == ["atrous-2", "atrous-4-small"]
    assert all(B.takes(c, 3) and B.takes(c, 4) for c in B.CASES)
    for c in B.CASES:
        for win, width in ((c.win_in, B.cin_pad(c)), (c.win_out, c.cout)):
            assert win is None or (win[1] + width <= win[0] and win[0] > width)
        assert c.win_in is None or (c.win_in[0] % 4 == 0 and c.win_in[1] % 4 == 0)

    c20 = B.BY_ID["c20-n136"]
    assert B.cin_pad(c20) < B.kp(c20) and c20.win_in[1] + B.kp(c20) > c20.win_in[0]    # the K padding reaches past the pixel: sentinels
    assert c20.win_in == (28, 4) and c20.win_out == (144, 4) and B.wide_ok(c20)
    assert all(B.tiles(c20, B.FAMILY[h]) < B.block(c20, h, b)[0] for h, b in B.BLOCKS)   # fewer tiles than any block has rows
    assert B.grid(c20, 4, 0) == (1, 2) and B.grid(c20, 2, 0) == (1, 2) and B.grid(c20, 3, 0) == (1, 2)
    assert c20.cout - 128 == 8 and B.cout_pad(c20) == 160 < 256 and c20.h % 2 and c20.w % 2 and c20.h % 4 and c20.w % 4

    rag = B.BY_ID["ragged-m"]
    assert B.kp(rag) % 32 == 16
    assert _one("ragged-m", 4, 0)[1] == "wino4_gemm_kernel<128,64,2,2,16>" and _one("ragged-m", 4, 64)[1] == "wino4_gemm_kernel<64,64,2,2,16>"
    assert B.kp(rag) // 16 == 3 and [b for b in B.HINTS[3] if B.half_stage(rag, 3, b)] == [4, 5, 6]
    assert B.grid(rag, 4, 0)[0] == 2 and B.grid(rag, 4, 64)[0] == 3 and B.tiles(rag, 4) == 128 + 40 == 2 * 64 + 40
    assert B.grid(rag, 2, 0)[0] == 5 and B.grid(rag, 2, 64)[0] == 10 and B.tiles(rag, 2) % 64
    assert all(B.block(rag, h, b)[1] == 64 for h, b in B.BLOCKS if h != 3) and rag.cout == 40

    c64 = B.BY_ID["c64-n32"]
    assert _one("c64-n32", 4, 0)[1] == _one("c64-n32", 4, 64)[1] == "wino4_gemm_kernel<128,32,4,1,32>" and B.grid(c64, 4, 0) == (2, 1)
    assert _one("c64-n32", 4, 16)[1] == "wino4_gemm_kernel<128,64,2,2,16>" and _one("c64-n32", 4, 80)[1] == "wino4_gemm_kernel<64,64,2,2,16>"
    assert _one("c64-n32", 2, 0)[0] == _one("c64-n32", 2, 64)[0] == "wino_gemm_kernel<128,32,4,1>"
    assert [k for k, v in inst.items() if k.startswith("wino4_gemm_kernel<128,32") and all(i.startswith(("c64-n32", "long-k")) for i in v)]

    lk = B.BY_ID["long-k"]
    assert (B.cin_pad(lk), B.kp(lk)) == (536, 544) and B.kp(lk) == 17 * 32 == max(B.kp(c) for c in B.CASES)

    a2 = B.BY_ID["atrous-2"]
    assert B.phase_sizes(a2) == ([7, 6], [5, 5]) and B.phase_tiles(a2, 2) == (4, 3) and B.phase_tiles(a2, 4) == (2, 2)   # 8 > 7, 6 > 5: past the map
    a4 = B.BY_ID["atrous-4-small"]
    assert a4.h < 4 * a4.dil and a4.w < 4 * a4.dil and 1 in B.phase_sizes(a4)[1] and B.phase_sizes(a4) == ([3, 2, 2, 2], [2, 2, 2, 1])
    assert B.kp(a4) == 16 and all(B.half_stage(a4, 3, b) for b in (4, 5, 6)) and B.block(a4, 4, 0) == (128, 128, 16) and a4.cout == 96

    p20 = B.BY_ID["pad-2-0"]
    assert B.out_extent(p20) == (12, 11) and p20.pad == (2, 0) and p20.dil == 1
    sc = B.BY_ID["scalar-store"]
    assert not B.wide_ok(sc) and sc.win_out[0] % 4 and sc.win_out[1] % 2 and _one("scalar-store", 4, 0)[2] == "wino4_output_kernel<false>"
    assert sum(B.wide_ok(c) for c in B.CASES) == 7

    # the GEMM loops: a single stage (epilogue only), two, many; every instance at both depths has a case with more than one stage
    for h, b in B.BLOCKS:
        stages = {B.kp(c) // B.block(c, h, b)[2] for c in B.CASES if B.takes(c, h) and not B.half_stage(c, h, b)}
        assert max(stages) >= 17 and min(stages) <= 2, (h, b, stages)
    assert B.kp(a4) // 16 == 1
    # interior row tiles and a ragged last one for every row count of every family
    for h, b in B.BLOCKS:
        assert any(B.grid(c, h, b)[0] > 1 and B.tiles(c, B.FAMILY[h]) % B.block(c, h, b)[0] for c in B.CASES if B.takes(c, h)), (h, b)
    # residual and every activation but sigmoid in every family
    for h in B.HINTS:
        took = [c for c in B.CASES if B.takes(c, h)]
        assert {c.act for c in took} == {"none", "relu", "leaky"} and {c.res for c in took} == {False, True}

    # the dense block: layer 1 reads what layer 0 read behind 32 new channels; the plan of ops.wino4_slab_plan
    d0, d1 = B.DENSE
    assert torch.equal(B.inputs(d0).x, B.inputs(d1).x[:, 32:]) and d0.win_out[1] == d1.win_in[1] == 32
    assert d0.win_in[1] + d0.cin == d1.win_in[1] + d1.cin == B.DENSE_PS and (B.kp(d0), B.kp(d1)) == (48, 80)
    assert all(B.block(d, 4, sk)[1:] == (64, 16) for d in B.DENSE for sk in B.HINTS[4]) and B.tiles(d0, 4) == 9


def _desc(case, hint, stage_k):
    """The shape fields of the case's descriptor (what premvos_conv2d_workspace_bytes and ops._candidates read).  The filter
    transforms are claimed by a non-null value that nothing dereferences."""
    from premvos_amd import _lib
    d = _lib.ConvDesc()
    d.n, d.h, d.w = case.n, case.h, case.w
    d.ho, d.wo = B.out_extent(case)
    d.cin, d.cin_pad, d.cout, d.cout_pad = case.cin, B.cin_pad(case), case.cout, B.cout_pad(case)
    d.in_ps = (case.win_in or (B.cin_pad(case), 0))[0]
    d.out_ps = (case.win_out or ((case.cout + 3) // 4 * 4, 0))[0]
    d.kh = d.kw = 3
    d.sh = d.sw = 1
    d.dh = d.dw = case.dil
    d.pt, d.pl = case.pad
    d.k_pad = (9 * B.cin_pad(case) + 15) // 16 * 16
    d.precision = _lib.PRECISIONS["fp32"]
    d.out_mode, d.cout_ps = _lib.OUT_NHWC, 0
    d.wgt_wino = d.wgt_wino4 = 16
    d.tile_hint, d.stage_k, d.split_k = hint, stage_k, -1
    return d


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_workspace_query_returns_the_table_s_figure(case):
    from premvos_amd import ops
    for hint, stage_k in B.BLOCKS:
        need = ops.workspace_bytes(_desc(case, hint, stage_k))
        if B.takes(case, hint):
            mt, (_, bn, _) = B.tiles(case, B.FAMILY[hint]), B.block(case, hint, stage_k)
            nt = -(-case.cout // bn)
            assert need == B.workspace_need(case, hint, stage_k) == {2: 16 * mt * nt * bn * 4, 3: 0, 4: 36 * mt * (B.kp(case) + nt * bn) * 4}[hint]
            assert (need > 0) == (hint != 3)
        else:
            assert need == 0
    assert B.m_slab_need(case, 0) == B.workspace_need(case, 4, 0) - 36 * B.tiles(case, 4) * B.kp(case) * 4


def test_the_tuner_offers_no_winograd_block_the_table_does_not_hold():
    """ops._candidates reads only the shape fields.  A Winograd block later offered to the tuner without being added to the table (and
    thereby to the exact GPU test) fails here; and the dense block gets the plan the table expects."""
    from premvos_amd import ops
    offered = set()
    for c in B.CASES:
        d = _desc(c, 0, 0)
        cands = ops._candidates(d) + [ops.rule_choice(d)]
        for hint, sk, split, tail_rows, tail_split in cands:
            if hint in (2, 3, 4):
                assert (hint, sk) in B.BLOCKS and B.takes(c, hint), (c.id, hint, sk)
                offered.add((hint, sk))
        # (the slab-free kernel is not offered to cout <= 32: the GPU test adds its blocks by hand)
        assert {h for h in B.HINTS if B.takes(c, h) and (h != 3 or c.cout > 32)} == {cand[0] for cand in cands if cand[0] in (2, 3, 4)}, c.id
        assert len({ops.numerics_key(d, (h, b, -1, 0, 0)) for h, b in B.BLOCKS}) == 3      # one key per family: blocks are timed against each other
    assert offered == set(B.BLOCKS)
    layers = [(_desc(c, 4, 0), c.win_in[1]) for c in B.DENSE]
    need, plan = ops.wino4_slab_plan(layers)
    assert need == 36 * B.tiles(B.DENSE[0], 4) * B.DENSE_PS and [p[1:] for p in plan] == B.DENSE_PLAN
