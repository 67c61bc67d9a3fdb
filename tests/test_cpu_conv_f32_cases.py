"""Without a GPU: the premises of tests/test_gpu_conv_f32.py.  The lattice inputs of tests/conv_f32_cases.py make every product a
multiple of 2^-8, every case keeps S_abs below 2^16 -- so a float32 evaluation of the sums in any order is exact, which is why the GPU
test may ask for equality --, and the table reaches, by its shapes alone, every kernel instance and every mechanism its comments name."""
import pytest
import torch

import conv_f32_cases as B
from conv_exact_device import shape_desc

IDS = [c.id for c in B.CASES]


@pytest.mark.parametrize("case", B.CASES, ids=IDS)
def test_lattice_inputs_make_every_sum_exact(case):
    data = B.inputs(case)
    for t in (data.x, data.w):
        q = t * 16
        assert torch.equal(q, q.round()) and t.abs().min().item() >= 1 - 3 / 16 and t.abs().max().item() == case.hmax + 3 / 16
        assert set(((t.abs() + 0.25).floor()).unique().tolist()) == set(range(1, case.hmax + 1))          # every |h| occurs
    for t in (data.b, data.res):
        assert t is None or (t.abs().max().item() <= 8 and torch.equal(t / B.QUANTUM, (t / B.QUANTUM).round()))
    assert (data.res is not None) == case.res
    ref, s_abs = B.expected(case)
    assert ref.shape == (case.n, case.cout) + B.out_extent(case) == s_abs.shape
    print(f"{case.id}: max S_abs = {s_abs.max().item():.1f}")
    assert s_abs.max().item() < B.S_ABS_LIMIT == 2.0 ** 24 * B.QUANTUM             # the exactness condition
    assert torch.equal(ref.float().double(), ref)                                   # representable in float32
    pre64 = B.pre_activation(case, data)
    pre32 = B.pre_activation(case, data, torch.float32)
    assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)      # a float32 evaluation rounds nowhere
    assert torch.equal(pre64 / B.QUANTUM, (pre64 / B.QUANTUM).round()) and pre64.abs().max().item() <= s_abs.max().item()
    assert torch.equal(B.activate(case, pre32).double(), ref)
    # the data tells a dropped or doubled product from the right sum: no product is zero, and most outputs are not
    assert (ref != 0).float().mean().item() > (0.4 if case.act == "relu" else 0.9)


def test_table_reaches_every_instance_and_every_mechanism():
    assert len(B.BY_ID) == len(B.CASES) and all(i in B.BY_ID for i in B.GAUSSIAN)
    assert len(B.TILES) == 9 and len(B.PAIRS) == len(set(B.PAIRS)) == 13 and set(B.TILES_KB32) <= set(B.TILES)
    inst = B.instances()
    assert len(inst) == 65 and all(inst.values())                                   # every kernel is launched by some case
    geo = {c.id: (B.gemm_rows(c), B.cin_pad(c), B.k_pad(c)) for c in B.CASES}
    assert geo["k3-c20"] == (198, 20, 192) and geo["k7-c3"] == (99, 4, 208) and geo["pw-c32"] == (35, 32, 32)
    assert geo["pw-c728"] == (169, 728, 736) and geo["pw-s2-c200"] == (168, 200, 208) and geo["atrous"] == (216, 36, 336)
    assert geo["s2-pad01"] == (25, 64, 576) and geo["scalar-c134"] == (126, 24, 32) and geo["deconv"] == (60, 40, 368)
    assert geo["deconv-c132"] == (28, 132, 1200) and geo["tail-pw"] == (429, 72, 80) and geo["tail-k3"] == (429, 12, 112)
    assert geo["tail-deconv"] == (270, 20, 192) and geo["pw-c64"] == (180, 64, 64) and geo["head-c36"] == (1591, 36, 336)
    for c in B.CASES:
        assert c.act in ("none", "relu", "leaky") and all(B.out_extent(c)) and B.k_pad(c) - B.k_real(c) < 16
        if c.win_in:
            assert c.win_in[0] % 4 == 0 and c.win_in[1] % 4 == 0 and c.win_in[1] + B.cin_pad(c) <= c.win_in[0]
        if c.win_out:
            assert c.win_out[1] + c.cout <= c.win_out[0] and c.win_out[0] > c.cout
        assert not (c.deconv and c.res)                                             # (the library: a residual needs NHWC output)

    all_launches = [(c, l) for c in B.CASES for l in B.launches(c)]
    # both reduce forms with m_begin 0 and with m_begin > 0, for every tile
    for tile in B.TILES:
        seen = {(l.reduce, B.m_begin(c, tile, l) > 0) for c, l in all_launches if l.reduce}
        assert seen == {(k, b) for k in ("nhwc", "pixshuf") for b in (False, True)}, tile
    # k-slices: the count the case asks for at either stage depth, a short last slice, single-stage slices
    for c, l in all_launches:
        if l.reduce:
            for st in (16, 32):
                per, count, last = B.slices(c, st, l.split_k if l.split_k > 1 else l.tail[1])
                assert count > 1 and 0 < last <= per
    assert B.slices(B.BY_ID["pw-c728"], 16, 4) == (12, 4, 10) and B.slices(B.BY_ID["pw-c728"], 32, 4) == (6, 4, 5)
    assert B.slices(B.BY_ID["tail-pw"], 16, 3) == (2, 3, 1) and B.slices(B.BY_ID["tail-pw"], 32, 3) == (1, 3, 1)
    assert B.slices(B.BY_ID["tail-k3"], 16, 3) == (3, 3, 1) and B.slices(B.BY_ID["tail-k3"], 32, 3) == (2, 2, 2)
    assert B.slices(B.BY_ID["deconv"], 16, 2) == (12, 2, 11)
    # NARROW with one, two and three live column blocks, on general and on pointwise layers; not where the store is scalar
    nvn = {n for c, l in all_launches for n in B.narrow_blocks(c, (128, 128), l)}
    assert nvn == {1, 2, 3}
    assert B.narrow_blocks(B.BY_ID["k3-c20"], (128, 128), B.launches(B.BY_ID["k3-c20"])[0]) == [1]
    assert B.narrow_blocks(B.BY_ID["pw-c728"], (128, 128), B.launches(B.BY_ID["pw-c728"])[0]) == [2]
    assert B.narrow_blocks(B.BY_ID["pw-c728"], (128, 128), B.launches(B.BY_ID["pw-c728"])[1]) == []        # never with k-slices
    assert B.narrow_blocks(B.BY_ID["pw-s2-c200"], (128, 128), B.launches(B.BY_ID["pw-s2-c200"])[0]) == [3]
    sc = B.BY_ID["scalar-c134"]
    assert not B.wide_ok(sc) and sc.cout % 4 and sc.win_out[1] % 2 and 0 < sc.cout - 128 <= 96 and B.narrow_blocks(sc, (128, 128), B.launches(sc)[0]) == []
    assert sum(B.wide_ok(c) for c in B.CASES) >= 8 and not any(B.wide_ok(c) for c in B.CASES if c.deconv)
    # empty 32-column blocks of a wave (nvalid < NTL) in every tile whose waves are wider than one block
    for tile in B.TILES:
        wide_wave = B.tile_bn(tile) // B.WAVES[tile][1] > 32
        assert any(B.skipped_blocks(c, tile) for c in B.CASES) == wide_wave, tile
    # k_pad % 32 == 16 on the PW and on the general path; the single 32-deep stage; a partly filled last stage at either depth
    assert any(B.is_pw(c) and B.k_pad(c) % 32 == 16 for c in B.CASES) and any(not B.is_pw(c) and B.k_pad(c) % 32 == 16 for c in B.CASES)
    assert any(B.k_pad(c) == 32 for c in B.CASES)
    for st in (16, 32):
        groups = {min(st // 8, -(-(B.k_real(c) - (-(-B.k_pad(c) // st) - 1) * st) // 8)) for c in B.CASES}     # h_last
        assert groups == set(range(1, st // 8 + 1)), (st, groups)
        # ... and a last real group that is not the stage's first and is half filled: rounding the group count down loses products
        rem = {c.id: B.k_real(c) - (-(-B.k_pad(c) // st) - 1) * st for c in B.CASES}
        assert rem["tail-k3"] == 12 and any(r > 8 and r % 8 for r in rem.values()), (st, rem)
    # pointwise addressing: unit and strided
    assert any(B.is_pw(c) and B.pw_unit(c) for c in B.CASES) and any(B.is_pw(c) and not B.pw_unit(c) for c in B.CASES)
    s2 = B.BY_ID["pw-s2-c200"]
    assert (-(-B.k_pad(s2) // 16) - 1) * 16 <= B.cin_pad(s2) < B.k_pad(s2)           # interior loads with a half-real last stage
    # interior tiles (unpredicated loads) for every BM, in every tile whose staging divides evenly; a ragged last row tile for every BM;
    # rows of more than one image inside a row tile; a workgroup count that is no multiple of 8 (the XCD swizzle's remainder)
    for tile in B.TILES:
        even = tile not in ((128, 96), (128, 32))
        assert any(B.interior_tiles(c, tile, 16) for c in B.CASES) == even, tile
        assert not any(B.interior_tiles(c, tile, 32) for c in B.CASES)
        assert any(B.gemm_rows(c) % tile[0] and B.gemm_rows(c) > tile[0] for c in B.CASES), tile
        assert any(w % 8 for c, l in all_launches for w in B.workgroups(c, tile, l)), tile
        assert any(w > 8 and w % 8 for c, l in all_launches for w in B.workgroups(c, tile, l)) or tile[0] == 256, tile
    assert B.interior_tiles(B.BY_ID["tail-pw"], (256, 128), 16) == 1 and B.interior_tiles(B.BY_ID["pw-s2-c200"], (128, 128), 16) == 1
    assert any(c.n > 1 and (B.gemm_rows(c) // c.n) % 64 for c in B.CASES if not c.deconv and c.k > 1)
    # the same-products kernels
    hints = {h: [c.id for c in B.CASES if h in c.hints] for h in ((1, 0), (1, 1), (5, 0), (6, 0))}
    assert hints == {(1, 0): ["head-c36"], (1, 1): ["head-c36"], (5, 0): ["pw-c64"], (6, 0): ["pw-c728", "pw-s2-c200"]}
    head = B.BY_ID["head-c36"]
    assert -(-head.h // 4) * -(-head.w // 4) >= 100 and B.k_real(head) >= 32          # the direct kernel's tiled form applies


def _desc(case):
    return shape_desc(B, case)


@pytest.mark.parametrize("case", B.CASES, ids=IDS)
def test_workspace_is_asked_for_exactly_by_the_split_and_tail_launches(case):
    from premvos_amd import ops
    d = _desc(case)
    for tile, stage in B.PAIRS:
        for l in B.launches(case):
            d.tile_hint, d.stage_k, d.split_k, (d.tail_m_tiles, d.tail_split_k) = (tile[0] << 16) | tile[1], stage, l.split_k, l.tail
            need = ops.workspace_bytes(d)
            assert need == B.workspace_need(case, tile, stage, l), (tile, stage, l.name)
            assert (need > 0) == (l.reduce is not None) == (len(l.forms) > 1 or l.forms[0].startswith("splitk"))
    for hint, stage in case.hints:
        d.tile_hint, d.stage_k, d.split_k, d.tail_m_tiles, d.tail_split_k = hint, stage, -1, 0, 0
        assert ops.workspace_bytes(d) == 0


def test_the_tuner_offers_no_fp32_tile_or_stage_the_table_does_not_hold():
    """ops._candidates reads only the shape fields.  A tile or stage depth later added to the fp32 candidate list without being added to
    the table (and thereby to the exact GPU test) fails here."""
    from premvos_amd import ops
    pairs = {((t[0] << 16) | t[1], st) for t, st in B.PAIRS}
    offered = set()
    for c in B.CASES:
        for scale in (1, 12, 40):                                # up to 1600 x the pixels: the large-M tiles (256x128, 256x129) appear
            d = _desc(c)
            d.h, d.w, d.ho, d.wo = d.h * scale, d.w * scale, d.ho * scale, d.wo * scale
            for hint, st, sk, tail_rows, tail_split in ops._candidates(d) + [ops.rule_choice(d)]:
                if hint > 6:
                    assert (hint, st) in pairs, (c.id, scale, hint >> 16, hint & 0xffff, st)
                    offered.add((hint, st))
    assert offered == pairs
