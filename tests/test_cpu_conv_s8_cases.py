"""Without a GPU: the premises of tests/test_gpu_conv_s8_exact.py.  The lattice inputs of tests/conv_s8_cases.py split into bf16 hi / lo
without remainder -- so their S8 image holds all of them --, every case keeps S_abs below 2^13 -- so a float32 evaluation of the
product sums in any order is exact, which is why the GPU test may ask for equality --, the table reaches every kernel instance and
every mechanism its comments name, ops.pack_conv_s8 stores exactly the hi / lo parts the reference multiplies, and the host-side S8
encoder of the case module agrees with the package's decoder."""
import pytest
import torch

import conv_s8_cases as S

IDS = [c.id for c in S.CASES]


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_lattice_inputs_are_exact(case):
    data = S.inputs(case)
    for t in (data.x, data.w) + ((data.res,) if case.res == "s8" else ()):
        hi, lo = S.split(t)                                                      # asserts hi + lo == t
        assert hi.abs().min().item() >= 1 and hi.abs().max().item() == case.hmax and torch.equal(hi, hi.round())
        assert lo.abs().max().item() == 3 * S.QUANTUM and torch.equal(lo / S.QUANTUM, (lo / S.QUANTUM).round())
        assert torch.equal(S.decode_s8(S.encode_s8(S.nhwc(t))), S.nhwc(t))       # the S8 image holds all of it
    assert (data.b is not None) == case.bias and (data.res is not None) == (case.res is not None)
    for t in (data.b, data.res if case.res == "f32" else None):
        assert t is None or (t.abs().max().item() <= 8 and torch.equal(t / S.QUANTUM, (t / S.QUANTUM).round()))
    if case.res is not None:
        assert torch.equal(S.residual_value(case, data), data.res)               # hi + lo in float32 restores an S8 residual
    ref, (ref_hi, ref_lo) = S.expected(case)
    s_abs = S.s_abs(case)
    assert ref.shape == (case.n, case.cout) + S.out_extent(case) == s_abs.shape == ref_hi.shape == ref_lo.shape
    print(f"{case.id}: max S_abs = {s_abs.max().item():.1f}")
    assert s_abs.max().item() < S.S_ABS_LIMIT                                    # the exactness condition
    assert torch.equal(ref.float().double(), ref)                                # expected.float() loses nothing
    # every partial product is a multiple of 2^-11
    terms = S.product_terms("bf16x3", data.x, data.w)
    assert len(terms) == 3
    for a, b in terms:                                                           # (integer) x (multiple of 2^-11): never lo * lo
        assert torch.equal(a, a.round()) or torch.equal(b, b.round())
        prod = a.double().abs().max().item() * b.double().abs().max().item()
        assert prod <= case.hmax ** 2 and prod / S.QUANTUM == round(prod / S.QUANTUM)
        part = S.conv(case, a.double(), b.double())
        assert torch.equal(part / S.QUANTUM, (part / S.QUANTUM).round())
    pre64, _ = S.product_sum(case, data)
    pre32, _ = S.product_sum(case, data, torch.float32)
    assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)   # a float32 evaluation rounds nowhere
    assert torch.equal(pre64 / S.QUANTUM, (pre64 / S.QUANTUM).round())
    assert torch.equal(S.activate(case, pre32).double(), ref)
    assert ref_hi.dtype == ref_lo.dtype == torch.bfloat16
    assert torch.equal(ref_hi.float(), ref.float().to(torch.bfloat16).float())
    assert torch.equal(ref_lo.float(), (ref.float() - ref_hi.float()).to(torch.bfloat16).float())
    # the reference pins down WHICH terms are added: the three of them are far closer to the full product than hi.hi alone
    full = S.conv(case, data.x.double(), data.w.double())
    e3 = (full - sum(S.conv(case, a.double(), b.double()) for a, b in terms)).abs().max().item()
    e1 = (full - S.conv(case, terms[2][0].double(), terms[2][1].double())).abs().max().item()
    assert e1 > 100 * e3 > 0, (e1, e3)


def test_table_reaches_every_instance_and_every_mechanism():
    tiles = range(len(S.TILES))
    assert len(S.BY_ID) == len(S.CASES) == 12 and len(S.TILES) == 12
    assert S.TILES[S.PINGPONG_TILE] == S.TILES[0]                                # the fallback of tile 10 is tile 0's instance
    geo = {c.id: (S.rows(c), S.taps(c), S.kc32(c), c.cin // 8) for c in S.CASES}
    assert geo["pw-c8"] == (35, 1, 1, 1) and geo["pw-c64"] == (99, 1, 2, 8) and geo["pw-c96"] == (30, 1, 3, 12)
    assert geo["pw-c40"] == (1150, 1, 2, 5) and geo["pw-c728"] == (338, 1, 23, 91) and geo["pw-s2"] == (60, 1, 2, 8)
    assert geo["k3-c24"] == (198, 9, 1, 3) and geo["k3-c72"] == (272, 9, 3, 9) and geo["s2-pad01"] == (25, 9, 2, 8)
    assert geo["atrous"] == (216, 9, 2, 5) and geo["k7-c8"] == (120, 49, 1, 1) and geo["k1x3"] == (120, 3, 1, 2)
    assert S.out_extent(S.BY_ID["pw-s2"]) == (5, 6) and S.out_extent(S.BY_ID["s2-pad01"]) == (5, 5)
    assert S.out_extent(S.BY_ID["k7-c8"]) == (10, 12) and S.out_extent(S.BY_ID["k1x3"]) == (6, 20)
    for c in S.CASES:
        assert c.cin % 8 == 0 and c.cout % 8 == 0 and c.act in ("none", "relu", "leaky") and c.res in (None, "f32", "s8")
        assert S.taps(c) <= 49 and all(S.out_extent(c)) and S.cout_pad(c) % 256 == 0
        for name in ("in", "out8", "res8"):                                      # S8 windows: whole groups, 32-byte boundaries
            ps, off = S.window(c, name)
            assert ps % 8 == 0 and off % 8 == 0
        if c.win_in:                                                             # an absent chunk wrongly fetched stays inside the buffer
            assert c.win_in[0] >= c.win_in[1] + S._r(c.cin, 32) and c.win_in[1] > 0
        if c.win_out:
            assert c.win_out[0] % 4 == 0 and c.win_out[1] % 4 == 0 and c.win_out[1] > 0 and c.win_out[1] + c.cout < c.win_out[0]
        for win in (c.win_out8, c.win_res8):
            assert win is None or (win[1] > 0 and win[1] + c.cout < win[0])
        assert c.win_res8 is None or c.res == "s8"
    # every one of the 12 tiles gets both its PW and its general instantiation
    pw = [c for c in S.CASES if S.is_pw(c)]
    assert {c.id for c in pw} == {"pw-c8", "pw-c64", "pw-c96", "pw-c40", "pw-c728"}
    assert len(pw) >= 1 and len(pw) < len(S.CASES)                                # all cases run on all tiles
    names = {S.instance(c, t) for c in S.CASES for t in tiles}
    assert len(names) == 2 * 11 + 1 and "pingpong" in names                      # tiles 0 and 10 share two instances
    # stage counts: 1, 2 and 3, and a steady state of at least 2 * NSTAGE + 1 for every tile
    for t in tiles:
        kts = {S.kt(c, t) for c in S.CASES}
        assert max(kts) >= 2 * S.TILES[t][3] + 1
        if S.TILES[t][4] == 32:
            assert {1, 2, 3} <= kts, (t, kts)
        else:                                                                    # KC 16: every 32-block is two stages
            assert {2, 4, 6} <= kts and min(kts) == 2
        for kind in (True, False):                                               # ... in both instantiations
            assert max(S.kt(c, t) for c in S.CASES if S.is_pw(c) == kind) >= 2 * S.TILES[t][3] + 1
    assert {S.kt(c, S.PINGPONG_TILE) for c in pw} >= {1, 2, 3, 23}
    # a wholly absent KC-16 half-stage, in a pointwise and in a general layer
    assert S.absent_half_stage(S.BY_ID["pw-c8"]) and S.absent_half_stage(S.BY_ID["pw-c40"]) and S.absent_half_stage(S.BY_ID["k7-c8"])
    assert not S.absent_half_stage(S.BY_ID["k3-c24"]) and not S.absent_half_stage(S.BY_ID["pw-c728"])
    # tile 10 takes both its ping-pong form and its fallback
    assert {S.pingpong(c) for c in S.CASES} == {True, False} and all(S.pingpong(c) == S.is_pw(c) for c in S.CASES)
    # work-group counts above 8 that are no multiple of 8 (xcd_contiguous), and M smaller than every tile
    ragged = {S.work_groups(c, t) for c in S.CASES for t in tiles if S.work_groups(c, t) > 8 and S.work_groups(c, t) % 8}
    assert {S.work_groups(S.BY_ID["pw-c40"], t) for t in tiles} == {10, 15, 18, 25, 27} <= ragged
    assert S.rows(S.BY_ID["pw-c8"]) < min(bm for bm, *_ in S.TILES)
    assert {S.row_tiles(S.BY_ID["pw-c40"], t) for t in tiles} == {5, 9} and {S.row_tiles(S.BY_ID["k3-c72"], t) for t in tiles} == {2, 3}
    # a last column tile with 8 real columns at BN 64, 128 and 256
    for bn in (64, 128, 256):
        assert any(S.TILES[t][1] == bn and S.last_tile_columns(c, t) == 8 and S.col_tiles(c, t) > 1 for c in S.CASES for t in tiles)
    assert any(c.kh != c.kw for c in S.CASES) and any(S.taps(c) == 49 for c in S.CASES)
    assert any(S.taps(c) == 1 and c.stride == 2 and not S.is_pw(c) for c in S.CASES)
    assert {c.res for c in S.CASES} == {None, "f32", "s8"} and {c.act for c in S.CASES} == {"none", "relu", "leaky"}
    assert any(not c.bias for c in S.CASES) and all(i in S.BY_ID for i in S.GAUSSIAN)


def test_xcd_contiguous_restated_is_a_bijection():
    """premvos::xcd_contiguous of csrc/common.h, restated: the work-group counts of the table are the ones at which its remainder
    branch (nwg % 8 != 0) places work items, and every tile of a launch is owned by exactly one work-group."""
    def xcd_contiguous(i, nwg):
        xcd, local, q, r = i & 7, i >> 3, nwg >> 3, nwg & 7
        return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + local
    counts = {S.work_groups(c, t) for c in S.CASES for t in range(len(S.TILES))}
    assert {1, 2, 3, 10, 15, 18, 25, 27} <= counts
    for nwg in counts:
        assert sorted(xcd_contiguous(i, nwg) for i in range(nwg)) == list(range(nwg))


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_pack_conv_s8_stores_the_hi_and_lo_parts(case):
    from premvos_amd import ops
    data = S.inputs(case)
    pk = ops.pack_conv_s8(data.w, data.b, device="cpu")
    t, kc = S.taps(case), S.kc32(case)
    assert (pk.cin, pk.cout, pk.kh, pk.kw, pk.cout_pad) == (case.cin, case.cout, case.kh, case.kw, S.cout_pad(case))
    assert pk.cout_pad % 256 == 0 and pk.cout_pad >= case.cout
    assert pk.wgt.dtype == torch.bfloat16 and pk.wgt.is_contiguous() and pk.wgt.numel() == pk.cout_pad * t * kc * 64
    parts = pk.wgt.reshape(pk.cout_pad, t, kc, 4, 2, 8).float()                  # [cout_pad][tap][block][group][hi | lo][8]
    hi, lo = S.split(data.w)
    for part, want in ((0, hi), (1, lo)):
        got = parts[..., part, :].reshape(pk.cout_pad, t, kc * 32)               # channel = 32 block + 8 group + j
        full = torch.zeros((pk.cout_pad, t, kc * 32))
        full[:case.cout, :, :case.cin] = want.permute(0, 2, 3, 1).reshape(case.cout, t, case.cin)      # tap = ky * kw + kx
        assert torch.equal(got, full)                                            # rows and channels beyond the layer are zero
    if case.bias:
        assert pk.bias.shape == (pk.cout_pad,) and torch.equal(pk.bias[:case.cout], data.b) and not pk.bias[case.cout:].count_nonzero()
    else:
        assert pk.bias is None


def test_pack_conv_s8_applies_the_scale_in_float32_before_the_split():
    from premvos_amd import ops
    g = torch.Generator().manual_seed(11)
    w = torch.randn((24, 40, 3, 1), generator=g)
    scale = torch.randn((24,), generator=g) + 2
    pk = ops.pack_conv_s8(w, None, device="cpu", scale=scale)
    parts = pk.wgt.reshape(256, 3, 2, 4, 2, 8).float()
    hi, lo = S.hi_lo(w * scale.view(-1, 1, 1, 1))                                # one float32 product, then the split
    for part, want in ((0, hi), (1, lo)):
        got = parts[:24, :, :, :, part, :].reshape(24, 3, 64)
        assert torch.equal(got[..., :40], want.permute(0, 2, 3, 1).reshape(24, 3, 40)) and not got[..., 40:].count_nonzero()
    assert not parts[24:].count_nonzero()
    unscaled = ops.pack_conv_s8(w, None, device="cpu")
    assert not torch.equal(unscaled.wgt, pk.wgt)


def _special_values():
    bits = [0x00000000, 0x80000000 - 2 ** 32, 0x3F808000, 0x3F818000, 0x3F7FFFFF, 0x3F7F8000, 0x3F804040, 0x3F8040C0]
    return torch.tensor(bits, dtype=torch.int32).view(torch.float32)


def test_encode_and_decode_s8_round_trip_and_agree_with_ops():
    from premvos_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 3, 5, 24), generator=g) * torch.exp2(torch.randint(-20, 21, (2, 3, 5, 24), generator=g).float())
    x[0, 0, 0, :8] = _special_values()
    words = S.encode_s8(x)
    assert words.dtype == torch.int32 and words.shape == x.shape
    hi, lo = S.hi_lo(x)
    halves = words.view(torch.bfloat16).reshape(2, 3, 5, 3, 2, 8).float()        # group, hi | lo, 8
    assert torch.equal(halves[..., 0, :].reshape(x.shape), hi) and torch.equal(halves[..., 1, :].reshape(x.shape), lo)
    # byte order within a group: channel j of the hi half is the 16 bits at byte 2 j, of the lo half at byte 16 + 2 j
    one = torch.zeros(8)
    one[1], one[6] = 1.0, -2.0 - 2.0 ** -9                                       # hi 0x3F80; hi 0xC000, lo -2^-9 = 0xBB00
    assert S.encode_s8(one).tolist() == [0x3F80 << 16, 0, 0, 0xC000, 0, 0, 0, 0xBB00]
    dec = S.decode_s8(words)
    assert torch.equal(dec, hi + lo) and (dec - x).abs().max().item() <= 2.0 ** -16 * x.abs().max().item()
    again = S.encode_s8(dec)                                                     # hi + lo splits into the same halves; only -0 decodes to +0
    assert torch.equal(again.flatten()[1:], words.flatten()[1:]) and (again.flatten()[0], words.flatten()[0]) == (0, -2 ** 31)
    # the package's decoder reads a buffer this encoder wrote, windows included
    buf = torch.full((2, 3, 5, 48), S.NAN_WORD, dtype=torch.int32)
    buf[..., 16:40] = words
    view = ops.NHWC(buf.view(torch.float32), c=24, coff=16, layout="s8")
    assert torch.equal(view.torch(), dec.permute(0, 3, 1, 2))
    assert torch.equal(view.slice(8, 8).torch(), dec[..., 8:16].permute(0, 3, 1, 2))
    own = ops.NHWC(words.view(torch.float32), layout="s8")
    assert torch.equal(own.torch(), dec.permute(0, 3, 1, 2))
