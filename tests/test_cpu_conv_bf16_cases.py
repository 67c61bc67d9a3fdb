"""Without a GPU: the premises of tests/test_gpu_conv_bf16.py.  The lattice inputs of tests/conv_bf16_cases.py split into bf16 hi / lo
without remainder, every case keeps S_abs below 2^13 -- so a float32 evaluation of the product sums in any order is exact, which is why
the GPU test may ask for equality --, the table names every (tile, stage depth) the tuner can offer in the bf16 modes, and the weight
packers store exactly the hi / lo parts the reference multiplies."""
import pytest
import torch

import conv_bf16_cases as B


@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_lattice_inputs_are_exact_for_both_precisions(case):
    data = B.inputs(case)
    for t in (data.x, data.w):
        hi, lo = B.split(t)                                                      # asserts hi + lo == t
        assert hi.abs().min().item() >= 1 and hi.abs().max().item() == case.hmax and torch.equal(hi, hi.round())
        assert lo.abs().max().item() == 3 * B.QUANTUM and torch.equal(lo / B.QUANTUM, (lo / B.QUANTUM).round())
    for t in (data.b, data.res):
        assert t is None or (t.abs().max().item() <= 8 and torch.equal(t / B.QUANTUM, (t / B.QUANTUM).round()))
    assert (data.res is not None) == case.res
    for prec in B.PRECISIONS:
        ref, s_abs = B.expected(case, prec)
        assert ref.shape == (case.n, case.cout) + B.out_extent(case) == s_abs.shape
        print(f"{case.id} {prec}: max S_abs = {s_abs.max().item():.1f}")
        assert s_abs.max().item() < B.S_ABS_LIMIT                               # the exactness condition
        assert torch.equal(ref.float().double(), ref)                            # representable in float32
        pre64, _ = B.product_sum(case, prec, data)
        pre32, _ = B.product_sum(case, prec, data, torch.float32)
        assert pre32.dtype == torch.float32 and torch.equal(pre32.double(), pre64)   # a float32 evaluation rounds nowhere
        assert torch.equal(pre64 / B.QUANTUM, (pre64 / B.QUANTUM).round())
        assert torch.equal(B.activate(case, pre32).double(), ref)
    # the reference tells the precisions apart, and both from the true convolution: it pins down WHICH terms are added
    true, _ = B.true_conv(case, data)
    e1 = (B.expected(case, "bf16")[0] - true).abs().max().item()
    e3 = (B.expected(case, "bf16x3")[0] - true).abs().max().item()
    assert e1 > 100 * e3 > 0, (e1, e3)


def test_table_names_every_tile_and_stage_and_every_mechanism():
    assert len(B.BY_ID) == len(B.CASES) == 8
    assert sorted(B.TILES) == sorted((bm, bn) for bm in (64, 128) for bn in (32, 64, 128)) and B.STAGES == [16, 32]
    assert len({(t, s) for t in B.TILES for s in B.STAGES}) == 12
    forms = {f for c in B.CASES for f, _ in B.launches(c)}
    assert forms == {"plain", "pixshuf", "splitk"}                               # x 12 x 2 precisions = the 72 instances
    assert any(c.deconv and c.split_k for c in B.CASES) and any(not c.deconv and c.split_k for c in B.CASES)
    geo = {c.id: (c.n * B.gemm_extent(c)[0] * B.gemm_extent(c)[1], B.cin_pad(c), B.k_pad(c)) for c in B.CASES}
    assert geo["k3-c20"] == (198, 20, 192) and geo["k7-c3"] == (99, 4, 224) and geo["pw-c32"] == (35, 32, 32)
    assert geo["pw-c728"] == (169, 728, 736) and geo["atrous"] == (216, 36, 352) and geo["s2-pad01"] == (25, 64, 576)
    assert geo["deconv"] == (60, 40, 384) and geo["deconv-c132"] == (28, 132, 1216)
    for c in B.CASES:
        assert c.act in ("none", "relu", "leaky") and all(B.out_extent(c))
        if c.win_in:
            assert c.win_in[0] % 4 == 0 and c.win_in[1] % 4 == 0 and c.win_in[1] + B.cin_pad(c) <= c.win_in[0]
        if c.win_out:
            assert c.win_out[1] + c.cout <= c.win_out[0] and c.win_out[0] > c.cout
        if c.split_k:                                                            # the slices the case table promises: a short last one
            for st in B.STAGES:
                kt = B.k_pad(c) // st
                per = -(-kt // c.split_k)
                assert -(-kt // per) == c.split_k, (c.id, st)
                if c.id == "pw-c728":
                    assert (per, kt - (c.split_k - 1) * per) == {32: (6, 5), 16: (12, 10)}[st]
    assert all(i in B.BY_ID for i in B.GAUSSIAN)


def _desc(_lib, prec, m_hw, cin, cout, k):
    d = _lib.ConvDesc()
    d.n, d.h, d.w, d.ho, d.wo = 1, m_hw, m_hw, m_hw, m_hw
    d.cin, d.cin_pad, d.cout, d.cout_pad = cin, (cin + 3) // 4 * 4, cout, (cout + 31) // 32 * 32
    d.in_ps, d.out_ps = d.cin_pad, (cout + 3) // 4 * 4
    d.kh = d.kw = k
    d.sh = d.sw = d.dh = d.dw = 1
    d.pt = d.pl = k // 2
    d.k_pad = (k * k * d.cin_pad + 31) // 32 * 32
    d.precision, d.out_mode = _lib.PRECISIONS[prec], _lib.OUT_NHWC
    return d


def test_the_tuner_offers_nothing_the_table_does_not_hold():
    """ops._candidates reads only the shape fields of a descriptor, so the descriptors need no device pointers.  A tile or stage depth
    later added to the candidate list of the bf16 modes without a test case fails here."""
    from premvos_amd import _lib, ops
    pairs = {((bm << 16) | bn, st) for bm, bn in B.TILES for st in B.STAGES}
    offered = set()
    for prec in B.PRECISIONS:
        for cout in (2, 64, 136):
            for cin, k in ((20, 3), (728, 1), (256, 3)):                         # k_pad 192, 736 and 2304: without and with k-slices
                for m_hw in (5, 40, 400):                                        # 25 ... 160 000 output pixels
                    d = _desc(_lib, prec, m_hw, cin, cout, k)
                    cands = ops._candidates(d)
                    assert cands
                    for hint, st, sk, tail_rows, tail_split in cands:
                        assert (hint, st) in pairs, (prec, cout, cin, k, m_hw, hint >> 16, hint & 0xffff, st)
                        assert sk in (-1, 2, 4, 8) and (tail_rows, tail_split) == (0, 0)
                        offered.add((hint, st))
                    hint, st = ops.rule_choice(d)[:2]
                    assert (hint, st) in pairs
    assert offered == pairs                                                      # and the table holds nothing the tuner never offers


def _expected_matrix(w_oihw, cout_pad, k_pad):
    """[cout_pad][k_pad] with k = (kh * KW + kw) * cin_pad + c (include/premvos_hip.h), zero elsewhere."""
    cout, cin, kh, kw = w_oihw.shape
    cp = (cin + 3) // 4 * 4
    m = torch.zeros((cout_pad, k_pad))
    for y in range(kh):
        for x in range(kw):
            k0 = (y * kw + x) * cp
            m[:cout, k0:k0 + cin] = w_oihw[:, :, y, x]
    return m


def _deconv_as_conv(w):
    """pack_deconv4x4s2's docstring, written out again: phase 2 * py + px of ConvTranspose2d(4, stride 2, pad 1) is a 3x3 conv whose
    tap (dy + 1, dx + 1) holds the transposed kernel's (ky, kx); py = 0: (dy, ky) in (0, 1), (-1, 3); py = 1: (0, 2), (1, 0)."""
    cin, cout = w.shape[:2]
    taps = {0: ((0, 1), (-1, 3)), 1: ((0, 2), (1, 0))}
    w3 = torch.zeros((4 * cout, cin, 3, 3))
    for py in (0, 1):
        for px in (0, 1):
            for dy, ky in taps[py]:
                for dx, kx in taps[px]:
                    for co in range(cout):
                        w3[(2 * py + px) * cout + co, :, dy + 1, dx + 1] = w[:, co, ky, kx]
    return w3


@pytest.mark.parametrize("prec", B.PRECISIONS)
@pytest.mark.parametrize("case", B.CASES, ids=[c.id for c in B.CASES])
def test_packers_store_the_hi_and_lo_parts_of_lattice_weights(case, prec):
    from premvos_amd import _lib, ops
    data = B.inputs(case)
    pack = ops.pack_deconv4x4s2 if case.deconv else ops.pack_conv
    pk = pack(data.w, data.b, device="cpu", precision=prec)
    cout, cout_pad, kp = B.gemm_cout(case), (B.gemm_cout(case) + 31) // 32 * 32, B.k_pad(case)
    assert (pk.cin, pk.cout, pk.cin_pad, pk.k_pad, pk.cout_pad) == (case.cin, cout, B.cin_pad(case), kp, cout_pad)
    assert pk.precision == _lib.PRECISIONS[prec] and pk.cout_ps == (case.cout if case.deconv else 0)
    assert pk.wgt.dtype == torch.bfloat16 and pk.wgt.shape == (cout_pad, kp) and pk.wgt.is_contiguous()
    h, l = B.split(data.w)
    as_conv = _deconv_as_conv if case.deconv else (lambda t: t)
    assert torch.equal(pk.wgt.float(), _expected_matrix(as_conv(h), cout_pad, kp))
    k = pk.kh * pk.kw * pk.cin_pad
    assert k <= kp and not pk.wgt[cout:].count_nonzero() and not pk.wgt[:, k:].count_nonzero()      # rows beyond cout, columns beyond K
    if prec == "bf16x3":
        assert pk.wgt_lo.dtype == torch.bfloat16 and pk.wgt_lo.shape == (cout_pad, kp) and pk.wgt_lo.is_contiguous()
        assert torch.equal(pk.wgt_lo.float(), _expected_matrix(as_conv(l), cout_pad, kp))
        assert not pk.wgt_lo[cout:].count_nonzero() and not pk.wgt_lo[:, k:].count_nonzero()
    else:
        assert pk.wgt_lo is None
    want_b = data.b.repeat(4) if case.deconv else data.b
    assert torch.equal(pk.bias[:cout], want_b) and not pk.bias[cout:].count_nonzero()
