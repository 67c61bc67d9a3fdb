"""Every instance of the fp32 implicit GEMM (csrc/conv_igemm_f32.hip), launched directly: 9 tiles at 16-deep stages, four of them at
32-deep stages too, each as {plain, plain-PW, split-K, split-K-PW, pixel-shuffle} = 65 kernels, plus both forms of the split-K reduce
-- the default arithmetic of all four networks, and what most of the shipped tune table points at.

The cases and the reasoning are tests/conv_f32_cases.py; tests/test_cpu_conv_f32_cases.py proves its premises without a GPU.

(a) On lattice inputs no partial sum of an output element needs rounding, so every instance has to return the float64 value of
    conv + bias + residual bit for bit: torch.equal, no tolerance.  One product dropped or doubled changes the value by at least 2^-8.
(b) The kernels that promise the same products (hints 1, 5, 6) are exact on the same data.
(c) Tile and stage depth are order-neutral (what ops.numerics_key says and ops.autotune times across), on Gaussian data with full
    mantissas; so are they under a fixed k-slicing and a fixed tail split.
(d) On the same Gaussian data the error stays inside a derived bound, element by element.
(e) What the kernel cannot run is refused with a message and nothing is written.

Mutations (a) is meant to catch, each made by hand in a scratch copy of conv_igemm_f32.hip, none touching an address, a bound or a
barrier; ids of (a) that failed on the MI355X, and what test_gpu_flow_kernels.py (82 tests) said of the same library:
  k_loop's `compute` (the 32-deep stages' loop) without the .w MFMA     -> exactly the 4 kb32 ids; there 1 failure (test_conv2d_tail_split[case0])
  h_last rounded down, (kreal - (KT_all - 1) * KB) / 8 without the + 7   -> all 13 ids, through tail-k3 alone at 16-deep stages (kreal 108 = 6 * 16
                                                                            + 12: the second group of the last stage is half real); there all 82 passed
  the after-barrier mfma_rows((H - 1) & 1, MT - 1, MT) reading set 0     -> exactly the 9 kb16 ids; there 51 failures
"""
import pytest
import torch

import conv_f32_cases as B
from conv_exact_device import DeviceLayer, bits, difference, ops as _ops, tile_hint

pytestmark = pytest.mark.gpu

PAIR_IDS = [f"{t[0]}x{t[1]}-kb{st}" for t, st in B.PAIRS]


class _Layer(DeviceLayer):
    table = B

    def pack(self, ops, data):
        return (ops.pack_deconv4x4s2 if self.case.deconv else ops.pack_conv)(data.w, data.b)

    def check_desc(self, _lib, ops, d):
        case = self.case
        assert (d.out_mode == ops.OUT_PIXSHUF2) == case.deconv and d.precision == _lib.PRECISIONS["fp32"]
        assert (d.k_pad, d.cin_pad, d.cout, d.cout_pad) == (B.k_pad(case), B.cin_pad(case), B.gemm_cout(case), B.cout_pad(case))
        assert (d.ho, d.wo) == B.gemm_extent(case)
        wide = d.cout % 4 == 0 and d.out_ps % 4 == 0 and d.out % 16 == 0 and (not d.res or (d.res_ps % 4 == 0 and d.res % 16 == 0)) \
            and (d.bias or 0) % 16 == 0
        assert case.deconv or wide == B.wide_ok(case), case.id      # the epilogue the case table counts on

    def run(self, tile, stage, launch):
        """One launch of the implicit GEMM.  The library's workspace query and the launch have to agree with the case table on the
        k-slicing of this (tile, stage): the query returns the table's figure, the launch accepts exactly that many bytes, writes
        every word of them and none behind."""
        need = self.configure(tile_hint(tile), stage, launch.split_k, launch.tail)
        assert need == B.workspace_need(self.case, tile, stage, launch), (self.case.id, launch.name, need)
        return self.launch(launch.name)


@pytest.mark.parametrize("pair", B.PAIRS, ids=PAIR_IDS)
def test_every_instance_is_exact_on_lattice_inputs(pair):
    tile, stage = pair
    wrong = []
    for case in B.CASES:
        ref = B.expected(case)[0].float()
        layer = _Layer(case, B.inputs(case))
        for launch in B.launches(case):
            got = layer.run(tile, stage, launch)
            assert got.shape == ref.shape
            if not torch.equal(got, ref):
                wrong.append(difference(case.id, launch.name, got, ref))
    assert not wrong, wrong                  # (case, launch, elements that differ, the first of them, largest difference)


def test_same_products_kernels_are_exact_on_lattice_inputs():
    """Hint 1 (the direct kernel for two-channel heads, tiled and -- stage_k 1 -- per pixel), hint 5 (streaming pointwise) and hint 6
    (LDS-DMA pointwise) add the products of the implicit GEMM, hints 5 and 6 in its order: exact where it is exact."""
    _lib, lib, ops = _ops()
    wrong, ran = [], set()
    for case in B.CASES:
        if not case.hints:
            continue
        ref = B.expected(case)[0].float()
        layer = _Layer(case, B.inputs(case))
        d = layer.d
        for hint, stage in case.hints:
            d.tile_hint, d.stage_k = hint, stage
            assert {1: d.cout <= 2, 5: ops.stream_applicable(d), 6: ops.pwdma_applicable(d)}[hint], (case.id, hint)
            got = layer.run_hint(hint, stage)
            ran.add((hint, stage))
            if not torch.equal(got, ref):
                wrong.append(difference(case.id, f"hint {hint} stage_k {stage}", got, ref))
    assert ran == {(1, 0), (1, 1), (5, 0), (6, 0)}
    assert not wrong, wrong


def _gaussian_layers():
    return [_Layer(B.BY_ID[i], B.gaussian_inputs(B.BY_ID[i])) for i in B.GAUSSIAN]


def test_order_neutral_knobs_are_bit_identical():
    """The construction of test_gpu_tune.py::test_order_neutral_knobs_are_bit_identical with all 13 (tile, stage) pairs added by hand
    (the candidate list goes by cout and offers 256x128 / 256x129 only to maps of 131072 / 16384 pixels and more): everything the tuner
    may time against each other (same ops.numerics_key) writes the same bits.  The pairs are also added under the case's own k-slicing
    and tail split, where the key tells apart what does change the order: the stages per slice, the rows the tail covers."""
    _lib, lib, ops = _ops()
    for layer in _gaussian_layers():
        d, case = layer.d, layer.case
        plain = [(tile_hint(t), st, -1, 0, 0) for t, st in B.PAIRS]
        sliced = [(tile_hint(t), st, l.split_k) + l.tail for t, st in B.PAIRS for l in B.launches(case)[1:]]
        cands = list(dict.fromkeys(ops._candidates(d) + [ops.rule_choice(d)] + plain + sliced))
        groups = {}
        for c in cands:
            groups.setdefault(ops.numerics_key(d, c), []).append(c)
        assert len({ops.numerics_key(d, c) for c in plain}) == 1 and set(plain) <= set(groups[ops.numerics_key(d, plain[0])])
        if case.id in ("pw-c728", "pw-s2-c200"):
            assert (6, 0, -1, 0, 0) in groups[ops.numerics_key(d, plain[0])]       # the LDS-DMA kernel is timed against the tiles
        if sliced:
            assert len(groups) > 1
        for key, members in groups.items():
            ref = None
            for hint, st, sk, tail_rows, ts in members:
                layer.configure(hint, st, sk, (tail_rows, ts))
                got = layer.launch()
                assert torch.isfinite(got).all()
                if ref is None:
                    ref = got
                assert torch.equal(bits(got), bits(ref)), (case.id, key, members[0], (hint, st, sk, tail_rows, ts))


def _slices_per_element(case, tile, stage, launch):
    """The number of k-slices behind each output element (0 = unsplit), shaped to broadcast against the NCHW output."""
    mb = B.m_begin(case, tile, launch)
    ho, wo = B.gemm_extent(case)
    per_row = torch.zeros(B.gemm_rows(case), dtype=torch.float64)
    if mb is not None:
        per_row[mb:] = B.slices(case, stage, launch.split_k if launch.split_k > 1 else launch.tail[1])[1]
    s = per_row.view(case.n, 1, ho, wo)
    return s.repeat_interleave(2, 2).repeat_interleave(2, 3) if case.deconv else s


def test_gaussian_inputs_stay_inside_the_derived_bound():
    """Derived, not measured from the kernel; it holds element by element:
        |got - true| <= (k_pad + slices + 2) * 2^-23 * S_true,    S_true = conv(|x|, |w|) + |b| + |res|,
    the first-order bound of a float32 sum of that many terms in any order (k_pad products, the `slices` slab sums of a k-sliced
    element, bias, residual); 2^-23 is twice the unit roundoff, which covers an MFMA accumulate that truncates instead of rounding to
    nearest.  The first addition, to a zero accumulator, is exact, which leaves room for the one rounding of leaky ReLU's multiply;
    ReLU and leaky ReLU are 1-Lipschitz and keep the bound.  The bound is loose at long k;
    test_every_instance_is_exact_on_lattice_inputs is the sharp test."""
    worst = 0.0
    for layer in _gaussian_layers():
        case = layer.case
        true, s_true = B.true_conv(case, B.gaussian_inputs(case))
        assert s_true.min().item() > 0
        for tile, stage in B.PAIRS:
            for launch in B.launches(case):
                bound = (B.k_pad(case) + _slices_per_element(case, tile, stage, launch) + 2) * 2.0 ** -23 * s_true
                got = layer.run(tile, stage, launch).double()
                ratio = ((got - true).abs() / bound).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1, (case.id, tile, stage, launch.name, ratio)
    print(f"fp32 implicit GEMM: largest error / bound = {worst:.4f}")


def test_fp32_path_refuses_what_it_cannot_run():
    _lib, lib, ops = _ops()
    stream = _lib.current_stream()
    layer = _Layer(B.BY_ID["k3-c20"], B.inputs(B.BY_ID["k3-c20"]))
    for hint in (7, tile_hint((64, 96)), tile_hint((256, 64)), tile_hint((128, 129)), tile_hint((32, 32)), tile_hint((256, 256))):
        for stage in (16, 32):
            layer.configure(hint, stage, -1)
            assert "no tile config" in layer.refused(lib, stream), hint
    for case_id, split_k, tail, what in (("pw-c728", 4, (0, 0), "split_k=4 needs"), ("tail-pw", -1, (1, 3), "tail split 1x3 needs"),
                                         ("tail-deconv", -1, (1, 3), "tail split 1x3 needs")):
        sliced = _Layer(B.BY_ID[case_id], B.inputs(B.BY_ID[case_id]))
        for tile, stage in (((64, 64), 16), ((128, 128), 32), ((256, 129), 16)):
            need = sliced.configure(tile_hint(tile), stage, split_k, tail)
            assert need > 0
            for ptr, size in ((None, 0), (sliced.ws.data_ptr(), need - 4), (None, need)):      # none, too small, claimed but absent
                sliced.d.workspace, sliced.d.workspace_bytes = ptr, size
                msg = sliced.refused(lib, stream)
                assert what in msg and f"{need} workspace bytes" in msg, msg
            assert torch.isnan(sliced.ws).all()                                    # ... and no slab was written either
