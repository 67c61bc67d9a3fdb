"""Every instance of the bf16 / bf16x3 implicit GEMM (csrc/conv_igemm_bf16.hip), launched directly: 6 tiles x 2 stage depths x NPASS 1 / 3
x {plain, pixel-shuffle, split-K} = 72 kernels, any of which the plan-time tuner may put into a production plan of the bf16 modes.

The cases and the reasoning are tests/conv_bf16_cases.py; tests/test_cpu_conv_bf16_cases.py proves its premises without a GPU.

(a) On lattice inputs no partial sum of an output element needs rounding, so the kernel has to return the float64 value of
    sum hi hi (+ hi lo + lo hi) + bias + residual bit for bit: torch.equal, no tolerance.  That also pins down WHICH product terms are
    added: dropping one, or splitting an activation differently, changes the value by far more than one bit.
(b) Tile and stage depth are order-neutral in these modes too (what ops.numerics_key says and ops.autotune times across), on Gaussian
    data with full mantissas.
(c) On the same Gaussian data the error stays inside two derived bounds, against the emulated split products and against the true
    convolution.
(d) What the kernel cannot run is refused with a message and nothing is written.

Mutations (a) is meant to catch, each made by hand in a scratch copy of conv_igemm_bf16.hip, none touching an address, a bound or a
barrier; ids of (a) that failed on the MI355X:
  the FRAG_PF loop's mfma_rows without the ah * bl product            -> exactly the 6 bf16x3 ids with stage 32
  lstore computing lo from v instead of v - hi                         -> all 12 bf16x3 ids
  the after-barrier mfma_rows((S - 1) & 1, MT - 1, MT) reading set 0   -> exactly the 6 bf16x3 ids with stage 32
test_gpu_precision_modes.py::test_conv_precision_modes passes under the first and the third: it never launches that loop.
"""
import pytest
import torch

import conv_bf16_cases as B
from conv_exact_device import DeviceLayer, bits, difference, ops as _ops, tile_hint

pytestmark = pytest.mark.gpu

TILE_IDS = [f"{bm}x{bn}" for bm, bn in B.TILES]


class _Layer(DeviceLayer):
    table = B

    def __init__(self, case, prec, data):
        self.prec = prec
        super().__init__(case, data)

    def pack(self, ops, data):
        return (ops.pack_deconv4x4s2 if self.case.deconv else ops.pack_conv)(data.w, data.b, precision=self.prec)

    def check_desc(self, _lib, ops, d):
        assert (d.out_mode == ops.OUT_PIXSHUF2) == self.case.deconv and d.k_pad == B.k_pad(self.case)
        assert (d.ho, d.wo) == B.gemm_extent(self.case)

    def run(self, tile, stage, split_k=-1):
        need = self.configure(tile_hint(tile), stage, split_k)
        assert (need > 0) == (split_k > 1), (self.case.id, need)    # the split-K instance really is what runs
        return self.launch(f"split_k {split_k}")


@pytest.mark.parametrize("stage", B.STAGES)
@pytest.mark.parametrize("tile", B.TILES, ids=TILE_IDS)
@pytest.mark.parametrize("prec", B.PRECISIONS)
def test_every_instance_is_exact_on_lattice_inputs(prec, tile, stage):
    wrong = []
    for case in B.CASES:
        ref, _ = B.expected(case, prec)
        ref = ref.float()
        layer = _Layer(case, prec, B.inputs(case))
        for form, sk in B.launches(case):
            got = layer.run(tile, stage, sk)
            assert got.shape == ref.shape
            if not torch.equal(got, ref):
                wrong.append(difference(case.id, form, got, ref))
    assert not wrong, wrong                  # (case, form, elements that differ, the first of them, largest difference)


def _gaussian_layers(prec):
    return [_Layer(B.BY_ID[i], prec, B.gaussian_inputs(B.BY_ID[i])) for i in B.GAUSSIAN]


@pytest.mark.parametrize("prec", B.PRECISIONS)
def test_order_neutral_knobs_are_bit_identical_in_the_bf16_modes(prec):
    """The construction of test_gpu_tune.py::test_order_neutral_knobs_are_bit_identical, for the modes that file leaves out: everything
    the tuner may time against each other (same ops.numerics_key) writes the same bits.  Tiles the candidate list does not offer for a
    shape (it goes by cout) are added by hand, so all 12 (tile, stage) pairs are compared on every layer."""
    _lib, lib, ops = _ops()
    plain = [(tile_hint(t), st, -1, 0, 0) for t in B.TILES for st in B.STAGES]
    for layer in _gaussian_layers(prec):
        d = layer.d
        cands = list(dict.fromkeys(ops._candidates(d) + [ops.rule_choice(d)] + plain))
        groups = {}
        for c in cands:
            groups.setdefault(ops.numerics_key(d, c), []).append(c)
        assert len({ops.numerics_key(d, c) for c in plain}) == 1 and set(plain) <= set(groups[ops.numerics_key(d, plain[0])])
        if layer.case.id == "pw-c728":
            assert len(groups) > 1           # k_pad 736: k-slices are offered, and their keys differ with the stage depth
        for key, members in groups.items():
            ref = None
            for hint, st, sk, _, _ in members:
                layer.configure(hint, st, sk)
                got = layer.launch()
                assert torch.isfinite(got).all()
                if ref is None:
                    ref = got
                assert torch.equal(bits(got), bits(ref)), (layer.case.id, key, members[0], (hint, st, sk))


@pytest.mark.parametrize("prec", B.PRECISIONS)
def test_gaussian_inputs_stay_inside_the_derived_bound(prec):
    """Both bounds are derived, neither is measured from the kernel; they hold element by element.

    Emulated sum: against the float64 sum of the split products the kernel is specified to add (+ bias + residual),
        |got - emu| <= n_add * 2^-23 * S_abs,    n_add = NPASS * k_pad + 2,
    the first-order bound of a float32 sum of n_add terms in any order; 2^-23 is twice the unit roundoff, which covers an MFMA
    accumulate that truncates instead of rounding to nearest.  The first addition, to a zero accumulator, is exact, which leaves room
    for the one rounding of leaky ReLU's multiply; ReLU and leaky ReLU are 1-Lipschitz and keep the bound.
    True convolution: the same plus the algorithmic term c * S_true, S_true = conv(|x|, |w|) + |b| + |res|, c = 2^-8 + 2^-16 for bf16
    (two operand roundings) and 2^-16 for bf16x3 (lo * lo and the two residues of rounding lo).
    The bounds are loose at long k; test_every_instance_is_exact_on_lattice_inputs is the sharp test."""
    c_prec = {"bf16": 2.0 ** -8 + 2.0 ** -16, "bf16x3": 2.0 ** -16}[prec]
    worst_emu, worst_true = 0.0, 0.0
    for layer in _gaussian_layers(prec):
        case = layer.case
        data = B.gaussian_inputs(case)
        pre, s_abs = B.product_sum(case, prec, data)
        emu = B.activate(case, pre)
        true, s_true = B.true_conv(case, data)
        bound_emu = (B.NPASS[prec] * B.k_pad(case) + 2) * 2.0 ** -23 * s_abs
        bound_true = bound_emu + c_prec * s_true
        assert bound_emu.min().item() > 0
        for tile in B.TILES:
            for stage in B.STAGES:
                got = layer.run(tile, stage).double()
                r_emu = ((got - emu).abs() / bound_emu).max().item()
                r_true = ((got - true).abs() / bound_true).max().item()
                worst_emu, worst_true = max(worst_emu, r_emu), max(worst_true, r_true)
                assert r_emu <= 1 and r_true <= 1, (case.id, tile, stage, r_emu, r_true)
    print(f"{prec}: largest error / bound = {worst_emu:.4f} against the emulated products, {worst_true:.4f} against the true convolution")


@pytest.mark.parametrize("prec", B.PRECISIONS)
def test_bf16_modes_refuse_what_they_cannot_run(prec):
    _lib, lib, ops = _ops()
    stream = _lib.current_stream()
    layer = _Layer(B.BY_ID["k3-c20"], prec, B.inputs(B.BY_ID["k3-c20"]))
    for hint in (1, 2, 3, 4, 5, 6, (256 << 16) | 128, (128 << 16) | 96):       # the fp32 path's other kernels and tiles
        for stage in B.STAGES:
            layer.configure(hint, stage, -1)
            assert "no tile config" in layer.refused(lib, stream), hint
    long_k = _Layer(B.BY_ID["pw-c728"], prec, B.inputs(B.BY_ID["pw-c728"]))
    long_k.configure(tile_hint((64, 64)), 16, 4)
    long_k.d.workspace, long_k.d.workspace_bytes = None, 0
    assert "workspace bytes" in long_k.refused(lib, stream)
    long_k.d.workspace, long_k.d.workspace_bytes = long_k.ws.data_ptr(), 16    # ... or with one that is too small
    assert "workspace bytes" in long_k.refused(lib, stream)
    if prec == "bf16x3":
        layer.configure(tile_hint((64, 64)), 16, -1)
        layer.d.wgt_lo = None
        assert "wgt_lo" in layer.refused(lib, stream)
