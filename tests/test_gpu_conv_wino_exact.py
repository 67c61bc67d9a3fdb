"""Every Winograd kernel (csrc/conv_wino_f32.hip, csrc/conv_wino4_f32.hip: 24 kernels and the kept-slab entry), launched directly at
the smallest shapes at which its mechanisms engage, and held to an exact answer -- what ops.rule_choice and the shipped tune table
pick for most 3x3 stride-1 layers.

The cases and the reasoning are tests/conv_wino_cases.py; tests/test_cpu_conv_wino_cases.py proves its premises without a GPU.

(a) On lattice inputs neither transform, no partial sum of a component GEMM and no step of the output transform needs rounding, so
    every block of every family has to return the float64 value of conv + bias + residual bit for bit: torch.equal, no tolerance.
(b) The kept-slab entry on a DenseNet block in miniature: each layer exact, the second bit-identical to a self-contained launch.
(c) The blocks of a family are order-neutral (what ops.numerics_key says and ops.autotune times across), on Gaussian data with full
    mantissas.
(d) On the same Gaussian data the error stays inside a derived bound, element by element.
(e) What a family cannot run is refused with a message and nothing is written.

Measured on the MI355X: the 16 tests of this file take 2.8 s together (the first 0.6 s, every other id under 0.1 s); largest
error / bound of (d): hint 2 0.0035, hint 3 0.0028, hint 4 0.0017.

Mutations, each made by hand in a scratch copy of the sources, none touching an address, a bound or a barrier; ids of (a) that failed
on the MI355X, and what tests/test_gpu_conv_wino.py (25 tests) said of the same library:
  mfma_rows of the F(4x4) 16-deep loop without its .w MFMA                 -> exactly the 4 hint4 ids; there 13 failures (all of
                                                                              test_winograd_4x4_matches_torch and ..._4x4_on_atrous_layers_...)
  the slab-free kernel's lstore selecting by `kok = ... < p.k_pad`         -> none of the 12 ids, and there all 25 passed: an equivalent
                                                                              mutant.  gload clamps the channel of a request past cin_pad to 0,
                                                                              so what the select lets through is finite data of the window, and
                                                                              it meets the zeros pack_winograd puts behind cin.  The select
                                                                              matters only to a non-finite value, which the clamp keeps away.
  at6's s[1] = d12 - 2 d34 (one sign)                                      -> exactly the 4 hint4 ids; there the same 13 failures

Found while the cases were checked against the code, before anything ran: with Kp = 16 (atrous-4-small) the 32-deep blocks of the
slab-free kernel requested weights at row + j4 for j4 in [16, 32), up to 64 bytes behind the last row of the last filter transform
(the value was discarded).  gload now sends such a request to the start of the row.
"""
import pytest
import torch

import conv_wino_cases as B
from conv_exact_device import SENTINEL, DeviceLayer, bits, check_workspace, difference, ops as _ops, sentinel_bits

pytestmark = pytest.mark.gpu

BLOCK_IDS = [f"hint{h}-block{b}" for h, b in B.BLOCKS]


def _act(ops, case):
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}[case.act]


class _Layer(DeviceLayer):
    """The K padding of c20-n136 reaches from the window into the sentinels behind it.  stride > 1: a layer no family takes, with the
    output it would have and no residual."""
    table = B

    def __init__(self, case, data, stride=1):
        ho, wo = B.out_extent(case)
        if stride > 1:
            ho, wo, data = (ho - 1) // stride + 1, (wo - 1) // stride + 1, data._replace(res=None)
        super().__init__(case, data, stride=stride, out_hw=(ho, wo))

    def pack(self, ops, data):
        pk = ops.pack_conv(data.w, data.b, wino4_min_c=B.WINO4_MIN_C)
        assert pk.wgt_wino is not None and (pk.wgt_wino4 is not None) == B.takes(self.case, 4)
        assert tuple(pk.wgt_wino.shape) == (16, B.cout_pad(self.case), B.kp(self.case))
        return pk

    def check_desc(self, _lib, ops, d):
        case = self.case
        d.split_k = -1
        assert d.precision == _lib.PRECISIONS["fp32"] and (d.cin_pad, d.cout, d.cout_pad) == (B.cin_pad(case), case.cout, B.cout_pad(case))
        wide = d.out_ps % 4 == 0 and d.out % 16 == 0 and (not d.res or (d.res_ps % 4 == 0 and d.res % 16 == 0)) and (d.bias or 0) % 16 == 0
        assert wide == B.wide_ok(case), case.id                     # the epilogue the case table counts on

    def run(self, hint, stage_k):
        """One launch.  The library's workspace query and the launch have to agree with the case table: the query returns the table's
        figure, the launch accepts exactly that many bytes, writes every word of them and none behind; hint 3 asks for none."""
        need = self.configure(hint, stage_k)
        assert need == B.workspace_need(self.case, hint, stage_k), (self.case.id, hint, stage_k, need)
        assert (need == 0) == (hint == 3)
        return self.launch(f"hint {hint} stage_k {stage_k}")


@pytest.mark.parametrize("block", B.BLOCKS, ids=BLOCK_IDS)
def test_every_block_is_exact_on_lattice_inputs(block):
    hint, stage_k = block
    wrong, ran = [], []
    for case in B.CASES:
        if not B.takes(case, hint):
            continue
        ref = B.expected(case).float()
        got = _Layer(case, B.inputs(case)).run(hint, stage_k)
        assert got.shape == ref.shape
        ran.append(case.id)
        if not torch.equal(got, ref):
            wrong.append(difference(case.id, f"hint {hint} stage_k {stage_k}", got, ref))
    assert len(ran) == (6 if hint == 2 else 8)
    assert not wrong, wrong                  # (case, launch, elements that differ, the first of them, largest difference)


def test_kept_slab_of_a_dense_block_is_exact_layer_by_layer():
    """premvos_conv_wino4_slab_f32 on a concat buffer of 112 channels, planned by ops.wino4_slab_plan on a NaN-filled slab.  Layer 0
    transforms its whole window; its output window is then overwritten with fresh lattice data, as if it had produced it, and layer 1
    transforms only those 32 channels and reuses the slab for the rest.  Each layer is exact, with every GEMM block; layer 1 is
    bit-identical to a self-contained hint-4 launch on the same buffer."""
    _lib, lib, ops = _ops()
    c0, c1 = B.DENSE
    d0_data, d1_data = B.inputs(c0), B.inputs(c1)
    sent = sentinel_bits()
    for stage_k in B.HINTS[4]:
        buf = torch.full((c0.n, c0.h, c0.w, B.DENSE_PS), SENTINEL)
        buf[..., 64:] = d0_data.x.permute(0, 2, 3, 1)
        X = ops.NHWC(buf.cuda())
        layers = []
        for case, data in ((c0, d0_data), (c1, d1_data)):
            pk = ops.pack_conv(data.w, data.b, wino4_min_c=B.WINO4_MIN_C)
            assert pk.wgt_wino4 is not None
            d = ops.conv_desc(X.slice(case.win_in[1], case.cin), pk, X.slice(case.win_out[1], case.cout), pad=case.pad,
                              act=_act(ops, case), slope=B.SLOPE, tile_hint=4, stage_k=stage_k)
            d.split_k = -1
            layers.append((d, case.win_in[1], pk))                 # (pk: the packed weights stay alive)
        need, plan = ops.wino4_slab_plan([(d, off) for d, off, _ in layers])
        assert need == 36 * B.tiles(c0, 4) * B.DENSE_PS and [p[1:] for p in plan] == B.DENSE_PLAN
        slab = torch.full((need + 64,), float("nan"), device="cuda")
        rows = slab[:need].view(36 * B.tiles(c0, 4), B.DENSE_PS)

        def run(i, case):
            d, pitch, v_c0, t_cn = plan[i]
            words = B.m_slab_need(case, stage_k) // 4
            ms = torch.full((words + 64,), float("nan"), device="cuda")
            d.workspace, d.workspace_bytes = ms.data_ptr(), words * 4          # exactly the M slab
            before = X.buf.clone()
            ops.run_wino4_slab(d, slab[:need], pitch, v_c0, t_cn)
            torch.cuda.synchronize()
            check_workspace(f"{case.id} stage_k {stage_k}", ms.cpu(), words)
            lo = case.win_out[1]
            after = X.buf.clone()
            after[..., lo:lo + case.cout] = before[..., lo:lo + case.cout]
            assert torch.equal(bits(after), bits(before)), f"{case.id}: written outside the output window"
            return X.buf[..., lo:lo + case.cout].permute(0, 3, 1, 2).contiguous().cpu()

        got0 = run(0, c0)
        assert torch.equal(got0, B.expected(c0).float()), difference(c0.id, stage_k, got0, B.expected(c0).float())
        finite = torch.isfinite(rows).cpu()
        assert finite[:, 64:].all() and not finite[:, :64].any() and torch.isnan(slab[need:]).all()      # only its window of the slab
        X.buf[..., 32:64] = d1_data.x[:, :32].permute(0, 2, 3, 1).cuda()
        assert torch.all(bits(X.buf[..., :32]) == sent)
        got1 = run(1, c1)
        assert torch.equal(got1, B.expected(c1).float()), difference(c1.id, stage_k, got1, B.expected(c1).float())
        finite = torch.isfinite(rows).cpu()
        assert finite[:, 32:].all() and not finite[:, :32].any() and torch.isnan(slab[need:]).all()
        # the same layer self-contained: its own V slab, all 80 channels transformed again
        d1 = layers[1][0]
        full = ops.workspace_bytes(d1)
        assert full == B.workspace_need(c1, 4, stage_k)
        ws = torch.full((full // 4 + 64,), float("nan"), device="cuda")
        d1.workspace, d1.workspace_bytes = ws.data_ptr(), full
        X.buf[..., :32] = SENTINEL
        ops.run_desc(d1)
        torch.cuda.synchronize()
        alone = X.buf[..., :32].permute(0, 3, 1, 2).contiguous().cpu()
        assert torch.equal(bits(alone), bits(got1)), stage_k


def _gaussian_layers():
    return [_Layer(B.BY_ID[i], B.gaussian_inputs(B.BY_ID[i])) for i in B.GAUSSIAN]


def test_blocks_of_a_family_are_bit_identical():
    """Everything the tuner may time against each other (same ops.numerics_key) writes the same bits: the two row counts of hint 2,
    the six blocks of hint 3, the four of hint 4 -- also the blocks ops._candidates does not offer to the layer's cout (hint 3 to
    cout <= 32, 64-column blocks to wide layers and 128-column blocks to narrow ones), added by hand."""
    _lib, lib, ops = _ops()
    for layer in _gaussian_layers():
        d, case = layer.d, layer.case
        by_hand = [(h, b, -1, 0, 0) for h, b in B.BLOCKS if B.takes(case, h)]
        offered = [c for c in ops._candidates(d) + [ops.rule_choice(d)] if c[0] in (2, 3, 4)]
        assert set(offered) <= set(by_hand)
        groups = {}
        for c in by_hand:
            groups.setdefault(ops.numerics_key(d, c), []).append(c)
        assert sorted(groups) == [(h,) for h in B.HINTS if B.takes(case, h)]
        for key, members in groups.items():
            assert len(members) == len(B.HINTS[key[0]])
            ref = None
            for hint, stage_k, *_ in members:
                got = layer.run(hint, stage_k)
                assert torch.isfinite(got).all()
                if ref is None:
                    ref = got
                assert torch.equal(bits(got), bits(ref)), (case.id, key, members[0][:2], (hint, stage_k))


def test_gaussian_inputs_stay_inside_the_derived_bound():
    """Derived, not measured from the kernel; it holds element by element:
        |got - true| <= (Kp + T + 2) * 2^-23 * S_w,    S_w = |A^T| (sum_k V_abs * U_abs) |A| + |b| + |res|,
    the first-order bound of a float32 evaluation in which every term of an output element passes T roundings in the transforms
    (counted in the code: conv_wino_cases.ROUNDINGS, 7 / 12 / 13 for hints 2 / 3 / 4), the Kp accumulations of its component GEMM, and the
    additions of bias and residual; 2^-23 is twice the unit roundoff, which covers an MFMA accumulate that truncates instead of
    rounding to nearest.  The first accumulation, to a zero accumulator, is exact, which leaves room for the one rounding of leaky
    ReLU's multiply; ReLU and leaky ReLU are 1-Lipschitz and keep the bound.  The bound is loose;
    test_every_block_is_exact_on_lattice_inputs is the sharp test."""
    worst = {}
    for layer in _gaussian_layers():
        case = layer.case
        data = B.gaussian_inputs(case)
        true = B.true_conv(case, data)
        scale = {m: B.bound_scale(case, data, m) for m in (2, 4)}
        assert min(s.min().item() for s in scale.values()) > 0
        for hint, stage_k in B.BLOCKS:
            if not B.takes(case, hint):
                continue
            s_w = scale[B.FAMILY[hint]]
            bound = (B.kp(case) + B.ROUNDINGS[hint] + 2) * 2.0 ** -23 * s_w
            got = layer.run(hint, stage_k).double()
            ratio = ((got - true).abs() / bound).max().item()
            worst[hint] = max(worst.get(hint, 0.0), ratio)
            assert ratio <= 1, (case.id, hint, stage_k, ratio)
    print("Winograd: largest error / bound = " + ", ".join(f"hint {h}: {r:.4f}" for h, r in sorted(worst.items())))


def test_winograd_paths_refuse_what_they_cannot_run():
    _lib, lib, ops = _ops()
    stream = _lib.current_stream()
    # hint 2 on an atrous layer
    atrous = _Layer(B.BY_ID["atrous-2"], B.inputs(B.BY_ID["atrous-2"]))
    atrous.d.tile_hint, atrous.d.stage_k = 2, 0
    assert ops.workspace_bytes(atrous.d) == 0 and "Winograd needs a 3x3 / stride 1 / dilation 1" in atrous.refused(lib, stream)
    # stride 2
    strided = _Layer(B.BY_ID["c20-n136"], B.inputs(B.BY_ID["c20-n136"]), stride=2)
    for hint, what in ((2, "Winograd needs a 3x3 / stride 1 / dilation 1"), (3, "Winograd needs a 3x3 / stride 1 fp32"), (4, "Winograd F(4x4,3x3) needs")):
        strided.d.tile_hint, strided.d.stage_k = hint, 0
        assert ops.workspace_bytes(strided.d) == 0 and what in strided.refused(lib, stream), hint
    # block ids that do not exist
    layer = _Layer(B.BY_ID["pad-2-0"], B.inputs(B.BY_ID["pad-2-0"]))
    for stage_k in (1, 7, 16, 32, 64, -1):
        layer.configure(3, stage_k)
        assert f"stage_k {stage_k} is not a block id (0, 2..6)" in layer.refused(lib, stream)
    for stage_k in (1, 2, 32, 48, 96, 128, -1):
        assert layer.configure(4, stage_k) > 0
        assert f"stage_k {stage_k} is not a block id (0, 16, 64, 80)" in layer.refused(lib, stream)
        assert torch.isnan(layer.ws).all()
    # hint 4 without F(4x4) filter transforms
    layer.configure(4, 0)
    kept, layer.d.wgt_wino4 = layer.d.wgt_wino4, None
    assert ops.workspace_bytes(layer.d) == 0 and "packed filter transforms (wgt_wino4)" in layer.refused(lib, stream)
    assert torch.isnan(layer.ws).all()
    layer.d.wgt_wino4 = kept
    # no workspace, one 4 bytes short, one claimed but absent
    for case_id in ("c20-n136", "pad-2-0"):
        starved = _Layer(B.BY_ID[case_id], B.inputs(B.BY_ID[case_id]))
        for hint, stage_k in ((2, 0), (2, 64), (4, 0), (4, 80)):
            need = starved.configure(hint, stage_k)
            assert need == B.workspace_need(starved.case, hint, stage_k) > 0
            for ptr, size in ((None, 0), (starved.ws.data_ptr(), need - 4), (None, need)):
                starved.d.workspace, starved.d.workspace_bytes = ptr, size
                msg = starved.refused(lib, stream)
                assert "conv2d(winograd" in msg and f"needs {need} workspace bytes" in msg, msg
            assert torch.isnan(starved.ws).all()                                   # ... and no slab was written either
