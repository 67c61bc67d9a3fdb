"""Every kernel of csrc/conv_bf16x3_s8.hip, launched directly: the LDS-DMA implicit GEMM on the resident split layout S8 (12 tile
configurations x {pointwise, general} instantiation), the ping-pong pointwise kernel and split8_kernel.  In bf16x3 mode they carry
every bottleneck conv of the proposal net from group 1 on and every long-K pointwise conv of the refinement net.

The cases and the reasoning are tests/conv_s8_cases.py; tests/test_cpu_conv_s8_cases.py proves its premises without a GPU.
tests/test_gpu_conv_s8.py checks the same kernels at production-like shapes to 3e-5 of the largest output, one number per case.

(a) On lattice inputs no partial sum of an output element needs rounding, so the fp32 output has to be the float64 value of
    sum(lo.hi + hi.lo + hi.hi) + bias + residual bit for bit, and the S8 output the words hi = bf16(v), lo = bf16(v - hi) of it:
    torch.equal, no tolerance.  Inputs, outputs and the S8 residual are channel windows of wider buffers (NaN around what is read,
    a sentinel around what is written), the stage counts include 1, 2 and 3, the work-group counts the ones at which
    xcd_contiguous takes its remainder branch.
(b) split8_kernel against the host encoder: rounding ties, carries into the exponent, +-0, a partial last group, windows.
(c) The tile is order-neutral on Gaussian data with full mantissas: all 12 write the same bits, to both outputs.
(d) On the same Gaussian data the error stays inside two derived bounds, against the emulated split products and against the true
    convolution, element by element.
(e) What the entries cannot run is refused on the host with a message, and nothing is written.  No launch here is built to fault.

Mutations (a) is meant to catch, each made by hand in a scratch copy of conv_bf16x3_s8.hip / common.h, none touching an address, a
bound, a barrier or a wait count; ids that failed on the MI355X, and what the tolerance tests said of the same build (s8 =
test_gpu_conv_s8.py, 98 ids; pm = test_gpu_precision_modes.py, 33 ids).  (c) and (d) stand for the Gaussian tests above.
  1 conv_bf16x3_s8_kernel: the second 16-deep step without term(ah, bl)
      -> (a) exactly the KC-32 tiles 0-5, 9, 10, 11; in each the 9 cases with more than 16 input channels, on tile 10 only the 5 of
         them that are not pointwise: the ping-pong kernel is what runs the others.  (c), (d).    s8: 70 failed.  pm: 7 failed.
  2 conv_bf16x3_s8_pp_kernel without term(ah[1], bl[1])
      -> (a) tile10 alone, and there exactly pw-c64, pw-c96, pw-c40, pw-c728: pingpong(case) and more than 16 input channels.
         (c), (d).    s8: 4 failed (tile 10 on its three pointwise layers, the chain test).  pm: all passed.
  3 the epilogue without join_split8
      -> (a) all 12 tiles, in each exactly pw-c40, pw-c728, atrous: the res = "s8" cases.  (d).
         s8: 1 failed (the chain test, the file's one S8 residual).  pm: 2 failed.
  4 store_split8 rounding the lo half from v instead of v - hi
      -> (a) all 12 tiles, every case, the S8 words of both launch forms and no fp32 output; (b) all three widths; (d).
         s8: 97 failed.  pm: 2 failed.
  5 store_split8 truncating the lo half to bf16 instead of rounding it to nearest even
      -> (a) all 12 tiles, the S8 words of every case but pw-c8; (b) all three widths; (d).    s8: all passed.  pm: all passed.
  6 store_split8 truncating the hi half (lo = bf16(v - hi) still rounded)
      -> (a) all 12 tiles, the S8 words of every case; (b) all three widths; (d).    s8: all passed.  pm: all passed.
The tolerance tests notice the loss of a whole product term (2^-9 relative), though not where: 1 and 2 differ there only in how
many ids fail.  5 and 6 keep hi + lo within 2^-16 of the value and pass both older files; only equality sees them.
"""
import ctypes
import functools

import pytest
import torch

import conv_s8_cases as S
from conv_exact_device import SENTINEL, bits, check_unchanged, extract_window, ops as _ops, sentinel_bits, windowed

pytestmark = pytest.mark.gpu

FORMS = ("f32", "s8", "both")                # the outputs a launch is given


class _Layer:
    """One case on the device: the S8 input inside its channel window of a NaN-filled buffer, packed weights, the residual, and
    sentinel-filled buffers around the two output windows."""

    def __init__(self, case, data):
        _lib, lib, ops = _ops()
        self.case, self.ops = case, ops
        ho, wo = S.out_extent(case)
        ps, off = S.window(case, "in")
        self.xin = windowed(S.encode_s8(S.nhwc(data.x)), ps, off, S.NAN_WORD).view(torch.float32).cuda()
        self.x = ops.NHWC(self.xin, c=case.cin, coff=off, layout="s8")
        self.pk = ops.pack_conv_s8(data.w, data.b)
        self.res, self.res8, self.res_buf = None, None, None
        if case.res == "f32":
            self.res = ops.NHWC.alloc(case.n, ho, wo, case.cout)
            self.res.buf[..., :case.cout] = S.nhwc(data.res).cuda()
            self.res_buf = self.res.buf
        elif case.res == "s8":
            ps, off = S.window(case, "res8")
            self.res_buf = windowed(S.encode_s8(S.nhwc(data.res)), ps, off, S.NAN_WORD).view(torch.float32).cuda()
            self.res8 = ops.NHWC(self.res_buf, c=case.cout, coff=off, layout="s8")
        self.read = [t for t in (self.xin, self.pk.wgt, self.pk.bias, self.res_buf) if t is not None]
        self.before = [t.clone() for t in self.read]
        (ps, self.off), (ps8, self.off8) = S.window(case, "out"), S.window(case, "out8")
        self.out_buf = torch.empty((case.n, ho, wo, ps), device="cuda")
        self.out8_buf = torch.empty((case.n, ho, wo, ps8), device="cuda")
        self.out = ops.NHWC(self.out_buf, c=case.cout, coff=self.off)
        self.out8 = ops.NHWC(self.out8_buf, c=case.cout, coff=self.off8, layout="s8")
        self.act = {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "leaky": ops.ACT_LEAKY}[case.act]

    def desc(self, form):
        c = self.case
        return self.ops.conv_s8_desc(self.x, self.pk, self.out if form != "s8" else None, self.out8 if form != "f32" else None,
                                     stride=(c.stride, c.stride), dilation=(c.dil, c.dil), pad=c.pad[:2], act=self.act, slope=S.SLOPE, res=self.res)

    def run(self, tile, form):
        """-> (fp32 window NHWC or None, S8 window as int32 words NHWC or None), after asserting that nothing around the windows, no
        output the launch was not given and nothing the kernel reads was written."""
        c = self.case
        self.out_buf.fill_(SENTINEL)
        self.out8_buf.fill_(SENTINEL)
        d = self.desc(form)
        assert (d.ho, d.wo) == S.out_extent(c) and d.cout_pad == S.cout_pad(c)
        self.ops.run_s8(d, self.x, self.pk, self.out8 if form != "f32" else None, tile, res_s8=self.res8)
        torch.cuda.synchronize()
        for t, b in zip(self.read, self.before):
            check_unchanged(f"{c.id} tile {tile} {form}", "input, weight or residual buffer", t, b)
        got = []
        for buf, off, given in ((self.out_buf, self.off, form != "s8"), (self.out8_buf, self.off8, form != "f32")):
            lo, width = (off, c.cout) if given else (0, 0)                     # an output the launch was not given: no window at all
            words = extract_window(f"{c.id} tile {tile} {form}", bits(buf.cpu()), lo, width, fill=sentinel_bits())
            got.append(words if given else None)
        return (got[0].view(torch.float32) if got[0] is not None else None), got[1]


@functools.lru_cache(maxsize=None)
def _layer(case_id, gaussian=False):
    """The layers are built once and shared by the tests (they assert after every launch that nothing they read has changed)."""
    case = S.BY_ID[case_id]
    return _Layer(case, S.gaussian_inputs(case) if gaussian else S.inputs(case))


@pytest.mark.parametrize("tile", range(len(S.TILES)), ids=[f"tile{t}" for t in range(len(S.TILES))])
def test_every_instance_is_exact_on_lattice_inputs(tile):
    wrong = []
    for case in S.CASES:
        ref = S.nhwc(S.expected(case)[0].float())
        ref8 = S.encode_s8(ref)
        layer = _layer(case.id)
        words = {}
        for form in FORMS:
            got, got8 = layer.run(tile, form)
            if got is not None:
                assert got.shape == ref.shape
                if not torch.equal(got, ref):
                    bad = got != ref
                    wrong.append((case.id, form + ":f32", int(bad.sum()), bad.nonzero()[0].tolist(), (got - ref).abs().max().item()))
            if got8 is not None:
                assert got8.shape == ref8.shape
                words[form] = got8
                if not torch.equal(got8, ref8):
                    bad = got8 != ref8
                    wrong.append((case.id, form + ":s8", int(bad.sum()), bad.nonzero()[0].tolist(),
                                  (S.decode_s8(got8) - S.decode_s8(ref8)).abs().max().item()))
        if not torch.equal(words["s8"], words["both"]):
            wrong.append((case.id, "s8 != both", int((words["s8"] != words["both"]).sum()), [], 0.0))
    # (case, launch form : output, elements that differ, the first of them (NHWC), largest difference), one per line and unabridged
    assert not wrong, f"tile {tile}: " + "\n".join(map(str, wrong))


def _split8_values(pixels, c, generator):
    """Full mantissas over 200 binades, with +-0, exact round-to-nearest-even ties of the hi half (low half 0x8000, bit 16 clear and
    set) and of the lo half, and values whose rounding carries into the exponent, in both signs."""
    x = torch.randn((pixels, c), generator=generator) * torch.exp2(torch.randint(-100, 101, (pixels, c), generator=generator).float())
    x = torch.where(x.abs() < 2.0 ** -100, x * 2.0 ** 40, x)                   # (a low half below 2^-126 would be a denormal)
    pos = [0x00000000, 0x3F808000, 0x3F818000, 0x40FE8000, 0x40FF8000,       # +0; hi ties: to even down, to even up, ..., with a carry
           0x3F7FFFFF, 0x3FFFFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x3F808001,       # carries into the exponent; just below and above a tie
           0x3F804040, 0x3F8040C0, 0x3F80BFC0, 0x42C87F80, 0x6C7FFFFF, 0x0E7FC080]      # lo ties: to even down, up; negative lo; ...
    special = torch.tensor(pos + [b - 2 ** 31 for b in pos], dtype=torch.int64)
    special = torch.where(special >= 2 ** 31, special - 2 ** 32, special).to(torch.int32).view(torch.float32)
    flat = x.flatten()
    where = torch.randperm(flat.numel(), generator=generator)[:special.numel()]
    flat[where] = special
    flat[c - 1], flat[-1] = special[2], special[12]                            # the last channel of a partial group, the last element
    return flat.view(pixels, c)


@pytest.mark.parametrize("c", [8, 20, 44])
def test_split8_is_the_bf16_split_bit_for_bit(c):
    """premvos_split8_f32 against the host encoder of tests/conv_s8_cases.py.  c = 20 and 44 end in a partial group, whose absent
    channels are NaN in the input buffer and must be stored as zeros.  Denormal inputs or low halves and values that round to
    infinity are left out: what becomes of them is decided by the compile mode (flush-to-zero), not by the kernel."""
    _lib, lib, ops = _ops()
    n, h, w = 1, 7, 43                                                         # 301 pixels: 2 to 8 blocks of 256 threads, the last ragged
    g = torch.Generator().manual_seed(c)
    x = _split8_values(n * h * w, c, g).view(n, h, w, c)
    tiny = 2.0 ** -126
    assert torch.isfinite(x).all() and ((x == 0) | (x.abs() >= 2.0 ** -100)).all() and x.abs().max().item() < 2.0 ** 120
    c8 = S._r(c, 8)
    full = torch.zeros((n, h, w, c8))
    full[..., :c] = x
    want = S.encode_s8(full)
    lo_half = want.view(torch.bfloat16).view(n, h, w, -1, 2, 8)[..., 1, :].float()
    assert ((lo_half == 0) | (lo_half.abs() >= tiny)).all()
    off, off8 = 4, 8
    src = torch.full((n, h, w, off + c8 + 4), float("nan"))
    src[..., off:off + c] = x
    src = src.cuda()
    before = src.clone()
    dst = torch.full((n, h, w, off8 + c8 + 16), SENTINEL, device="cuda")
    ops.split8(ops.NHWC(src, c=c, coff=off), ops.NHWC(dst, c=c8, coff=off8, layout="s8"))
    torch.cuda.synchronize()
    assert torch.equal(bits(src), bits(before))
    got = bits(dst.cpu())
    assert torch.all(torch.cat([got[..., :off8], got[..., off8 + c8:]], -1) == sentinel_bits())
    got = got[..., off8:off8 + c8]
    bad = got != want
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[0].tolist(), hex(bits(full)[bad][0].item() & 0xffffffff))
    # ... and as the package reads it back
    view = ops.NHWC(dst, c=c8, coff=off8, layout="s8").torch().cpu()
    assert torch.equal(view, S.decode_s8(want).permute(0, 3, 1, 2))


def test_tiles_are_bit_identical_on_gaussian_data():
    """Every tile adds an output's products in the same order (32-channel blocks in ascending k; lo.hi, hi.lo, hi.hi per 16-deep
    step): the tile is an order-neutral knob, for the general instantiation and the fallback of tile 10 as for the pointwise one."""
    for case_id in S.GAUSSIAN:
        layer = _layer(case_id, True)
        ref = None
        for tile in range(len(S.TILES)):
            got, got8 = layer.run(tile, "both")
            assert torch.isfinite(got).all() and torch.isfinite(S.decode_s8(got8)).all()
            if ref is None:
                ref = (got, got8)
            assert torch.equal(bits(got), bits(ref[0])) and torch.equal(got8, ref[1]), (case_id, tile, S.instance(layer.case, tile))


def test_gaussian_inputs_stay_inside_the_derived_bounds():
    """Both bounds are derived, neither is measured from the kernel; they hold element by element.

    Emulated sum: against the float64 sum of the split products the kernel is specified to add (+ bias + residual, an S8 residual as
    hi + lo),
        |got - emu| <= (3 * k_pad + 2) * 2^-23 * S_abs,    k_pad = taps * roundup(cin, 32),
    the first-order bound of a float32 sum of that many terms in any order; 2^-23 is twice the unit roundoff, which covers an MFMA
    accumulate that truncates instead of rounding to nearest.  The first addition, to a zero accumulator, is exact, which leaves room
    for the one rounding of leaky ReLU's multiply; ReLU and leaky ReLU are 1-Lipschitz and keep the bound.
    True convolution: the same plus 2^-16 * S_true, S_true = conv(|x|, |w|) + |b| + |res| (lo * lo and the two residues of rounding
    lo), and for an S8 residual 2^-16 |res| for what hi + lo loses of it.
    The S8 output is the split of the fp32 output: its words are encode_s8 of it, and hi + lo is within 2^-16 |v| of v."""
    worst_emu, worst_true = 0.0, 0.0
    for case_id in S.GAUSSIAN:
        layer = _layer(case_id, True)
        case = layer.case
        data = S.gaussian_inputs(case)
        pre, s_abs = S.product_sum(case, data)
        emu = S.nhwc(S.activate(case, pre))
        true, s_true = S.true_conv(case, data)
        bound_emu = S.nhwc((3 * S.k_pad(case) + 2) * 2.0 ** -23 * s_abs)
        bound_true = bound_emu + S.nhwc(2.0 ** -16 * s_true + (2.0 ** -16 * data.res.double().abs() if case.res == "s8" else 0))
        true = S.nhwc(true)
        assert bound_emu.min().item() > 0
        for tile in range(len(S.TILES)):
            got, got8 = layer.run(tile, "both")
            assert torch.equal(got8, S.encode_s8(got)), (case_id, tile)
            assert ((S.decode_s8(got8).double() - got.double()).abs() <= 2.0 ** -16 * got.double().abs()).all(), (case_id, tile)
            r_emu = ((got.double() - emu).abs() / bound_emu).max().item()
            r_true = ((got.double() - true).abs() / bound_true).max().item()
            worst_emu, worst_true = max(worst_emu, r_emu), max(worst_true, r_true)
            assert r_emu <= 1 and r_true <= 1, (case_id, tile, r_emu, r_true)
    print(f"largest error / bound = {worst_emu:.4f} against the emulated products, {worst_true:.4f} against the true convolution")


def test_entry_refuses_what_it_cannot_run():
    """One launch per PV_REQUIRE of premvos_conv_bf16x3_s8_f32 and premvos_split8_f32.  All are host-side checks that return before
    anything is launched: an error code, the message, and every output word keeps the sentinel."""
    _lib, lib, ops = _ops()
    stream = _lib.current_stream()
    g = torch.Generator().manual_seed(1)
    x = ops.NHWC(torch.zeros((1, 6, 6, 48), device="cuda"), c=32, coff=8, layout="s8")
    pk = ops.pack_conv_s8(torch.randn((16, 32, 1, 1), generator=g), torch.randn((16,), generator=g))
    out = ops.NHWC(torch.empty((1, 6, 6, 24), device="cuda"), c=16, coff=4)
    out8 = ops.NHWC(torch.empty((1, 6, 6, 32), device="cuda"), c=16, coff=8, layout="s8")
    res = ops.NHWC.alloc(1, 6, 6, 16)
    res8 = ops.NHWC(torch.zeros((1, 6, 6, 32), device="cuda"), c=16, coff=8, layout="s8")
    sent = sentinel_bits()

    def refused(message, edit=None, **args):
        d = ops.conv_s8_desc(x, pk, out, out8)
        a = dict(dp=ctypes.byref(d), inp=x.ptr, wgt=pk.wgt.data_ptr(), out8=out8.ptr, out8_ps=out8.ps, res8=None, res8_ps=0, tile=0)
        a.update(args)
        if edit is not None:
            edit(d)
        out.buf.fill_(SENTINEL)
        out8.buf.fill_(SENTINEL)
        rc = lib.premvos_conv_bf16x3_s8_f32(a["dp"], a["inp"], a["wgt"], a["out8"], a["out8_ps"], a["res8"], a["res8_ps"], a["tile"], stream)
        torch.cuda.synchronize()
        assert rc != 0, message
        assert message in lib.premvos_last_error().decode(), (message, lib.premvos_last_error().decode())
        assert torch.all(bits(out.buf) == sent) and torch.all(bits(out8.buf) == sent), f"{message}: a refused launch wrote"

    def setter(**fields):
        def edit(d):
            for k, v in fields.items():
                setattr(d, k, v)
        return edit

    refused("null pointer", dp=None)
    refused("null pointer", inp=None)
    refused("null pointer", wgt=None)
    refused("no output", setter(out=None), out8=None)
    refused("bad dims", setter(n=0))
    refused("bad geometry", setter(kh=5, kw=10))                               # 50 taps
    refused("bad geometry", setter(dh=0))
    refused("S8 input needs", setter(cin=12))                                  # cin % 8
    refused("S8 input needs", setter(in_ps=44))
    refused("S8 input needs", inp=x.ptr + 16)                                  # a 16-byte but not 32-byte boundary
    refused("cout % 8 == 0", setter(cout=12))
    refused("fp32 output", setter(out_ps=22))                                  # out_ps % 4
    refused("fp32 output", setter(out=out.ptr + 8))
    refused("S8 output", out8=out8.ptr + 16)
    refused("S8 output", out8_ps=20)
    refused("residual: res_ps", setter(res=res.ptr, res_ps=18))
    refused("bias must be", setter(bias=pk.bias.data_ptr() + 4))
    refused("an S8 residual excludes", setter(res=res.ptr, res_ps=res.ps), res8=res8.ptr, res8_ps=res8.ps)       # both residual kinds
    refused("an S8 residual excludes", res8=res8.ptr + 16, res8_ps=res8.ps)
    refused("bad activation", setter(act=ops.ACT_SIGMOID))
    refused("NHWC output only", setter(out_mode=ops.OUT_PIXSHUF2))
    refused("unknown tile -1", tile=-1)
    refused("unknown tile 12", tile=12)

    src = torch.zeros((1, 6, 6, 24), device="cuda")
    dst = torch.full((1, 6, 6, 32), SENTINEL, device="cuda")
    for message, a in (("split8: bad arguments", (None, 24, dst.data_ptr(), 32, 36, 20)),
                       ("split8: bad arguments", (src.data_ptr(), 24, None, 32, 36, 20)),
                       ("split8: bad arguments", (src.data_ptr(), 24, dst.data_ptr(), 32, 0, 20)),
                       ("split8: in_ps", (src.data_ptr(), 22, dst.data_ptr(), 32, 36, 20)),
                       ("split8: in_ps", (src.data_ptr(), 24, dst.data_ptr(), 16, 36, 20)),        # out_ps < roundup(c, 8)
                       ("split8: in_ps", (src.data_ptr(), 24, dst.data_ptr() + 4, 32, 36, 20))):
        rc = lib.premvos_split8_f32(*a, stream)
        torch.cuda.synchronize()
        assert rc != 0 and message in lib.premvos_last_error().decode(), (message, a)
        assert torch.all(bits(dst) == sent), f"{message}: a refused launch wrote"
