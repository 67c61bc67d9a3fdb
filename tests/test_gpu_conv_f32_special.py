"""Every instance of the two fp32 conv kernels the tuner picks beside the implicit GEMM, launched directly: the streaming pointwise kernel
(csrc/conv_stream_f32.hip, tile hint 5: 12 instances <KG, ACT, HAS_RES>) and the direct kernel for one- and two-channel heads
(csrc/conv_smalln_f32.hip, tile hint 1 and, for cout <= 2, hint 0: conv_smalln_kernel<1>, <2> and conv_smalln_tile_kernel<2, 4, 4>).

The cases and the reasoning are tests/conv_f32_special_cases.py; tests/test_cpu_conv_f32_special_cases.py proves its premises without a GPU.

(a) On lattice inputs no partial sum of an output element needs rounding, so every instance has to return the float64 value of
    conv + bias + residual bit for bit: torch.equal, no tolerance.  One product dropped or doubled changes the value by at least 2^-8.
    Everything around the output window, and the whole input buffer, comes back bit for bit.
(b) The streaming kernel writes the bits of the implicit GEMM's tiles on Gaussian data (what ops.numerics_key promises the tuner), on
    the six instances no test launched before.
(c) The direct kernel's form follows the map, never the batch, and a launch repeats its bits.
(d) On Gaussian data the error stays inside a derived bound, element by element.
(e) +Inf in border pixels reaches exactly the outputs whose window covers them: no NaN out of a clamped address.
(f) What the kernels cannot run is refused with a message, nothing is written, and ops.stream_applicable mirrors the library.

Mutations the file is meant to catch, each made by hand in a scratch copy of the kernel source, none touching a global address, a bound
or a barrier; the ids that failed on the MI355X, and what test_gpu_flow_kernels.py (82 tests) said of the same library:
  1. conv_stream_f32.hip: the fourth MFMA of a group (a[g].w * b[j].w) dropped in every instance
       -> (a) all 12 streaming ids, (b), (d); there 8 failures (every case of test_streaming_pointwise_kernel_is_bit_identical_...)
  2. ... dropped in <8, NONE, false> alone (`if constexpr`), the Xception entry flow's instance
       -> (a) k64-none alone, (b), (d); there all 82 passed: no test launched that instance
  3. conv_stream_f32.hip: the staging store reading acc[jj * 2 + half] for acc[half * 2 + jj]
       -> (a) all 12 streaming ids, (b), (d); there the same 8 failures
  4. conv_smalln_f32.hip, tiled form: the FMA reading the tap weight w[(kx + 1) % 3][co]
       -> (a) tile-37x43-n3, tile-40x40, tile-c568, tile-900, (e) tiled, (d); there 3 failures (test_two_channel_heads_tiled_form_...)
  5. conv_smalln_f32.hip, tiled form: the accumulators zeroed once before the grid-stride loop, not on every trip
       -> (a) tile-900 alone (the second trip adds to the first trip's sums); there all 82 passed: no grid took a second trip
  6. conv_smalln_f32.hip, tiled form: the border select `in ? v[q] : 0` replaced by the product v[q] * (m * my[r])
       -> (e) tiled alone (NaN where +Inf belongs); (a) to (d) and (f) passed; there all 82 passed
"""
import ctypes

import pytest
import torch

import conv_f32_special_cases as T
from conv_exact import round_up
from conv_exact_device import SENTINEL, DeviceLayer, bits, difference, ops as _ops, tile_hint

pytestmark = pytest.mark.gpu

EXACT = [c for c in T.CASES if not c.inf]
GEMM_TILES = [((128, 128), 16), ((64, 64), 16)]


class _Special(DeviceLayer):
    """Besides the input and output windows, a residual inside a window of a sentinel-filled buffer with a pixel stride of its own, and
    weights packed without a bias."""
    table = T
    RES_WINDOWED = True

    def pack(self, ops, data):
        pk = ops.pack_conv(data.w, data.b if self.case.bias else None)
        assert (pk.bias is None) == (not self.case.bias)
        return pk

    def check_desc(self, _lib, ops, d):
        case = self.case
        assert d.out_mode == ops.OUT_NHWC and d.precision == _lib.PRECISIONS["fp32"] and (d.ho, d.wo) == T.gemm_extent(case)
        assert (d.k_pad, d.cin_pad, d.cout, d.in_ps, d.out_ps) == (T.k_pad(case), T.cin_pad(case), case.cout, self.xin.shape[-1], self.out.shape[-1])
        assert d.res_ps == (self.res.ps if self.res else 0) and bool(d.bias) == case.bias
        if case.kernel == "stream":
            assert ops.stream_applicable(d), case.id
        else:
            assert T.smalln_applicable(case) and (1, 0, -1, 0, 0) in ops._candidates(d), case.id


def _run_all(layer, ref):
    """Every launch of the case (run_hint asserts that the library asks for no workspace) -> the launches that differ from ``ref``."""
    wrong = []
    for hint, stage, inst in T.launches_of(layer.case):
        got = layer.run_hint(hint, stage)
        assert got.shape == ref.shape
        if not torch.equal(got, ref):
            wrong.append(difference(layer.case.id, f"hint {hint} stage_k {stage}: {inst}", got, ref))
    return wrong


@pytest.mark.parametrize("case", EXACT, ids=[c.id for c in EXACT])
def test_every_instance_is_exact_on_lattice_inputs(case):
    """(a).  A tiled case runs both forms of the direct kernel; `hints` of the case names its launches."""
    ref = T.expected(case)[0].float()
    wrong = _run_all(_Special(case, T.inputs(case)), ref)
    assert not wrong, wrong                  # (case, launch, elements that differ, the first of them, largest difference)


@pytest.mark.parametrize("stage_k", [0, 1], ids=["tiled", "per-pixel"])
def test_non_finite_border_pixels_reach_only_the_outputs_that_cover_them(stage_k):
    """(e).  +Inf in every channel of the four corner pixels, all other operands positive.  The tiled form reads the patch positions
    outside the map from clamped addresses -- for the corner tiles, the +Inf pixels -- and must select zero for them: a zero mask that
    is multiplied gives 0 * Inf = NaN, here inside the +Inf outputs.  The per-pixel form skips the taps."""
    case = T.BY_ID["tile-inf-corners"]
    assert T.smalln_kernel(case, stage_k) == T.SMALLN_KERNELS[2 if stage_k == 0 else 1]
    ref = T.expected(case)[0].float()
    got = _Special(case, T.inputs(case)).run_hint(1, stage_k)
    corners = T.corner_outputs(case).expand_as(ref)
    assert not torch.isnan(got).any(), torch.isnan(got).nonzero().tolist()
    assert torch.equal(torch.isinf(got), corners) and (got[corners] > 0).all()
    assert torch.equal(got, ref), difference(case.id, f"stage_k {stage_k}", got, ref)


def _gaussian(kernel):
    return [T.BY_ID[i] for i in T.GAUSSIAN if T.BY_ID[i].kernel == kernel]


def test_streaming_kernel_writes_the_bits_of_the_gemm_tiles():
    """(b).  The construction of test_gpu_flow_kernels.py::test_streaming_pointwise_kernel_is_bit_identical_to_the_implicit_gemm on the
    six instances it does not run, with input, output and residual windows: same numerics_key, same bits."""
    _lib, lib, ops = _ops()
    ran = set()
    for case in _gaussian("stream"):
        layer = _Special(case, T.gaussian_inputs(case))
        d = layer.d
        got = layer.run_hint(5, 0)
        assert torch.isfinite(got).all()
        for tile, stage in GEMM_TILES:
            assert ops.numerics_key(d, (tile_hint(tile), stage, -1, 0, 0)) == ops.numerics_key(d, (5, 0, -1, 0, 0))
            layer.configure(tile_hint(tile), stage, -1)
            gemm = layer.launch()
            assert torch.equal(bits(got), bits(gemm)), (case.id, tile, difference(case.id, "hint 5 vs tile", got, gemm))
        ran.add(T.stream_instance(case))
    assert ran == set(T.STREAM_UNTESTED_BEFORE)


def test_direct_kernel_form_follows_the_map_never_the_batch():
    """(c).  Gaussian data, where the two forms' summation orders show: the tiled form runs at 100 tiles and not at 99, nor for one
    output channel; image 0 of a batch of 3 has the bits of a batch of 1 in either form; a launch repeats its bits."""
    def both(case, data=None):
        layer = _Special(case, T.gaussian_inputs(case) if data is None else data)
        runs = [layer.run_hint(1, 0), layer.run_hint(1, 1), layer.run_hint(1, 0), layer.run_hint(1, 1)]
        assert torch.equal(bits(runs[0]), bits(runs[2])) and torch.equal(bits(runs[1]), bits(runs[3])), case.id
        assert torch.isfinite(runs[0]).all() and torch.isfinite(runs[1]).all()
        return runs[0], runs[1]
    tiled, pixel = both(T.BY_ID["tile-40x40"])
    assert not torch.equal(bits(tiled), bits(pixel))               # 100 tiles: the tiled form ran
    for i in ("pp2-same-36x44", "pp1-same-40x40"):                   # 99 tiles; one output channel
        auto, pixel = both(T.BY_ID[i])
        assert torch.equal(bits(auto), bits(pixel)), i
    batch = T.BY_ID["tile-37x43-n3"]
    data = T.gaussian_inputs(batch)
    tiled3, pixel3 = both(batch)
    assert not torch.equal(bits(tiled3), bits(pixel3))
    one = batch._replace(id=batch.id + "-image0", n=1)
    tiled1, pixel1 = both(one, T.Data(data.x[:1], data.w, data.b, data.res[:1]))
    assert torch.equal(bits(tiled3[:1]), bits(tiled1)) and torch.equal(bits(pixel3[:1]), bits(pixel1))


def test_gaussian_inputs_stay_inside_the_derived_bound():
    """(d).  Derived, not measured from the kernels; it holds element by element:
        |got - true| <= (terms + 2) * 2^-23 * S_true,    S_true = conv(|x|, |w|) + |b| + |res|,
    the bound of tests/test_gpu_conv_f32.py: the first-order bound of a float32 sum of terms + 2 numbers in any order (the products --
    k_pad of them in the streaming kernel, kh * kw * cin_pad in the direct one, whose 16 lanes add their shares in a butterfly --, bias,
    residual) with 2^-23, twice the unit roundoff, per addition; the first addition, to a zero accumulator, is exact, which leaves room
    for the one rounding of leaky ReLU's multiply; ReLU and leaky ReLU are 1-Lipschitz.  The exact test (a) is the sharp one."""
    worst = {}
    for case in _gaussian("stream") + _gaussian("smalln"):
        data = T.gaussian_inputs(case)
        true, s_true = T.true_conv(case, data)
        assert s_true.min().item() > 0
        bound = (T.terms(case) + 2) * 2.0 ** -23 * s_true
        layer = _Special(case, data)
        for hint, stage, inst in T.launches_of(case):
            got = layer.run_hint(hint, stage).double()
            ratio = ((got - true).abs() / bound).max().item()
            name = inst if isinstance(inst, str) else "conv_stream_f32_kernel"
            worst[name] = max(worst.get(name, 0.0), ratio)
            print(f"{case.id} hint {hint} stage_k {stage}: largest error / bound = {ratio:.4f}")
            assert ratio <= 1, (case.id, hint, stage, ratio)
    print("largest error / bound per kernel:", {k: round(v, 4) for k, v in worst.items()})


def _edge_desc(ops, cin=64, cout=128, k=1, stride=1, act=None, out_ps=None, out_off=0, res_ps=None, hint=5, shuffle=False):
    """A 6 x 8 layer on buffers of its own (sentinel-filled output) -> (descriptor, output buffer, what has to stay alive)."""
    g = torch.Generator().manual_seed(cin + cout)
    n, h, w = 1, 6, 8
    x = ops.NHWC(torch.randn((n, h, w, round_up(cin, 4)), generator=g).cuda(), c=cin)
    if shuffle:                                                        # ConvTranspose2d(2, stride 2): a 1x1 layer with 4 * cout phase outputs
        pk = ops.pack_deconv2x2s2(torch.randn((cin, cout // 4, 2, 2), generator=g), torch.zeros(cout // 4))
        ho, wo, c_out = 2 * h, 2 * w, cout // 4
    else:
        pk = ops.pack_conv(torch.randn((cout, cin, k, k), generator=g), torch.zeros(cout))
        ho, wo, c_out = (h - 1) // stride + 1, (w - 1) // stride + 1, cout
    out_buf = torch.full((n, ho, wo, out_ps or round_up(c_out, 4)), SENTINEL, device="cuda")
    out = ops.NHWC(out_buf, c=c_out, coff=out_off)
    res = ops.NHWC(torch.zeros((n, ho, wo, res_ps), device="cuda"), c=cout) if res_ps else None
    d = ops.conv_desc(x, pk, out, stride=(stride, stride), pad=(k // 2, k // 2), act=ops.ACT_RELU if act is None else act, res=res,
                      tile_hint=hint, split_k=-1)
    return d, out_buf, (x, pk, out, res)


def test_refusals_and_the_python_mirror():
    """(f).  On each edge of premvos::conv_stream_applicable the library's decision equals ops.stream_applicable(d); a refused launch
    says why and writes nothing.  Hint 1 is refused for three outputs and for fewer than 32 products.  No accepted launch of either
    kernel asks for workspace."""
    _lib, lib, ops = _ops()
    stream = _lib.current_stream()
    untouched = bits(torch.tensor([SENTINEL]))[0].item()

    def launch(d, out_buf):
        need = lib.premvos_conv2d_workspace_bytes(ctypes.byref(d))
        rc = lib.premvos_conv2d_f32(ctypes.byref(d), stream)
        torch.cuda.synchronize()
        assert rc != 0 or need == 0
        wrote = not bool(torch.all(bits(out_buf) == untouched))
        return rc, wrote, lib.premvos_last_error().decode()

    edges = {"k_pad 192": dict(cin=192), "cout 640": dict(cout=640), "cout 96": dict(cout=96), "stride 2": dict(stride=2),
             "3x3": dict(k=3), "out_ps 130": dict(out_ps=130), "out offset 2": dict(out_ps=132, out_off=2), "res_ps 130": dict(res_ps=130),
             "sigmoid": dict(act=ops.ACT_SIGMOID), "pixel shuffle": dict(shuffle=True)}
    accepted = {"k 64": dict(), "k 128 / cout 512": dict(cin=128, cout=512), "cin 62": dict(cin=62), "leaky": dict(act=ops.ACT_LEAKY),
                "res_ps 132 / out_ps 136": dict(res_ps=132, out_ps=136, out_off=4)}
    for name, kw in list(edges.items()) + list(accepted.items()):
        d, out_buf, keep = _edge_desc(ops, **kw)
        rc, wrote, msg = launch(d, out_buf)
        assert ops.stream_applicable(d) == (rc == 0), (name, rc, msg)
        assert (rc == 0) == (name in accepted) == wrote, (name, rc, wrote, msg)
        if rc != 0:
            assert "streaming pointwise" in msg, (name, msg)
            with pytest.raises(_lib.PremvosError, match="streaming pointwise"):
                ops.run_desc(d)
    for name, kw, ok in (("cout 3", dict(cin=16, cout=3, k=3), False), ("16 products", dict(cin=16, cout=2), False),
                         ("32 products", dict(cin=32, cout=2), True), ("cout 1", dict(cin=16, cout=1, k=3), True)):
        d, out_buf, keep = _edge_desc(ops, hint=1, **kw)
        rc, wrote, msg = launch(d, out_buf)
        assert (rc == 0) == ok == wrote == ((1, 0, -1, 0, 0) in ops._candidates(d)), (name, rc, wrote, msg)
        if not ok:
            assert "the direct small-N kernel does not apply" in msg, (name, msg)
