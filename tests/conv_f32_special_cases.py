"""The case table of the exact tests of the two fp32 conv kernels beside the implicit GEMM that the tuner picks on its own (ops._candidates,
ops.rule_choice): the streaming pointwise kernel (csrc/conv_stream_f32.hip, tile hint 5) and the direct kernel for one- and two-channel
heads (csrc/conv_smalln_f32.hip, tile hint 1, and hint 0 for cout <= 2).  The shapes tests/test_gpu_conv_f32_special.py runs, the inputs
for which the kernels have to be EXACT, and the float64 value they have to return for them.  A plain module without a GPU:
tests/test_cpu_conv_f32_special_cases.py proves on the CPU that the exactness condition holds for every case and that the table reaches
every mechanism its comments name.

conv_stream_f32_kernel is one template <KG, ACT, HAS_RES> with 12 instances (KG 8 / 16 = K 64 / 128, three activations, with / without a
residual); conv_smalln_f32.hip has conv_smalln_kernel<1>, conv_smalln_kernel<2> (16 lanes per output pixel) and
conv_smalln_tile_kernel<2, 4, 4> (16 lanes per 4x4 tile of outputs).  `python tests/conv_f32_special_cases.py` prints, per instance, the
cases that launch it.

Exactness: the argument of tests/conv_f32_cases.py.  Activations and weights come from the lattice +-h + j * 2^-4 (h in 1 .. hmax, j in
-3 .. 3), bias and residual are multiples of 2^-8 in [-8, 8]; every product is a multiple of 2^-8 and while
    S_abs = conv(|x|, |w|) + |bias| + |residual| < 2^16
every partial sum of an output element, in ANY order, fits the 24 bits of a float: nothing rounds, with or without FMA contraction (a
fused multiply-add rounds once what needs no rounding), through the MFMA accumulators and through the 16-lane shuffle butterfly of the
direct kernel.  The expected value is the float64 pre-activation -> .float() -> the activation in float32 (conv_f32_cases.activate);
the comparison is torch.equal on floats.  Sigmoid is out of scope: the streaming kernel refuses it and its rounding is not exact."""
import functools
from collections import namedtuple

import torch

import conv_exact as K
import conv_f32_cases as B
from conv_f32_cases import Data, S_ABS_LIMIT, QUANTUM, SLOPE, activate, magnitude  # noqa: F401  (the lattice is the fp32 table's)

ACTS = ["none", "relu", "leaky"]
STREAM_INSTANCES = [(kg, act, res) for kg in (8, 16) for act in ACTS for res in (False, True)]
# the six instances test_gpu_flow_kernels.py::test_streaming_pointwise_kernel_is_bit_identical_to_the_implicit_gemm never launches
STREAM_UNTESTED_BEFORE = [(8, "none", False), (8, "none", True), (8, "leaky", False), (8, "leaky", True), (16, "relu", False),
                          (16, "leaky", True)]
SMALLN_KERNELS = ["conv_smalln_kernel<1>", "conv_smalln_kernel<2>", "conv_smalln_tile_kernel<2, 4, 4>"]
STREAM_ROWS, STREAM_BN = 256, 128            # rows of output pixels per workgroup step; columns per column tile
LPP, TY, TX = 16, 4, 4                       # the direct kernel: lanes per output pixel (or tile), the tile
GRID_CAP = 256 * 12                          # ... and its largest grid: 3072 workgroups of 16 pixels (or tiles) = 49152 per trip
TILED_MIN_TILES = 100
LDS_ATTR = 48 * 1024                         # above it the launch raises the kernel's dynamic-LDS limit first

# kernel: "stream" / "smalln".  pad = (top, left, bottom, right).  win_in / win_out / win_res: (pixel stride, first channel) of the
# channel window in a wider, sentinel-filled buffer; None = a buffer of its own.  bias False: packed with bias=None.  inf: all operands
# positive and +Inf in every channel of the map's four corner pixels.  hints: the (tile_hint, stage_k) launches of the case.
Case = namedtuple("Case", "id kernel n h w cin cout k stride dil pad act res hmax win_in win_out win_res bias inf hints deconv")


def _s(id, n, h, w, cin, cout, act="none", res=False, win_in=None, win_out=None, win_res=None, bias=True):
    return Case(id, "stream", n, h, w, cin, cout, 1, 1, 1, (0, 0, 0, 0), act, res, 3, win_in, win_out, win_res, bias, False, ((5, 0),), False)


def _d(id, n, h, w, cin, cout, k, stride=1, dil=1, pad=(0, 0, 0, 0), act="none", res=False, hmax=3, win_out=None, inf=False,
       hints=((1, 0),)):
    return Case(id, "smalln", n, h, w, cin, cout, k, stride, dil, pad, act, res, hmax, None, win_out, None, True, inf, hints, False)


SAME = (1, 1, 1, 1)
BOTH = ((1, 0), (1, 1))                      # a tiled case: the tiled form and, with stage_k 1, the per-pixel form on the same layer
AUTO = ((1, 0), (0, 0))                      # forced, and what hint 0 (auto) does for cout <= 2

STREAM_CASES = [
    # One case per instance <KG, ACT, HAS_RES>.  M = output pixels = rows; a step is 256 rows (8 waves x 32), a column tile 128 couts.
    # <8, NONE, false>, the Xception entry flow's pointwise half (BN folded, no ReLU).  M = 35: one step, waves 2 .. 7 see only clamped rows
    _s("k64-none", 1, 5, 7, 64, 128),
    # M = 256: one exactly full step; two column tiles; the residual is a window (offset 4) of a buffer with res_ps 264 != out_ps
    _s("k64-none-res", 1, 16, 16, 64, 256, res=True, win_res=(264, 4)),
    # M = 257: a second step that holds one row; cout 384 = three column tiles, 80 walkers (85 rounded down to a multiple of 8)
    _s("k64-relu", 1, 1, 257, 64, 384, act="relu"),
    # cout 512 (64 walkers) with m_steps = 67: three workgroups of every column tile walk a second step (the A prefetch inside the loop,
    # step += wgs)
    _s("k64-relu-res-walk", 1, 100, 170, 64, 512, act="relu", res=True),
    # cin 62 < cin_pad 64 inside an input window (in_ps 72, offset 4): the window's two pad channels are zero and meet zero weights
    _s("k64-leaky-c62", 2, 9, 10, 62, 128, act="leaky", win_in=(72, 4)),
    # an output window (out_ps = cout + 8, offset 4); M = 273: two steps, batch boundaries inside a step
    _s("k64-leaky-res", 3, 7, 13, 64, 256, act="leaky", res=True, win_out=(264, 4)),
    # packed with bias=None: the kernel's `p.bias != nullptr ? ... : 0` in a launch that runs
    _s("k128-none-nobias", 1, 5, 7, 128, 128, bias=False),
    # cout 384 (80 walkers) with m_steps = 83 at K = 128
    _s("k128-none-res-walk", 2, 100, 105, 128, 384, res=True),
    # cin 126 < cin_pad 128 inside an input window (in_ps 136, offset 4); M = 257
    _s("k128-relu-c126", 1, 1, 257, 126, 256, act="relu", win_in=(136, 4)),
    # four column tiles, one full step, output window and residual window of different pixel strides
    _s("k128-relu-res", 1, 16, 16, 128, 512, act="relu", res=True, win_out=(520, 4), win_res=(516, 0)),
    # M = 429: an interior step and a ragged one
    _s("k128-leaky", 3, 11, 13, 128, 128, act="leaky"),
    # <16, LEAKY, true> on three column tiles, M = 35
    _s("k128-leaky-res", 1, 5, 7, 128, 384, act="leaky", res=True),
]

SMALLN_CASES = [
    # --- the per-pixel form: 16 lanes share an output pixel, lane `sub` owns channels 4 * sub + 64 * u (u = 0 .. 3) + 256 * trip ---
    # 1x1 with cin 32: on the applicability floor kh * kw * cin_pad >= 32; lanes 8 .. 15 are idle (sub * 4 >= cin_pad).
    # 230 x 230 = 52900 pixels > 49152: the grid is capped and the grid-stride loop takes a second trip
    _d("pp1-pw-c32-230", 1, 230, 230, 32, 1, 1, act="leaky"),
    # M = 3: fewer pixels than one workgroup holds (16); the output is the window [3, 5) of 5-float pixels: an odd channel offset,
    # pixels that are not 8-byte aligned; a residual with res_ps 4
    _d("pp2-pw-c32-m3", 1, 1, 3, 32, 2, 1, act="leaky", res=True, win_out=(5, 3), hints=AUTO),
    _d("pp1-pw-c32-m3", 1, 1, 3, 32, 1, 1, res=True, win_out=(5, 3), hints=AUTO),
    # 3x3 with cin 4: only lane 0 of the 16 has channels
    _d("pp1-k3-c4", 1, 5, 6, 4, 1, 3, pad=SAME),
    _d("pp2-k3-c4", 1, 5, 6, 4, 2, 3, pad=SAME, act="leaky", hints=AUTO),
    # cin 68: lane 0 runs a second 64-channel step (u = 1), the other lanes one
    _d("pp1-k3-c68", 1, 5, 6, 68, 1, 3, pad=SAME, res=True),
    _d("pp2-k3-c68", 1, 5, 6, 68, 2, 3, pad=SAME, act="relu"),
    # cin 260: lane 0 takes a second trip of the 256-channel c loop
    _d("pp1-k3-c260", 1, 5, 6, 260, 1, 3, pad=SAME, act="leaky"),
    _d("pp2-k3-c260", 1, 5, 6, 260, 2, 3, pad=SAME, res=True),
    # the k7-c3 geometry of conv_f32_cases.py with two outputs: 7x7, stride 2, asymmetric padding, cin_pad 4
    _d("pp2-k7-c3", 1, 19, 23, 3, 2, 7, stride=2, pad=(2, 2, 3, 3), act="relu"),
    _d("pp1-k7-c3", 1, 19, 23, 3, 1, 7, stride=2, pad=(2, 2, 3, 3)),
    # dilation 2 with taps outside the map on all four sides; a batch of 3: m / hw crosses images inside a workgroup
    _d("pp1-atrous", 3, 8, 9, 36, 1, 3, dil=2, pad=(2, 2, 2, 2), act="relu"),
    _d("pp2-atrous", 3, 8, 9, 36, 2, 3, dil=2, pad=(2, 2, 2, 2), act="leaky", res=True),
    # 3x3 with cin 700 and two outputs: 2 x 6304 x 4 = 50432 B of weights in LDS, the > 48 KB attribute branch
    _d("pp2-c700-lds", 1, 5, 6, 700, 2, 3, pad=SAME, hmax=2),
    # 3x3 "same" with ONE output on a map of 100 tiles: it must stay on the per-pixel form (the tiled kernel exists for two outputs)
    _d("pp1-same-40x40", 1, 40, 40, 36, 1, 3, pad=SAME, act="leaky", hints=AUTO),
    # 36 x 44 = 9 x 11 = 99 tiles: just under the threshold, the per-pixel form
    _d("pp2-same-36x44", 1, 36, 44, 36, 2, 3, pad=SAME, hints=AUTO),
    # --- the tiled form (3x3 / stride 1 / "same" / two outputs / >= 100 tiles of 4x4): lane `sub` owns channels 4 * sub + 64 * step ---
    # 37 x 43 = 10 x 11 tiles, a ragged last tile in both directions; three images; cin 36 < one 64-channel step (lanes 9 .. 15 idle)
    _d("tile-37x43-n3", 3, 37, 43, 36, 2, 3, pad=SAME, act="leaky", res=True, hints=BOTH),
    # exactly 100 tiles, the threshold; cin 68: lane 0 takes a second channel step
    _d("tile-40x40", 1, 40, 40, 68, 2, 3, pad=SAME, act="relu", hints=BOTH + ((0, 0),)),
    # cin 568 (PWC-Net's predict_flow heads read 565 .. 597 channels): nine channel steps, lanes 14 and 15 eight
    _d("tile-c568", 1, 40, 44, 568, 2, 3, pad=SAME, res=True, hmax=2, hints=BOTH),
    # 900 x 900 with cin 4: 225 x 225 = 50625 tiles > 49152, a second grid-stride trip of the tiled form (and 17 of the per-pixel form)
    _d("tile-900", 1, 900, 900, 4, 2, 3, pad=SAME, hints=BOTH),
    # non-finite border pixels: all operands positive, +Inf in every channel of the four corner pixels.  The tiled kernel reads a patch
    # position outside the map from the CLAMPED address -- here a corner -- and has to select zero, not multiply by a zero mask
    # (0 * Inf = NaN): +Inf exactly at the outputs whose 3x3 window covers a corner, the exact finite value everywhere else, no NaN
    _d("tile-inf-corners", 1, 37, 43, 36, 2, 3, pad=SAME, inf=True, hints=BOTH),
]

CASES = STREAM_CASES + SMALLN_CASES
BY_ID = {c.id: c for c in CASES}
# The layers of the Gaussian-data tests: the six streaming instances no test launched before, and both forms of the direct kernel
GAUSSIAN = ["k64-none", "k64-none-res", "k64-leaky-c62", "k64-leaky-res", "k128-relu-c126", "k128-leaky-res",
            "tile-37x43-n3", "tile-40x40", "pp2-same-36x44", "pp1-same-40x40", "pp2-k7-c3"]

cin_pad, k_pad, k_real, gemm_extent, out_extent, gemm_rows, conv = B.cin_pad, B.k_pad, B.k_real, B.gemm_extent, B.out_extent, B.gemm_rows, B.conv


def terms(case):
    """Products behind an output element as the kernel counts them: k_pad for the streaming kernel, kh * kw * cin_pad for the direct one."""
    return k_pad(case) if case.kernel == "stream" else k_real(case)


def stream_instance(case):
    """<KG, ACT, HAS_RES> of launch_kg."""
    return (k_pad(case) // 8, case.act, case.res)


def stream_walk(case):
    """(walkers per column tile, steps of 256 rows) the way launch() of conv_stream_f32.hip computes them."""
    m_steps = -(-gemm_rows(case) // STREAM_ROWS)
    n_tiles = case.cout // STREAM_BN
    wgs = max(8, (256 // n_tiles) & ~7)
    while wgs > 8 and wgs - 8 >= m_steps:
        wgs -= 8
    return wgs, m_steps


def tiles(case):
    """4x4 tiles of one image."""
    ho, wo = gemm_extent(case)
    return -(-ho // TY) * -(-wo // TX)


def smalln_kernel(case, stage_k=0):
    """The kernel conv_smalln() launches: the tiled form by the layer's geometry per IMAGE, never by the batch."""
    same = (case.k, case.stride, case.dil) == (3, 1, 1) and case.pad[:2] == (1, 1) and gemm_extent(case) == (case.h, case.w)
    if same and case.cout == 2 and stage_k != 1 and tiles(case) >= TILED_MIN_TILES:
        return SMALLN_KERNELS[2]
    return SMALLN_KERNELS[case.cout - 1]


def smalln_applicable(case):
    """conv_smalln_applicable, and the condition under which ops._candidates offers hint 1."""
    return case.cout <= 2 and case.cout * k_pad(case) * 4 <= 150 * 1024 and k_real(case) >= 32


def lds_bytes(case):
    return case.cout * k_pad(case) * 4


def work_items(case, stage_k=0):
    """Groups of 16 lanes the launch needs: tiles of the tiled form, pixels of the per-pixel form."""
    return case.n * tiles(case) if smalln_kernel(case, stage_k) == SMALLN_KERNELS[2] else gemm_rows(case)


def grid_trips(case, stage_k=0):
    """Trips of the grid-stride loop of the busiest group of 16 lanes."""
    items = work_items(case, stage_k)
    blocks = max(1, min(GRID_CAP, -(-items * LPP // 256)))
    return -(-items // (blocks * 256 // LPP))


def idle_lanes(case):
    """Lanes of the 16 that own no channel (sub * 4 >= cin_pad)."""
    return max(0, LPP - cin_pad(case) // 4)


def c_trips(case, stage_k=0):
    """Trips of lane 0 through the channel loop: 64 channels per step in the tiled form, 256 (four loads in flight) per pixel."""
    return -(-cin_pad(case) // (64 if smalln_kernel(case, stage_k) == SMALLN_KERNELS[2] else 256))


def corner_outputs(case):
    """Mask [ho][wo] of the outputs whose window covers one of the map's four corner pixels (3x3 "same": the 2x2 blocks at the corners)."""
    ho, wo = gemm_extent(case)
    m = torch.zeros((ho, wo), dtype=torch.bool)
    for ys in (slice(0, 2), slice(ho - 2, ho)):
        for xs in (slice(0, 2), slice(wo - 2, wo)):
            m[ys, xs] = True
    return m


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The lattice inputs of the case (float32, on the host; the same tensors on every call: do not write to them).  A case packed
    without a bias has b = 0 here: what the reference adds."""
    data = B.inputs(case)
    if not case.bias:
        data = data._replace(b=torch.zeros_like(data.b))
    if case.inf:
        data = data._replace(x=data.x.abs(), w=data.w.abs())
        data.x[:, :, ::case.h - 1, ::case.w - 1] = float("inf")
    return data


def finite_inputs(case):
    """inputs(case) with the +Inf pixels of an `inf` case replaced by zeros: what S_abs and the finite outputs are computed from."""
    data = inputs(case)
    return data._replace(x=torch.where(torch.isinf(data.x), torch.zeros(()), data.x)) if case.inf else data


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> (what the kernel must return for the lattice inputs, float64 NCHW; S_abs of the finite operands).  The activation is applied in
    float32 to the exact pre-activation.  An `inf` case: torch's float64 convolution with zero padding of the input as it is."""
    return K.exact(case.act, B.pre_activation(case, inputs(case))), magnitude(case, finite_inputs(case))


true_conv, gaussian_inputs = B.true_conv, B.gaussian_inputs


def launches_of(case):
    """[(tile_hint, stage_k, kernel instance)] of the case."""
    if case.kernel == "stream":
        return [(h, st, stream_instance(case)) for h, st in case.hints]
    return [(h, st, smalln_kernel(case, st)) for h, st in case.hints]


def instances():
    """Case ids (+ launch) per kernel instance: the 12 streaming instances, the three direct kernels."""
    out = {i: [] for i in STREAM_INSTANCES + SMALLN_KERNELS}
    for c in CASES:
        for hint, st, inst in launches_of(c):
            out[inst].append(c.id if (hint, st) in ((5, 0), (1, 0)) else f"{c.id} (hint {hint} stage_k {st})")
    return out


if __name__ == "__main__":                   # python tests/conv_f32_special_cases.py: per kernel instance, the cases that launch it
    for inst, ids in instances().items():
        name = inst if isinstance(inst, str) else f"conv_stream_f32_kernel<{inst[0]}, {inst[1].upper()}, {str(inst[2]).lower()}>"
        print(f"{name}  {', '.join(ids) if ids else 'NOTHING'}")
