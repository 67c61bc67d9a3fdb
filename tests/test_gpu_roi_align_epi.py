"""premvos_roi_align_epi_f32 (RoIAlign with a bin stride and a bias / ReLU epilogue) against the legacy entry premvos_roi_align_f32:
a kept bin is the legacy bin, bit for bit, and the epilogue is one fp32 add and one max on top of it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, W, R, OUT = 2, 9, 11, 6, 14
IW, IH = W * 16.0, H * 16.0
# image coordinates (spatial_scale 1/16): fully inside; over the left / top edge; beyond W-1 / H-1; the whole frame; zero width
BOXES = [[40.0, 30.0, 120.0, 100.0], [-50.0, -40.0, 60.0, 50.0], [100.0, 80.0, IW + 84.0, IH + 76.0], [0.0, 0.0, IW, IH],
         [64.0, 32.0, 64.0, 96.0]]
COUNT = [4, 0]
_CACHE = {}


def _case(c, rot, padded):
    """Inputs and the legacy output of one case, computed once: ``rot`` rotates the five boxes through the four valid slots of image
    0 (count = [4, 0]), so that each kind of box is a valid RoI in one of the two rotations."""
    key = (c, rot, padded)
    if key not in _CACHE:
        from premvos_amd import _lib, ops
        g = torch.Generator().manual_seed(100 * c + rot)
        ps = c + 4 if padded else c
        fm = ops.NHWC(torch.zeros((B, H, W, ps), device="cuda"), c=c)
        fm.buf[..., :c] = torch.randn((B, H, W, c), generator=g).cuda()
        fm.buf[..., c:] = 1e30                                    # a channel beyond c is never read
        order = [(i + rot) % len(BOXES) for i in range(R)]
        rois = torch.tensor([[BOXES[i] for i in order]] * B, dtype=torch.float32).cuda().contiguous()
        cnt = torch.tensor(COUNT, dtype=torch.int32, device="cuda")
        bias = (torch.randn(c, generator=g) * 0.5).cuda()
        assert (bias > 0).any() and (bias < 0).any()
        leg = ops.NHWC(torch.full((B * R, OUT, OUT, c), -3.0, device="cuda"), c=c)
        _lib.check(_lib.load().premvos_roi_align_f32(fm.ptr, fm.ps, B, H, W, c, rois.data_ptr(), cnt.data_ptr(), R, 1.0 / 16, OUT,
                                                     leg.ptr, leg.ps, _lib.current_stream()), "roi_align")
        torch.cuda.synchronize()
        assert not (leg.buf == -3.0).any() and float(leg.buf[COUNT[0]:].abs().max()) == 0.0 and float(leg.buf[:COUNT[0]].abs().max()) > 0
        _CACHE[key] = (fm, rois, cnt, bias, leg.buf)
    return _CACHE[key]


def _epi(fm, rois, cnt, c, step, bias, act, padded):
    """The new entry's output [B*R, on, on, c]; ``padded``: written into a channel window of a wider buffer, whose other channels
    must keep their fill."""
    from premvos_amd import _lib, ops
    on = (OUT + step - 1) // step
    buf = torch.full((B * R, on, on, c + 8 if padded else c), -7.0, device="cuda")
    out = ops.NHWC(buf, c=c, coff=4 if padded else 0)
    _lib.check(_lib.load().premvos_roi_align_epi_f32(fm.ptr, fm.ps, B, H, W, c, rois.data_ptr(), cnt.data_ptr(), R, 1.0 / 16, OUT, step,
                                                     bias.data_ptr() if bias is not None else None, act, out.ptr, out.ps,
                                                     _lib.current_stream()), "roi_align_epi")
    torch.cuda.synchronize()
    if padded:
        assert (buf[..., :4] == -7.0).all() and (buf[..., 4 + c:] == -7.0).all()
        return buf[..., 4:4 + c].contiguous()
    return buf


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("c", [8, 132])
def test_epilogue_and_bin_step_are_bit_exact_on_the_legacy_output(c, rot, padded):
    from premvos_amd.ops import ACT_NONE, ACT_RELU
    fm, rois, cnt, bias, leg = _case(c, rot, padded)
    n_valid = COUNT[0]
    # step 1, bias, ReLU = relu(legacy + bias)
    got = _epi(fm, rois, cnt, c, 1, bias, ACT_RELU, padded)
    want = torch.relu(leg + bias)
    assert (want[:n_valid] == 0).any() and (want[:n_valid] > 0).any()           # the ReLU bites, and not everywhere
    assert _same_bits(got, want)
    assert _same_bits(got[n_valid:], torch.relu(bias).expand(B * R - n_valid, OUT, OUT, c))     # beyond count, all of image 1: act(bias)
    # step 2, no epilogue = the even bins
    got = _epi(fm, rois, cnt, c, 2, None, ACT_NONE, padded)
    assert _same_bits(got, leg[:, ::2, ::2, :])
    assert float(got[n_valid:].abs().max()) == 0.0
    # step 2, bias, no activation
    got = _epi(fm, rois, cnt, c, 2, bias, ACT_NONE, padded)
    assert _same_bits(got, leg[:, ::2, ::2, :] + bias)
    assert _same_bits(got[n_valid:], bias.expand(B * R - n_valid, OUT // 2, OUT // 2, c))
    # step 1 without an epilogue is the legacy entry
    assert _same_bits(_epi(fm, rois, cnt, c, 1, None, ACT_NONE, padded), leg)


def test_arguments_outside_the_contract_are_refused():
    from premvos_amd import _lib
    from premvos_amd.ops import ACT_NONE, ACT_SIGMOID
    fm, rois, cnt, bias, _ = _case(8, 0, False)
    out = torch.zeros((B * R, OUT, OUT, 8), device="cuda")
    lib = _lib.load()

    def call(step, bias_ptr, act):
        return lib.premvos_roi_align_epi_f32(fm.ptr, fm.ps, B, H, W, 8, rois.data_ptr(), cnt.data_ptr(), R, 1.0 / 16, OUT, step, bias_ptr,
                                             act, out.data_ptr(), 8, _lib.current_stream())
    assert call(3, None, ACT_NONE) != 0                       # bin_step 1 or 2
    assert call(1, None, ACT_SIGMOID) != 0                    # none or ReLU
    assert call(1, bias.data_ptr() + 4, ACT_NONE) != 0        # a bias that 16-byte loads cannot read
    assert call(1, bias.data_ptr(), ACT_NONE) == 0
    torch.cuda.synchronize()
