"""The RoI head with conv5's first 1x1 projected once on the feature map (RoIAlign of W.fm, then bias and ReLU) against the head it
replaces (RoIAlign of fm, then the conv on every RoI pixel): both against group 3 computed in float64 from the SAME RoIAlign output.

Measured on MI355X, (1, 1, 2, 1) blocks, 112 x 160 image, 100 RoI slots, max|ref| 4.672, bar 2e-3 * max|ref|:
    max |feat5 - float64| / max|ref|: projected head 1.47e-06, legacy head 1.57e-06."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS, IMAGE_HW = (1, 1, 2, 1), (112, 160)      # the smallest net the suite runs (tests/golden/proposal_host_refs.json "graph")
PROJ = "group3/block0/conv1/proj"


def _mm(x, w_oihw, ky=0, kx=0):
    """NHWC float64 pixels times one tap of an OIHW kernel."""
    return x @ w_oihw[:, :, ky, kx].t()


def _group3_f64(net, w, roi):
    """resnet_conv5 (basemodel.py:92-99) on NHWC float64 RoIs with the net's own folded fp32 weights (scale folded in fp32, as packed)."""
    from premvos_amd.proposal.model import _fold_bn

    def folded(name):
        scale, bias = _fold_bn(w[name + "/bn"])
        return (w[name + "/W"].float() * scale.view(-1, 1, 1, 1)).double().cuda(), bias.double().cuda()

    x = roi
    for i in range(net.num_blocks[3]):
        p = f"group3/block{i}"
        s = 2 if i == 0 else 1
        w1, b1 = folded(p + "/conv1")
        t = torch.relu(_mm(x, w1) + b1)
        w2, b2 = folded(p + "/conv2")
        n, h, wd, _ = t.shape
        if s == 2:                      # pad [0,1] + VALID stride 2
            tp = torch.nn.functional.pad(t, (0, 0, 0, 1, 0, 1))
            ho, wo = (h + 1 - 3) // 2 + 1, (wd + 1 - 3) // 2 + 1
        else:
            tp = torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
            ho, wo = h, wd
        acc = torch.zeros((n, ho, wo, w2.shape[0]), dtype=torch.float64, device="cuda")
        for ky in range(3):
            for kx in range(3):
                acc += _mm(tp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s, :], w2, ky, kx)
        t = torch.relu(acc + b2)
        w3, b3 = folded(p + "/conv3")
        y = _mm(t, w3) + b3
        if p + "/convshortcut/W" in w:
            ws, bs = folded(p + "/convshortcut")
            sc = _mm(x[:, ::s, ::s, :][:, :ho, :wo, :], ws) + bs
        else:
            sc = x
        x = torch.relu(y + sc)
    return x


def test_projected_head_stays_within_the_bar_of_the_float64_head(capsys):
    from premvos_amd import _lib, ops, synth
    from premvos_amd.proposal import ProposalNet
    from premvos_amd.proposal.model import ANCHOR_STRIDE, TEST_POST_NMS_TOPK as R
    w = synth.proposal_weights(3, BLOCKS)
    fr, _ = synth.video_frames(1, *IMAGE_HW, rank=7)
    img = fr[:1, :, :, [2, 1, 0]].contiguous().cuda()
    new = ProposalNet(w, BLOCKS, use_graph=False)
    assert PROJ in new.packed
    old = ProposalNet(w, BLOCKS, use_graph=False)
    del old.packed[PROJ]                                   # without the projected weights the plan builds the legacy head
    pn, po = new.run_resized(img), old.run_resized(img)
    torch.cuda.synchronize()
    names = [n for n, _ in pn.steps]
    assert "conv:" + PROJ in names and "roi_align" not in names and "roi_align" in [n for n, _ in po.steps]
    # nothing upstream of the head moved
    fm = pn.featuremap
    assert torch.equal(fm.buf, po.featuremap.buf) and torch.equal(pn.rois, po.rois) and torch.equal(pn.roi_count, po.roi_count)
    assert int(pn.roi_count.item()) > 0
    # the float64 head, from the plan's own feature map and RoIs through the legacy RoIAlign
    roi = ops.NHWC.alloc(R, 14, 14, 1024)
    _lib.check(_lib.load().premvos_roi_align_f32(fm.ptr, fm.ps, 1, fm.h, fm.w, 1024, pn.rois.data_ptr(), pn.roi_count.data_ptr(), R,
                                                 1.0 / ANCHOR_STRIDE, 14, roi.ptr, roi.ps, _lib.current_stream()), "roi_align")
    ref = _group3_f64(new, w, roi.buf.double())
    scale = float(ref.abs().max())
    f_new = pn.feat5.buf[..., :2048].double()
    f_old = po.feat5.buf[..., :2048].double()
    assert f_new.shape == ref.shape
    e_new, e_old = float((f_new - ref).abs().max()) / scale, float((f_old - ref).abs().max()) / scale
    with capsys.disabled():
        print(f"\nfeat5 vs float64 head, max|err| / max|ref| (max|ref| {scale:.3f}): projected head {e_new:.3e}, legacy head {e_old:.3e}")
    assert e_new <= 2e-3
    # the results that hang on feat5: same detections
    assert torch.equal(pn.final_count, po.final_count) and torch.equal(pn.final_idx, po.final_idx)
    assert float((pn.final_probs - po.final_probs).abs().max()) < 1e-3 and float((pn.final_boxes - po.final_boxes).abs().max()) < 0.05
