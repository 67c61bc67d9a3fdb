"""The launch list of the proposal plan's RoI heads (host logic: the builder's shape-only pass on CPU tensors, no library, no GPU):
the fp32 main head projects conv5's first 1x1 once on the feature map and interpolates the result; the mask head is the legacy one."""
import pytest
import torch

from premvos_amd import _lib, arena

CPU = torch.device("cpu")
BLOCKS, B, IMG_H, IMG_W = (1, 1, 1, 2), 2, 64, 96
PROJ = "group3/block0/conv1/proj"


@pytest.fixture(scope="module")
def weights():
    from oracle import proposal_oracle as PO
    return PO.synth_weights(0, BLOCKS)


def _dry_plan(monkeypatch, weights, **kw):
    """ProposalNet on CPU tensors and the first (shape-only) pass of its plan builder; a launch would fail: the library is an object()."""
    from premvos_amd.proposal import model
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    monkeypatch.setattr(_lib, "load", lambda: object())
    net = model.ProposalNet(weights, BLOCKS, device=CPU, use_graph=False, **kw)
    plan = object.__new__(model._Plan)
    plan.b, plan.h, plan.w = B, IMG_H, IMG_W
    plan._build(net, B, IMG_H, IMG_W, arena.Arena(CPU, dry=True))
    return net, plan


def _conv_rows(plan):
    conv = [n for n, _ in plan.steps if n.startswith("conv:")]
    assert len(conv) == len(plan.descs)
    return {n: (d.n * d.ho * d.wo, d.kh * d.kw * d.cin, d.cout, d.sh, bool(d.bias)) for n, d in zip(conv, plan.descs)}


def test_fp32_main_head_projects_once_and_interpolates(monkeypatch, weights):
    from premvos_amd.proposal.model import TEST_POST_NMS_TOPK as R
    net, plan = _dry_plan(monkeypatch, weights, precision="fp32")
    names = [n for n, _ in plan.steps]
    rows = _conv_rows(plan)
    fh, fw = plan.featuremap.h, plan.featuremap.w
    # the projected conv: every feature-map pixel once, 1024 -> 512, no bias (bias and ReLU follow the interpolation)
    assert rows["conv:" + PROJ] == (B * fh * fw, 1024, 512, 1, False)
    assert plan.flops["conv:" + PROJ] == 2.0 * B * fh * fw * 1024 * 512
    head = names[names.index("rpn_proposals"):]
    assert head[:7] == ["rpn_proposals", "roi_align_epi:group3/block0/conv1", "roi_align_epi:group3/block0/convshortcut",
                        "conv:group3/block0/conv2", "conv:group3/block0/convshortcut", "conv:group3/block0/conv3",
                        "conv:group3/block1/conv1"]
    assert names.index("conv:" + PROJ) < names.index("rpn_proposals")
    assert "roi_align" not in names and "conv:group3/block0/conv1" not in names
    # no conv runs the 1024-deep matrix on every RoI pixel any more; the shortcut reads the 7 x 7 even bins at stride 1
    assert not [n for n, (m, k, _, _, _) in rows.items() if m == B * R * 196 and k == 1024]
    assert rows["conv:group3/block0/convshortcut"] == (B * R * 49, 1024, 2048, 1, True)
    assert rows["conv:group3/block0/conv2"][:2] == (B * R * 49, 9 * 512) and rows["conv:group3/block1/conv1"][:2] == (B * R * 49, 2048)
    assert plan.feat5.n == B * R and (plan.feat5.h, plan.feat5.w, plan.feat5.c) == (7, 7, 2048)


def test_mask_head_keeps_the_legacy_list(monkeypatch, weights):
    from premvos_amd.proposal.model import RESULTS_PER_IM as M
    net, plan = _dry_plan(monkeypatch, weights, precision="fp32", mode_mask=True)
    names = [n for n, _ in plan.steps]
    rows = _conv_rows(plan)
    assert names[names.index("roi_align_mask"):] == [
        "roi_align_mask", "conv:mask:group3/block0/conv1", "conv:mask:group3/block0/conv2", "conv:mask:group3/block0/convshortcut",
        "conv:mask:group3/block0/conv3", "conv:mask:group3/block1/conv1", "conv:mask:group3/block1/conv2", "conv:mask:group3/block1/conv3",
        "conv:maskrcnn/deconv", "conv:maskrcnn/conv"]
    assert rows["conv:mask:group3/block0/conv1"] == (B * M * 196, 1024, 512, 1, True)
    assert rows["conv:mask:group3/block0/convshortcut"] == (B * M * 49, 1024, 2048, 2, True)
    assert "conv:" + PROJ in names and names.count("conv:" + PROJ) == 1          # the main head of the same plan is the projected one


def test_without_fp32_group3_weights_the_head_is_the_legacy_one(monkeypatch, weights):
    """The projected weights exist only where group 3 is packed for the fp32 kernels; a plan without them builds the head as before."""
    net, plan = _dry_plan(monkeypatch, weights, precision="bf16")
    assert PROJ not in net.packed
    names = [n for n, _ in plan.steps]
    head = names[names.index("rpn_proposals"):]
    assert head[:3] == ["rpn_proposals", "roi_align", "conv:group3/block0/conv1"] and not [n for n in names if n.startswith("roi_align_epi")]
