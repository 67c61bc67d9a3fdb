"""The device path between "the refined masks are in HBM" and "the embeddings are in HBM" (premvos_amd/csrc/reid_ops.hip,
ReIDNet.embed_masks): the masks' rleToBbox boxes, their context boxes and the crops of several frames in one launch, each
against the host code it replaces.  Boxes and crops are exact; embeddings agree within 1e-3 of the tensor's max (the bar of
tests/test_gpu_reid.py: another launch size may pick another k-split)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import reid_oracle as R  # noqa: E402

SMALL_O = [R.UNITS[0], ("res3", 2, (64, 64), (3, 3), (2, 1)), ("res12", 2, (32, 64), (3, 3), (1, 2)),
           ("res15", 3, (32, 64, 96), (1, 3, 1), (1, 2, 1)), ("res16", 3, (48, 96, 128), (1, 3, 1), (1, 1, 1))]
SMALL = [(n, f, k, s) for n, _, f, k, s in SMALL_O]


def _host_boxes(masks):
    from premvos_amd import rle
    return np.array([rle.to_bbox(rle.encode(m)) for m in masks], np.float64).astype(np.int32).reshape(-1, 4)


def _device_boxes(block, n, h, w, feed=0, with_context=True):
    """``block``: a uint8 CUDA tensor [n, HB, WB] whose top-left h x w windows are the masks."""
    from premvos_amd import _lib
    assert block.is_contiguous()
    bbox = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    ctx = torch.full((n, 4), -7, dtype=torch.int32, device="cuda")
    ws = torch.zeros((n, _lib.MASK_BBOX_SLABS, 4), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().premvos_mask_bbox_u8(block.data_ptr(), n, h, w, block.stride(0), block.stride(1), feed, bbox.data_ptr(),
                                                ctx.data_ptr() if with_context else None, ws.data_ptr(), _lib.current_stream()),
               "mask_bbox")
    return bbox.cpu().numpy(), ctx.cpu().numpy()


def _blobs(rng, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(1, 4))):
            cy, cx = rng.uniform(0, h), rng.uniform(0, w)
            ry, rx = rng.uniform(2, h / 3), rng.uniform(2, w / 3)
            out[i] |= ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1).astype(np.uint8)
        out[i] &= (rng.random((h, w)) < 0.9).astype(np.uint8)            # ragged: many runs
        out[i] *= np.uint8(rng.integers(1, 256))                        # nonzero = foreground, whatever the value
    return out


def _special_masks(h, w):
    masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        masks.append(m)
    for second in ((0, 3), (1, 3)):          # a run that crosses from column 2 into column 3 / its neighbour that does not
        m = np.zeros((h, w), np.uint8)
        m[h - 1, 2] = 1
        m[second] = 1
        masks.append(m)
    m = np.zeros((h, w), np.uint8)           # the crossing far from the rest of the mask
    m[h // 2:h // 2 + 3, 5:9] = 1
    m[h - 1, w - 2] = m[0, w - 1] = 1
    masks.append(m)
    return np.stack(masks)


def test_issue_examples_of_the_column_rule_on_the_host():
    """The two 6x5 masks the rule is stated with (what the device kernel is held to below)."""
    from premvos_amd import rle
    for second, want in (((0, 2), [1, 0, 2, 6]), ((1, 2), [1, 1, 2, 5])):
        m = np.zeros((6, 5), np.uint8)
        m[5, 1] = 1
        m[second] = 1
        assert rle.to_bbox(rle.encode(m)) == [float(v) for v in want]


@pytest.mark.parametrize("h,w,hb,wb,n", [(6, 5, 6, 5, 9), (120, 200, 120, 200, 17), (120, 200, 131, 211, 17),
                                         (480, 854, 480, 854, 40), (480, 854, 487, 859, 40), (33, 1, 33, 1, 9), (1, 37, 1, 40, 9)])
def test_mask_boxes_equal_to_bbox_of_the_rle(h, w, hb, wb, n):
    rng = np.random.default_rng(h * 1000 + w)
    special = _special_masks(h, w) if h >= 4 and w >= 4 else np.stack(
        [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)] + [(rng.random((h, w)) < 0.5).astype(np.uint8) for _ in range(7)])
    masks = np.concatenate([special, _blobs(rng, n - len(special), h, w)]) if n > len(special) else special[:n]
    block = rng.integers(1, 256, (n, hb, wb), dtype=np.uint8)            # everything outside the windows is foreground-valued
    block[:, :h, :w] = masks
    want = _host_boxes(masks)
    got, ctx = _device_boxes(torch.from_numpy(block).cuda(), n, h, w)
    assert np.array_equal(got, want), (got[(got != want).any(1)], want[(got != want).any(1)])
    assert (want[0] == 0).all() and list(want[1]) == [0, 0, w, h]
    from premvos_amd.reid import context_boxes
    assert np.array_equal(ctx, context_boxes(want, h, w, feed=False))
    got2, _ = _device_boxes(torch.from_numpy(block).cuda(), n, h, w, with_context=False)
    assert np.array_equal(got2, got)


def _box_grid(H, W):
    xs = sorted({0, 1, 2, 3, 10, 11, 12, 13, 25, 26, W // 2, W // 2 + 1, W - 30, W - 11, W - 10, W - 6, W - 5, W - 1})
    ys = sorted({0, 1, 10, 11, H // 2, H // 2 + 1, H - 20, H - 10, H - 5, H - 1})
    ws = [1, 2, 3, 5, 10, 11, 15, 20, 25, 35, 45, 64, 100]
    hs = [1, 4, 5, 10, 15, 25, 30, 55]
    boxes = [[x, y, w, h] for x in xs for w in ws if x + w <= W for y in ys for h in hs if y + h <= H]
    boxes += [[0, 0, 0, 0], [0, 0, W, H], [0, 0, W, 1], [0, 0, 1, H], [W - 1, H - 1, 1, 1], [0, H - 5, W, 5], [W - 5, 0, 5, H]]
    return np.array(boxes, np.int32)


@pytest.mark.parametrize("feed", [False, True])
@pytest.mark.parametrize("H,W", [(120, 200), (480, 854)])
def test_context_boxes_equal_the_host_function_ties_included(feed, H, W):
    from premvos_amd import _lib
    from premvos_amd.reid import context_boxes
    boxes = _box_grid(H, W)
    # the inputs that land exactly on .5 before tf.round, computed as the host function does (float32, its order of operations)
    b = boxes.astype(np.float32)
    f = np.float32(1.2 - 1.0)
    pre = np.concatenate([b[:, 0] - np.float32(0.5) * b[:, 2] * f, b[:, 1] - np.float32(0.5) * b[:, 3] * f,
                          b[:, 2] * np.float32(1.2), b[:, 3] * np.float32(1.2)])
    ties = int((np.abs(pre - np.floor(pre)) == 0.5).sum())
    assert ties > 0, "the grid no longer holds a round-half-even tie"
    want = context_boxes(boxes, H, W, feed)
    assert list(context_boxes([[10, 0, 5, 5], [11, 0, 5, 5]], H, W, feed)[:, 0]) == [10, 10]
    d_in = torch.from_numpy(boxes).cuda()
    d_out = torch.full_like(d_in, -7)
    _lib.check(_lib.load().premvos_reid_context_boxes_i32(d_in.data_ptr(), len(boxes), H, W, int(feed), d_out.data_ptr(),
                                                          _lib.current_stream()), "context_boxes")
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want), (boxes[(got != want).any(1)][:5], got[(got != want).any(1)][:5], want[(got != want).any(1)][:5])


@pytest.mark.parametrize("zero_small", [0, 1])
def test_crops_of_three_frames_equal_the_one_frame_kernel_bit_for_bit(zero_small):
    from premvos_amd import _lib
    H, W, F, S = 120, 200, 3, 128
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).cuda()
    boxes = np.array([[10, 20, 60, 40], [0, 0, 200, 120], [150, 80, 50, 40], [0, 0, 0, 0], [5, 5, 8, 30], [30, 5, 100, 110],
                      [190, 110, 10, 10], [3, 100, 40, 9], [60, 60, 11, 11], [0, 0, 0, 0], [100, 0, 100, 119]], np.int32)
    fos = np.array([2, 0, 1, 1, 0, 2, 2, 0, 1, 2, 0], np.int32)
    n = len(boxes)
    lib = _lib.load()
    d_boxes, d_fos = torch.from_numpy(boxes).cuda(), torch.from_numpy(fos).cuda()
    got = torch.full((n, S, S, 4), 9.0, device="cuda")
    _lib.check(lib.premvos_reid_input_frames_u8(frames.data_ptr(), F, H, W, d_fos.data_ptr(), d_boxes.data_ptr(), n, S, zero_small,
                                                got.data_ptr(), _lib.current_stream()), "reid_input_frames")
    want = torch.full((n, S, S, 4), 7.0, device="cuda")
    for i in range(n):
        _lib.check(lib.premvos_reid_input_u8(frames[int(fos[i])].data_ptr(), H, W, d_boxes[i].data_ptr(), 1, S, zero_small,
                                             want[i].data_ptr(), _lib.current_stream()), "reid_input")
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    zero = want[3]                                           # the empty box: the normalised zero image
    assert torch.equal(got[9], zero)
    assert torch.equal(got[4], zero) == bool(zero_small)     # min(w, h) <= 10: zero only in the in-merge feed form
    assert not torch.equal(got[0], zero)


def test_embed_masks_against_the_host_fed_path_and_the_oracle():
    from premvos_amd import rle
    from premvos_amd.reid import ReIDEngine, ReIDNet
    from premvos_amd.reid.model import context_boxes
    H, W, F, n = 120, 200, 2, 7
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    masks = _blobs(rng, n, H, W)
    masks[3] = 0                                             # one empty mask keeps its slot
    masks[5] = 0
    masks[5, H - 1, 40] = masks[5, 0, 41] = 1                # the column rule inside the net's plan
    masks[5, 30:60, 40:90] = 1
    fos = np.array([0, 1, 1, 0, 1, 0, 1], np.int32)
    w = R.synth_weights(0, SMALL_O)
    net = ReIDNet(w, units=SMALL, use_graph=False)
    eng = ReIDEngine(net)
    d_frames, d_masks, d_fos = torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(fos).cuda()
    emb, bbox = net.embed_masks(d_frames, d_masks, d_fos, 8, feed=False)
    assert emb.is_cuda and bbox.is_cuda and emb.shape == (n, 128) and bbox.shape == (n, 4) and bbox.dtype == torch.int32
    first, boxes = emb.clone(), bbox.cpu().numpy()
    want_boxes = _host_boxes(masks)
    assert np.array_equal(boxes, want_boxes)
    assert (want_boxes[3] == 0).all() and want_boxes[5][1] == 0 and want_boxes[5][3] == H
    live = [i for i in range(n) if want_boxes[i][2] > 0 and want_boxes[i][3] > 0]
    assert live == [0, 1, 2, 4, 5, 6]
    got = first.cpu().numpy()
    assert np.isfinite(got).all()
    ref = np.zeros((n, 128), np.float32)
    host = np.zeros((n, 128), np.float32)
    for f in range(F):
        idx = [i for i in live if fos[i] == f]
        host[idx] = eng.embed(frames[f], [rle.to_bbox(rle.encode(masks[i])) for i in idx], feed=False)
        cb = R.context_boxes(want_boxes[idx].astype(np.float64), H, W, feed=False)
        assert np.array_equal(np.asarray(cb, np.int32), context_boxes(want_boxes[idx], H, W, False))
        ref[idx] = R.forward(w, np.stack([R.make_crop(frames[f], b, feed=False) for b in cb]), SMALL_O)
    for other in (host, ref):
        bar = 1e-3 * max(1.0, float(np.abs(other[live]).max()))
        assert np.abs(got[live] - other[live]).max() < bar
    # a second call: identical bits (no atomics, fixed launch sizes)
    emb2, bbox2 = net.embed_masks(d_frames, d_masks, d_fos, 8, feed=False)
    assert torch.equal(emb2.view(torch.int32), first.view(torch.int32)) and np.array_equal(bbox2.cpu().numpy(), boxes)
    # the engine: a strided window of a larger block as the masks, one packed result
    block = torch.zeros((n, H + 3, W + 5), dtype=torch.uint8, device="cuda")
    block[:, :H, :W] = d_masks
    block[:, H:, :] = 1
    block[:, :, W:] = 1
    out = torch.zeros((n, 132), device="cuda")
    e3, b3 = eng.embed_masks(d_frames, block[:, :H, :W], d_fos, feed=False, out=out)
    assert np.array_equal(b3.cpu().numpy(), boxes)
    assert np.array_equal(out[:, 128:].cpu().numpy().view(np.int32), boxes)
    bar = 1e-3 * max(1.0, float(np.abs(host[live]).max()))
    assert np.abs(e3.cpu().numpy()[live] - host[live]).max() < bar


def test_engine_chunks_more_slots_than_a_plan_holds():
    """45 masks of 3 frames with max_boxes 20: three launches (20, 20, 5 padded to 20), results in slot order."""
    from premvos_amd.reid import ReIDEngine, ReIDNet
    H, W, F, n = 60, 90, 3, 45
    rng = np.random.default_rng(13)
    frames = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).cuda()
    masks = _blobs(rng, n, H, W)
    fos = torch.from_numpy(rng.integers(0, F, n).astype(np.int32)).cuda()
    net = ReIDNet(R.synth_weights(0, SMALL_O), units=SMALL, use_graph=False)
    emb, bbox = ReIDEngine(net, max_boxes=20).embed_masks(frames, torch.from_numpy(masks).cuda(), fos)
    assert np.array_equal(bbox.cpu().numpy(), _host_boxes(masks))
    one, _ = ReIDEngine(net, max_boxes=45).embed_masks(frames, torch.from_numpy(masks).cuda(), fos)
    ok = (bbox[:, 2] > 0) & (bbox[:, 3] > 0)
    assert int(ok.sum()) >= 30
    assert (emb[ok] - one[ok]).abs().max().item() < 1e-3 * max(1.0, one[ok].abs().max().item())


def test_lanes_keep_their_own_plans_and_results():
    """Two refinement lanes of the streaming driver share one net: a call on lane 1 must not touch what lane 0 holds."""
    from premvos_amd.reid import ReIDNet
    H, W, n = 60, 90, 5
    rng = np.random.default_rng(17)
    frames = torch.from_numpy(rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)).cuda()
    a, b = (torch.from_numpy(_blobs(rng, n, H, W)).cuda() for _ in range(2))
    fos = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device="cuda")
    net = ReIDNet(R.synth_weights(0, SMALL_O), units=SMALL, use_graph=False)
    e0, b0 = net.embed_masks(frames, a, fos, 8, lane=0)
    keep_e, keep_b = e0.clone(), b0.clone()
    e1, b1 = net.embed_masks(frames, b, fos, 8, lane=1)
    assert e0.data_ptr() != e1.data_ptr() and b0.data_ptr() != b1.data_ptr()
    assert torch.equal(e0, keep_e) and torch.equal(b0, keep_b)
    assert np.array_equal(b1.cpu().numpy(), _host_boxes(b.cpu().numpy())) and not torch.equal(e0, e1)
    again, _ = net.embed_masks(frames, a, fos, 8, lane=1)                   # the same input on the other lane: the same bits
    assert torch.equal(again.view(torch.int32), keep_e.view(torch.int32))
