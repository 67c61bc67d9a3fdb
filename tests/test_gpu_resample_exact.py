"""The resampling kernels around the convs (csrc/refine_ops.hip: refine_input_kernel, resize_bilinear_kernel, broadcast_kernel,
seg_softmax_kernel / seg_uncrop_kernel / seg_conf_kernel; csrc/reid_ops.hip: reid_input_kernel, reid_input_frames_kernel) at the kernel
level, on the cases of tests/resample_exact.py (proven on the CPU by tests/test_cpu_resample_exact.py).  Every test checks
  (v) float values within the DERIVED bound of the float64 reference built from exact source coordinates (resample_exact.value_bound),
  (w) float values within the tolerance the project already uses against the float32 restatement (1e-5 resize / input / posterior / conf,
      2e-6 ReID crops),
  (i) everything an index picks -- crop boxes, guidance, class map, mask -- bit for bit what the float32 rule of the oracle picks,
  (s) sentinels: pad channels of a window, slots behind the batch and the bytes behind every array are left alone.
Each test prints the largest error next to its bound before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resample_exact as K  # noqa: E402
from oracle import refinement_oracle as R  # noqa: E402

TAIL = 64                                 # elements of sentinel behind every output array
NEG = ((np.float32(0) - R.IMAGENET_RGB_MEAN) / R.IMAGENET_RGB_STD).astype(np.float32)       # a zero image, normalised


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    from premvos_amd import _lib
    return _lib, _lib.load()


def _guarded(numel, dtype, fill):
    return torch.full((numel + TAIL,), fill, dtype=dtype, device=_dev())


def _body(t, *shape):
    numel = int(np.prod(shape))
    assert t.numel() == numel + TAIL
    return t[:numel].view(*shape).cpu().numpy()


def _tail_ok(t, fill):
    return bool((t[-TAIL:] == fill).all())


def _window(x, ps):
    """float32 [n][h][w][C] -> (device buffer [n][h][w][ps] with NaN in every pad channel, channel offset of the window)."""
    n, h, w, c = x.shape
    coff = 4 if ps - c >= 4 else 0
    buf = torch.full((n, h, w, ps), float("nan"), dtype=torch.float32, device=_dev())
    buf[..., coff:coff + c] = torch.from_numpy(x).to(_dev())
    return buf, coff


# ---- A. premvos_resize_bilinear_f32 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,align", [(c, a) for c in K.RESIZE_CASES for a in c[8]],
                         ids=lambda v: "x".join(str(i) for i in v[:8]) if isinstance(v, tuple) else f"align{v}")
def test_resize_bilinear(case, align):
    _l, lib = _lib()
    n, C, h, w, ho, wo, ips, ops_ = case[:8]
    x = K.resize_data(case, align)
    xin, icoff = _window(x, ips)
    ocoff = 4 if ops_ - C >= 4 else 0
    out = _guarded(n * ho * wo * ops_, torch.float32, K.SENTINEL)
    _l.check(lib.premvos_resize_bilinear_f32(xin.data_ptr() + 4 * icoff, ips, n, h, w, C, out.data_ptr() + 4 * ocoff, ops_, ho, wo, align,
                                             _l.current_stream()), "resize_bilinear")
    torch.cuda.synchronize()
    got = _body(out, n, ho, wo, ops_)
    val = got[..., ocoff:ocoff + C]
    bound = K.resize_bound(x, ho, wo, align)
    ev = float(np.abs(val.astype(np.float64) - K.bilinear_ref(x, ho, wo, align)).max())
    ew = float(np.abs(val - K.resize_f32(x, ho, wo, align)).max())
    print(f"resize {case[:8]} align {align}: |got - exact| {ev:.3e} (bound {bound:.3e})  |got - float32 rule| {ew:.3e}")
    assert np.isfinite(val).all()                                                            # no NaN pad channel was read
    assert ev <= bound                                                                        # (v)
    assert ew <= 1e-5                                                                         # (w)
    assert (got[..., :ocoff] == K.SENTINEL).all() and (got[..., ocoff + C:] == K.SENTINEL).all() and _tail_ok(out, K.SENTINEL)   # (s)
    if (h, w) == (ho, wo):
        assert val.tobytes() == x.tobytes()                                                   # identity size: a copy
    if (h, w) == (1, 1):
        assert np.array_equal(val, np.broadcast_to(x, val.shape))                             # one source pixel: that pixel everywhere


# ---- B. premvos_broadcast_pixel_f32 ---------------------------------------------------------------------------------------------------------

def test_broadcast_pixel():
    _l, lib = _lib()
    n, C, h, w, ips, ops_ = K.BROADCAST_CASE
    x = np.random.default_rng(2000).standard_normal((n, 1, 1, C)).astype(np.float32)
    xin, icoff = _window(x, ips)
    ocoff = 4
    out = _guarded(n * h * w * ops_, torch.float32, K.SENTINEL)
    _l.check(lib.premvos_broadcast_pixel_f32(xin.data_ptr() + 4 * icoff, ips, n, C, out.data_ptr() + 4 * ocoff, ops_, h, w,
                                             _l.current_stream()), "broadcast_pixel")
    torch.cuda.synchronize()
    got = _body(out, n, h, w, ops_)
    assert np.array_equal(got[..., ocoff:ocoff + C], np.broadcast_to(x, (n, h, w, C)))
    assert (got[..., :ocoff] == K.SENTINEL).all() and (got[..., ocoff + C:] == K.SENTINEL).all() and _tail_ok(out, K.SENTINEL)


# ---- C. premvos_refine_input_u8 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.INPUT_CASES, ids=lambda c: f"S{c[0]}-{c[1]}x{c[2]}")
def test_refine_input(case):
    _l, lib = _lib()
    S, H, W, seed, boxes, kinds = case
    img = K.frame_u8(seed, H, W)
    nb, P = len(boxes), len(boxes) + 2
    d_img = torch.from_numpy(img).to(_dev())
    d_boxes = torch.tensor(list(boxes) + [(1.0, 2.0, 30.0, 40.0)] * 2, dtype=torch.float32, device=_dev())      # two live boxes behind ``count``
    d_cnt = torch.tensor([nb], dtype=torch.int32, device=_dev())
    out = _guarded(P * S * S * 4, torch.float32, K.SENTINEL)
    crops = _guarded(P * 4, torch.int32, K.SENTINEL_I32)
    _l.check(lib.premvos_refine_input_u8(d_img.data_ptr(), H, W, d_boxes.data_ptr(), d_cnt.data_ptr(), P, S, out.data_ptr(), crops.data_ptr(),
                                         _l.current_stream()), "refine_input")
    torch.cuda.synchronize()
    got, gcrops = _body(out, P, S, S, 4), _body(crops, P, 4)
    visible = 0
    for i, (b, kind) in enumerate(zip(boxes, kinds)):
        f32, crop = K.refine_input_f32(img, b, S)
        ref, _ = K.refine_input_ref(img, b, S)
        bound = K.refine_input_bound(img, b, S)
        ev = float(np.abs(got[i, ..., :3].astype(np.float64) - ref).max())
        ew = float(np.abs(got[i, ..., :3] - f32[..., :3]).max())
        print(f"refine_input S {S} box {b} ({kind}): crop {crop}  |got - exact| {ev:.3e} (bound {bound:.3e})  |got - float32 rule| {ew:.3e}")
        assert tuple(gcrops[i]) == crop == R.crop_box(b, H, W)                                # (i) the crop box
        assert np.array_equal(got[i, ..., 3], f32[..., 3])                                    # (i) the guidance, float32 rule
        assert ev <= bound and ew <= 1e-5                                                     # (v), (w)
        if kind == "empty":
            assert not got[i].any()
        else:
            assert set(np.unique(got[i, ..., 3])) <= {-1.0, 1.0}
        if kind == "zero-area":
            assert (got[i, ..., 3] == -1.0).all()
        if kind == "flip":
            exact = 2 * K.guidance01(H, W, b, S, K.exact_nearest) - 1
            visible += int((exact != f32[..., 3]).sum())
    if "flip" in kinds:
        assert visible > 0                                                                    # the exact rule would have been caught
    assert not got[nb:].any() and not gcrops[nb:].any()                                       # (s) the slots behind ``count``: zeros
    assert _tail_ok(out, K.SENTINEL) and _tail_ok(crops, K.SENTINEL_I32)


# ---- D. premvos_refine_output_f32 -----------------------------------------------------------------------------------------------------------

def _run_output(c, logits, crops, with_posterior=True, buffers=None):
    """One launch of the output layer on guarded buffers -> (buffers, mask [P][H][W], posterior, conf)."""
    _l, lib = _lib()
    P, S, H, W = c["max_boxes"], c["S"], c["H"], c["W"]
    if buffers is None:
        nbytes = int(lib.premvos_refine_output_workspace_bytes(P, S, H, W))
        buffers = dict(lg=torch.from_numpy(logits).to(_dev()),
                       crops=torch.tensor(list(crops) + [(0, 0, H, W)] * (P - len(crops)), dtype=torch.int32, device=_dev()),
                       count=torch.tensor([len(crops)], dtype=torch.int32, device=_dev()),
                       mask=_guarded(P * H * W, torch.uint8, K.SENTINEL_U8), post=_guarded(P * H * W, torch.float32, K.SENTINEL),
                       conf=_guarded(P, torch.float32, K.SENTINEL), ws=_guarded(nbytes, torch.uint8, K.SENTINEL_U8))
    b = buffers
    _l.check(lib.premvos_refine_output_f32(b["lg"].data_ptr(), c["ps"], c["lh"], c["lw"], b["crops"].data_ptr(), b["count"].data_ptr(), P, S, H, W,
                                           b["mask"].data_ptr(), b["post"].data_ptr() if with_posterior else None, b["conf"].data_ptr(),
                                           b["ws"].data_ptr(), _l.current_stream()), "refine_output")
    torch.cuda.synchronize()
    assert _tail_ok(b["mask"], K.SENTINEL_U8) and _tail_ok(b["post"], K.SENTINEL) and _tail_ok(b["conf"], K.SENTINEL)      # (s)
    assert _tail_ok(b["ws"], K.SENTINEL_U8)
    return b, _body(b["mask"], P, H, W).copy(), _body(b["post"], P, H, W).copy(), _body(b["conf"], P).copy()


def _check_output(name, c, logits, crops):
    S, H, W = c["S"], c["H"], c["W"]
    b, mask, post, conf = _run_output(c, logits, crops)
    for i, crop in enumerate(crops):
        fm, fp, exempt = K.refine_output_f32(logits[i], crop, S, H, W, c["margin"])
        ref = K.refine_output_ref(logits[i], crop, S, H, W)[0]
        bound = K.refine_output_bound(logits[i], crop, S)
        ev, ew = float(np.abs(post[i].astype(np.float64) - ref).max()), float(np.abs(post[i] - fp).max())
        ec = abs(float(conf[i]) - K.conf_ref(fm, fp))
        wrong = (mask[i] != fm) & ~exempt
        print(f"refine_output {name} crop {crop}: |post - exact| {ev:.3e} (bound {bound:.3e})  |post - float32 rule| {ew:.3e}  conf {ec:.3e}  "
              f"mask pixels off the float32 rule {int((mask[i] != fm).sum())}, exempt {int(exempt.sum())}")
        assert not wrong.any()                                                                # (i)
        assert ev <= bound and ew <= 1e-5 and ec <= 1e-5                                      # (v), (w), conf
        if crop[2] <= crop[0] or crop[3] <= crop[1]:
            assert not mask[i].any() and not post[i].any() and conf[i] == np.float32(1.0)     # an empty crop: background, sure of it
    n = len(crops)
    assert not mask[n:].any() and not post[n:].any() and not conf[n:].any()                   # (s) the slots behind ``count``
    _, mask2, post2, conf2 = _run_output(c, logits, crops, buffers=b)                         # twice on the same buffers: the same bits
    assert mask2.tobytes() == mask.tobytes() and post2.tobytes() == post.tobytes() and conf2.tobytes() == conf.tobytes()
    _, mask0, post0, conf0 = _run_output(c, logits, crops, with_posterior=False)             # posterior = NULL
    assert mask0.tobytes() == mask.tobytes() and conf0.tobytes() == conf.tobytes() and (post0 == np.float32(K.SENTINEL)).all()
    return mask, post, conf


@pytest.mark.parametrize("name", list(K.OUTPUT_CASES))
def test_refine_output(name):
    c = K.OUTPUT_CASES[name]
    logits = K.output_logits(name)
    mask, _, _ = _check_output(name, c, logits, c["crops"])
    for (case, i), count in K.MASK_FLIPS.items():
        if case == name:        # the mask the exact rule would give differs from the one the kernel gave, on as many pixels as proven on the CPU
            cls = K.class_map_f32(logits[i], c["S"])[1]
            assert int((K.uncrop_map(cls, c["crops"][i], c["H"], c["W"], K.exact_nearest) != mask[i]).sum()) == count


def test_refine_output_ties():
    """l0 == l1 everywhere: class 0 (tf.argmax takes the first) and a probability of exactly 0.5."""
    c = dict(K.OUTPUT_CASES["smooth33"], margin=None)
    logits = K.output_logits("smooth33")
    logits[..., 1] = logits[..., 0]
    mask, post, _ = _check_output("ties", c, logits, c["crops"])
    for i, (y0, x0, y1, x1) in enumerate(c["crops"]):
        inside = np.zeros(post[i].shape, bool)
        inside[y0:y1, x0:x1] = True
        assert not mask[i].any() and (post[i][inside] == np.float32(0.5)).all() and not post[i][~inside].any()


def test_refine_output_saturated_logits():
    """Logits of +-90: probabilities of exactly 0 or 1 at the logits' own pixels, nothing that is not a number anywhere."""
    c = dict(S=33, H=40, W=56, lh=33, lw=33, ps=2, max_boxes=3, margin=None)
    crops = [(3, 10, 36, 43), (0, 0, 40, 56)]                                                 # identity size; the whole frame
    yy, xx = np.mgrid[:33, :33]
    l0 = np.where(((yy // 5) + (xx // 3)) % 2 == 0, 90.0, -90.0).astype(np.float32)
    logits = np.ascontiguousarray(np.broadcast_to(np.stack([l0, -l0], -1), (3, 33, 33, 2)))
    mask, post, _ = _check_output("saturated", c, logits, crops)
    assert np.isfinite(post).all() and post.min() >= 0.0 and post.max() <= 1.0
    want = (l0 < 0).astype(np.float32)
    assert np.array_equal(post[0][3:36, 10:43], want) and np.array_equal(mask[0][3:36, 10:43], want.astype(np.uint8))


# ---- E. premvos_reid_input_u8 / premvos_reid_input_frames_u8 -------------------------------------------------------------------------------

def _reid_crops(img, boxes, zero_small):
    """premvos_reid_input_u8 on one frame -> [n][S][S][4] float32."""
    _l, lib = _lib()
    S, n = K.REID_S, len(boxes)
    H, W = img.shape[:2]
    d_img, d_boxes = torch.from_numpy(img).to(_dev()), torch.tensor(boxes, dtype=torch.int32, device=_dev())
    out = _guarded(n * S * S * 4, torch.float32, K.SENTINEL)
    _l.check(lib.premvos_reid_input_u8(d_img.data_ptr(), H, W, d_boxes.data_ptr(), n, S, zero_small, out.data_ptr(), _l.current_stream()), "reid_input")
    torch.cuda.synchronize()
    assert _tail_ok(out, K.SENTINEL)                                                          # (s)
    got = _body(out, n, S, S, 4)
    assert not got[..., 3].any()                                                              # the fourth channel is 0
    return got[..., :3]


def _check_reid(img, boxes, zero_small, got):
    for i, box in enumerate(boxes):
        bound = K.reid_bound(img, box, K.REID_S, zero_small)
        ev = float(np.abs(got[i].astype(np.float64) - K.reid_crop_ref(img, box, K.REID_S, zero_small)).max())
        ew = float(np.abs(got[i] - K.reid_crop_f32(img, box, K.REID_S, zero_small)).max())
        print(f"reid crop {box} zero_small {zero_small}: |got - exact| {ev:.3e} (bound {bound:.3e})  |got - float32 rule| {ew:.3e}")
        assert ev <= bound and ew <= 2e-6                                                     # (v), (w)


@pytest.mark.parametrize("zero_small", [1, 0])
def test_reid_bytes(zero_small):
    """Identity size, t = 0: every byte value through the scaling of its entry point, bit for bit ((b / 255 | b * (1 / 255)) - mean) / std."""
    img = K.reid_byte_frame()
    assert all(np.array_equal(np.sort(img[..., ch].ravel()), np.arange(256)) for ch in range(3))
    got = _reid_crops(img, [(0, 0, 16, 16)], zero_small)
    want = ((K.reid_bytes_f32(img, zero_small) - R.IMAGENET_RGB_MEAN) / R.IMAGENET_RGB_STD).astype(np.float32)
    other = ((K.reid_bytes_f32(img, 1 - zero_small) - R.IMAGENET_RGB_MEAN) / R.IMAGENET_RGB_STD).astype(np.float32)
    print(f"reid bytes zero_small {zero_small}: {int((got[0] != want).sum())} of 768 values off; the other scaling would be off on {int((other != want).sum())}")
    assert (other != want).any()
    assert got[0].tobytes() == want.tobytes()
    _check_reid(img, [(0, 0, 16, 16)], zero_small, got)


@pytest.mark.parametrize("zero_small", [1, 0])
def test_reid_small_and_clipped_boxes(zero_small):
    img = K.frame_u8(41, 40, 56)
    boxes = K.REID_SMALL_BOXES + K.REID_CLIP_BOXES
    got = _reid_crops(img, boxes, zero_small)
    _check_reid(img, boxes, zero_small, got)
    zero = np.broadcast_to(NEG, got[0].shape)
    for i, box in enumerate(boxes):
        blank = box[2] == 0 or (zero_small and min(box[2:]) <= 10)
        assert np.array_equal(got[i], zero) == bool(blank), box                               # min(w, h) = 10 blank, 11 a real crop; zero_small = 0: all real
    # the over-hanging boxes against plain numpy slicing: the over-hang reads nothing, the crop is that of the part inside the frame
    for i, (x, y, w, h) in enumerate(boxes):
        part = img[y:y + h, x:x + w]
        inner = (x, y, part.shape[1], part.shape[0])
        if inner != (x, y, w, h) and part.size and not (zero_small and min(inner[2:]) <= 10):
            assert np.array_equal(got[i], _reid_crops(img, [inner], zero_small)[0]), box
    big = K.frame_u8(42, 120, 200)
    _check_reid(big, [K.REID_DOWN_BOX], zero_small, _reid_crops(big, [K.REID_DOWN_BOX], zero_small))


@pytest.mark.parametrize("zero_small", [1, 0])
def test_reid_frames_form(zero_small):
    """The slots of several frames in one launch: bit for bit the one-frame entry point per (frame, box); padded slots (a frame index
    outside [0, F), the empty box) are a zero image, normalised."""
    _l, lib = _lib()
    S, F, H, W = K.REID_S, 3, 40, 56
    frames = np.stack([K.frame_u8(50 + f, H, W) for f in range(F)])
    boxes = K.REID_SMALL_BOXES + K.REID_CLIP_BOXES[:2] + [(0, 0, 0, 0), (0, 0, 0, 0)]
    fos = [0, 1, 2, 0, 1, 2, -1, 3]
    assert len(boxes) == len(fos) == 8
    n = len(boxes)
    d_frames = torch.from_numpy(frames).to(_dev())
    d_boxes, d_fos = torch.tensor(boxes, dtype=torch.int32, device=_dev()), torch.tensor(fos, dtype=torch.int32, device=_dev())
    out = _guarded(n * S * S * 4, torch.float32, K.SENTINEL)
    _l.check(lib.premvos_reid_input_frames_u8(d_frames.data_ptr(), F, H, W, d_fos.data_ptr(), d_boxes.data_ptr(), n, S, zero_small, out.data_ptr(),
                                              _l.current_stream()), "reid_input_frames")
    torch.cuda.synchronize()
    got = _body(out, n, S, S, 4)
    assert _tail_ok(out, K.SENTINEL) and not got[..., 3].any()
    for f in range(F):
        idx = [i for i in range(n) if fos[i] == f]
        one = _reid_crops(frames[f], [boxes[i] for i in idx], zero_small)
        assert got[idx][..., :3].tobytes() == one.tobytes()
        _check_reid(frames[f], [boxes[i] for i in idx], zero_small, got[idx][..., :3])
    assert np.array_equal(got[6:, ..., :3], np.broadcast_to(NEG, (2, S, S, 3)))
