"""GPU baseline JPEG encoder and the overlay pictures built on it: premvos_jpeg_forward_u8 / premvos_overlay_blend_u8 against
tests/jpeg_forward_restated.py (pinned to the library in tests/test_cpu_jpeg_encode.py), whole files against PIL's -- all byte
for byte -- and ``--overlay`` of premvos_amd.track and premvos_amd.stream --track against PIL.save of the numpy blend."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_forward_restated as R
from test_cpu_jpeg import jpeg_bytes, picture, pil_rgb
from test_cpu_jpeg_encode import PIL_SUBSAMPLING, random_pixels

pytestmark = pytest.mark.gpu

# (h, w): a lone partial MCU, a dummy block row (17 rows: luma block row 3 of 4), a dummy block column, a clean multiple
SHAPES = [(9, 7, "4:2:0"), (17, 16, "4:2:0"), (37, 53, "4:2:0"), (48, 64, "4:2:0"), (37, 53, "4:2:2"), (17, 16, "4:4:4")]


def coefficients(e):
    """An ``Encoded`` -> the three components' arrays (waits for the copy; does not consume it)."""
    e.ready.synchronize()
    flat, I = e.coef.numpy(), e.info
    return [flat[I.coef_offset[c]:I.coef_offset[c] + I.blocks_h[c] * I.blocks_w[c] * 64].reshape(I.blocks_h[c], I.blocks_w[c], 64).copy()
            for c in range(3)]


def same(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("h,w,sub", SHAPES)
def test_forward_and_file_equal_the_restatement_and_the_library(h, w, sub):
    from premvos_amd import jpeg
    for im, quality in ((picture(h, w, seed=h + w), 95), (random_pixels(h, w, seed=h * w), 75)):
        dev = torch.from_numpy(im).cuda()
        assert same(coefficients(jpeg.forward(dev, quality, sub)), R.forward(im, quality, sub)), quality
        data = jpeg_bytes(im, quality=quality, subsampling=PIL_SUBSAMPLING[sub])
        mine = jpeg.encode(dev, quality, sub)
        assert mine == data
        assert np.array_equal(jpeg.decode(mine).cpu().numpy(), pil_rgb(data))


def test_forward_full_size_frame():
    """480 x 854: the strip raster (7 strips of 8 MCUs per MCU row) and the 854 = 53 x 16 + 6 tail exist only here."""
    from premvos_amd import jpeg, synth
    im = np.ascontiguousarray(synth.video_frames(1, 480, 856)[0][0].cpu().numpy()[:, :854, :3])      # the bench's synthetic video
    frame = torch.from_numpy(im)
    assert same(coefficients(jpeg.forward(frame.cuda())), R.forward(im, 95, "4:2:0"))
    assert jpeg.encode(frame.cuda()) == jpeg_bytes(im, quality=95, subsampling=2)


def test_blend_kernel_and_the_fused_path():
    from premvos_amd import jpeg, overlay
    from premvos_amd.track import voc_palette
    h, w = 37, 53
    im = picture(h, w, seed=5)
    ids = np.zeros((h, w), np.uint8)
    ids[3:20, 5:30], ids[15:37, 25:53], ids[0:9, 40:53] = 1, 7, 255
    assert set(np.unique(ids)) == {0, 1, 7, 255}
    pal = voc_palette()
    want = R.blend(im, ids, pal)
    assert np.array_equal(want[ids == 0], im[ids == 0]) and not np.array_equal(want, im)
    assert np.array_equal(want[ids == 7][0], ((im[ids == 7][0].astype(np.float64) * 0.5 + pal[7] * 0.5)).astype(np.uint8))    # draw_mask
    f, m = torch.from_numpy(im).cuda(), torch.from_numpy(ids).cuda()
    got = overlay.blend(f, m)
    assert np.array_equal(got.cpu().numpy(), want)
    for sub in ("4:2:0", "4:2:2", "4:4:4"):
        fused = coefficients(jpeg.forward(f, 95, sub, idmap=m, palette=overlay.palette(f.device)))
        assert same(fused, coefficients(jpeg.forward(got, 95, sub))) and same(fused, R.forward(want, 95, sub))
    assert jpeg.entropy_encode(overlay.forward(f, m)) == jpeg_bytes(want, quality=95, subsampling=2)
    assert jpeg.entropy_encode(overlay.forward(f, None)) == jpeg_bytes(im, quality=95, subsampling=2)


# ------------------------------------------------------------------------------------------------- --overlay of the two drivers
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEOS = {"bear": 4, "camel": 3}                                    # bear: two annotated objects; camel: none (plain frames)


def _files(base):
    return sorted(str(p.relative_to(base)) for p in base.rglob("*") if p.is_file())


def _check_overlays(root):
    """Every output/overlay file is PIL.save(numpy blend of the frame and the final PNG), and there is one per frame."""
    from premvos_amd.track import voc_palette
    final, over, images = root / "output" / "final", root / "output" / "overlay", root / "data" / "DAVIS" / "JPEGImages" / "480p"
    assert _files(over) == [f"{v}/{t:05d}.jpg" for v, n in sorted(VIDEOS.items()) for t in range(n)]
    tinted = 0
    for rel in _files(over):
        frame = np.array(Image.open(images / rel).convert("RGB"))
        ids = np.array(Image.open(final / (rel[:-4] + ".png")))
        want = io.BytesIO()
        Image.fromarray(R.blend(frame, ids, voc_palette())).save(want, "JPEG", quality=95, subsampling=2)
        assert (over / rel).read_bytes() == want.getvalue(), rel
        tinted += int(ids.any())
    assert tinted >= 1                                               # (some frame does carry an object: the blend was exercised)


@pytest.fixture(scope="module")
def two_program_tree(tmp_path_factory):
    """`stream --reid`, `track` (the final PNGs kept aside), then `track --overlay` over them: each a child under its own limit."""
    import shutil
    from test_gpu_stream_track import T, _child, _tree
    root = tmp_path_factory.mktemp("overlay") / "a"
    _tree(root, VIDEOS)
    _child("premvos_amd.stream", root, "--batch", "2", "--reid", *T.STREAM_ARGS, timeout=600)
    _child("premvos_amd.track", root, timeout=300)
    shutil.copytree(root / "output" / "final", root / "final_without_the_flag")
    before = {f: (root / "output" / f).read_bytes() for f in _files(root / "output")}
    out = _child("premvos_amd.track", root, "--overlay", timeout=300).stdout
    assert "output/overlay" in out
    return root, before


def test_track_overlay_writes_pil_bytes_and_leaves_every_other_file_alone(two_program_tree):
    root, before = two_program_tree
    _check_overlays(root)
    plain, final = root / "final_without_the_flag", root / "output" / "final"
    assert _files(plain) == _files(final) and all((plain / f).read_bytes() == (final / f).read_bytes() for f in _files(plain))
    after = {f: (root / "output" / f).read_bytes() for f in _files(root / "output") if not f.startswith("overlay/")}
    assert after == before


def test_stream_track_overlay_equals_track_overlay(two_program_tree, tmp_path):
    from test_gpu_stream_track import T, _child, _tree
    a, _ = two_program_tree
    b = tmp_path / "b"
    _tree(b, VIDEOS)
    assert "frames: 7" in _child("premvos_amd.stream", b, "--batch", "2", "--track", "--overlay", *T.STREAM_ARGS, timeout=600).stdout
    _check_overlays(b)
    for sub in ("intermediate", "final", "overlay"):                 # (stream --track without the flag = the two-program path:
        fa, fb = _files(a / "output" / sub), _files(b / "output" / sub)      # tests/test_gpu_stream_track.py)
        assert fa == fb, sub
        for f in fa:
            assert (a / "output" / sub / f).read_bytes() == (b / "output" / sub / f).read_bytes(), (sub, f)
