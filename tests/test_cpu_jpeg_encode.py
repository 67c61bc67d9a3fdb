"""GPU baseline JPEG encoder, the parts that need no GPU:
  * tests/jpeg_forward_restated.py (pixels -> quantised coefficients, written from the published rules) pinned against the
    coefficients the library itself writes (libjpeg-turbo inside PIL), read back with oracle/jpeg_oracle.entropy_decode: equal;
  * the host half of the C-ABI (premvos_jpeg_entropy_encode_host: markers + Huffman coding) against PIL's file, byte for byte,
    its buffer bound and its refusals;
  * header / binding agreement of the three new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_forward_restated as R
from oracle import jpeg_oracle as jo
from test_cpu_jpeg import jpeg_bytes, picture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
SIZES = [(1, 1), (8, 5), (9, 7), (16, 17), (17, 16), (37, 53), (41, 23), (48, 64)]        # (h, w)
OTHER_QUALITY = {(1, 1): 75, (8, 5): 100, (9, 7): 30, (16, 17): 90, (17, 16): 75, (37, 53): 100, (41, 23): 10, (48, 64): 75}


def random_pixels(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def info_for(h, w, quality, subsampling):
    """The info block of an h x w frame: premvos_jpeg_forward_u8 without a coefficient buffer touches no GPU."""
    from premvos_amd import _lib, jpeg
    info = jpeg.JpegInfo()
    ql, qc = jpeg.quant_tables(quality)
    hs, vs = jpeg.SAMPLING[subsampling]
    rc = _lib.load().premvos_jpeg_forward_u8(None, None, None, h, w, ql.ctypes.data, qc.ctypes.data, hs, vs, C.byref(info), None, 0, None)
    assert rc == 0, _lib.load().premvos_last_error()
    return info


def host_encode(coef, h, w, quality, subsampling, capacity=None, guard=0):
    """premvos_jpeg_entropy_encode_host on per-component coefficient arrays -> (status, bytes written, the whole buffer)."""
    from premvos_amd import _lib
    info = info_for(h, w, quality, subsampling)
    flat = np.concatenate([np.ascontiguousarray(c, np.int16).reshape(-1) for c in coef])
    assert flat.size == info.coef_count and [info.coef_offset[c] for c in range(3)] == list(np.cumsum([0] + [c.size for c in coef])[:3])
    capacity = 2 * flat.size + 4096 if capacity is None else capacity
    buf = np.full(capacity + guard, 0xA5, np.uint8)
    n = C.c_int64(-1)
    rc = _lib.load().premvos_jpeg_entropy_encode_host(flat.ctypes.data, C.byref(info), buf.ctypes.data, capacity, C.byref(n))
    return rc, n.value, buf


@pytest.mark.parametrize("h,w", SIZES)
def test_restatement_equals_the_library_and_the_host_pass_writes_its_file(h, w):
    for quality in (95, OTHER_QUALITY[(h, w)]):
        for sub in ("4:2:0", "4:2:2", "4:4:4"):
            for im in (picture(h, w, seed=h + w), random_pixels(h, w, seed=100 * h + w + quality)):
                data = jpeg_bytes(im, quality=quality, subsampling=PIL_SUBSAMPLING[sub])
                f = jo.parse(data)
                want = jo.entropy_decode(f)
                got = R.forward(im, quality, sub)
                for c in range(3):
                    assert got[c].shape == want[c].shape and got[c].dtype == np.int16
                    assert np.array_equal(got[c], want[c]), (quality, sub, c, int((got[c] != want[c]).sum()))
                rc, n, buf = host_encode(got, h, w, quality, sub)
                assert rc == 0 and bytes(buf[:n]) == data, (quality, sub)


@pytest.mark.parametrize("quality", [1, 10, 49, 50, 75, 95, 100])
def test_quant_tables_are_jpeg_set_quality(quality):
    from premvos_amd import jpeg
    f = jo.parse(jpeg_bytes(picture(8, 8), quality=quality, subsampling=2))
    for mine in (jpeg.quant_tables(quality), R.quant_tables(quality)):
        assert np.array_equal(mine[0], f["qt"][0]) and np.array_equal(mine[1], f["qt"][1])


def _scan(data):
    return data[data.index(b"\xff\xda") + 14:-2]


def test_longest_codes_zero_runs_flat_blocks_and_byte_stuffing():
    y, x = np.mgrid[0:24, 0:40]
    checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)       # the largest values a block can hold
    faint = (120 + checker // 255 * 16).astype(np.uint8)                                      # only coefficient 63 survives: ZRL x 3
    flat = np.full((21, 35, 3), (200, 40, 90), np.uint8)                                      # EOB only; dummy blocks repeat the DC
    noisy = random_pixels(40, 56, seed=7)                                                     # 16-bit codes + 10-bit values
    for im, quality, sub in ((checker, 100, "4:2:0"), (checker, 95, "4:4:4"), (faint, 50, "4:4:4"), (flat, 95, "4:2:0"),
                             (flat, 75, "4:2:2"), (noisy, 100, "4:2:0"), (noisy, 100, "4:4:4")):
        data = jpeg_bytes(im, quality=quality, subsampling=PIL_SUBSAMPLING[sub])
        coef = R.forward(im, quality, sub)
        if im is checker and quality == 100:
            assert np.abs(coef[0]).max() > 511                                                # 10 value bits
        if im is faint:
            assert all(list(np.flatnonzero(b[jo.ZIGZAG][1:])) == [62] for b in coef[0].reshape(-1, 64))     # 62 zeros in a row
        if im is flat:
            assert all(not c[..., 1:].any() for c in coef) and len(_scan(data)) < 40
        if im is noisy:
            assert b"\xff\x00" in _scan(data)                                                 # the scan does contain stuffed bytes
        rc, n, buf = host_encode(coef, im.shape[0], im.shape[1], quality, sub)
        assert rc == 0 and bytes(buf[:n]) == data


def test_a_short_output_buffer_is_refused_and_never_overrun():
    from premvos_amd import _lib, jpeg
    im = random_pixels(33, 47, seed=3)
    data = jpeg_bytes(im, quality=95, subsampling=2)
    coef = R.forward(im, 95, "4:2:0")
    rc, n, buf = host_encode(coef, 33, 47, 95, "4:2:0", capacity=len(data), guard=64)         # exactly enough
    assert rc == 0 and n == len(data) and bytes(buf[:n]) == data and (buf[n:] == 0xA5).all()
    for cap in (len(data) - 1, len(data) - 2, 700, 100, 1, 0):                                # in the EOI, the scan, the tables, ...
        rc, n, buf = host_encode(coef, 33, 47, 95, "4:2:0", capacity=cap, guard=64)
        assert rc == jpeg.ENOSPACE == -4 and n == 0, cap
        assert b"buffer" in _lib.load().premvos_last_error()
        assert (buf[cap:] == 0xA5).all(), cap                                                 # the guard bytes behind the buffer
        assert bytes(buf[:cap]) == data[:cap]                                                 # (what did fit is the file's head)


def test_host_pass_refuses_bad_arguments():
    from premvos_amd import _lib
    lib = _lib.load()
    info = info_for(16, 16, 95, "4:2:0")
    coef = np.zeros(info.coef_count, np.int16)
    out = np.zeros(4096, np.uint8)
    n = C.c_int64(0)
    f = lib.premvos_jpeg_entropy_encode_host
    assert f(None, C.byref(info), out.ctypes.data, 4096, C.byref(n)) == -1 and b"null" in lib.premvos_last_error()
    assert f(coef.ctypes.data, C.byref(info), None, 4096, C.byref(n)) == -1 and b"null" in lib.premvos_last_error()
    assert f(coef.ctypes.data, C.byref(info), out.ctypes.data, 4096, None) == -1 and b"null" in lib.premvos_last_error()
    bad = info_for(16, 16, 95, "4:2:0")
    bad.mcux = 7
    assert f(coef.ctypes.data, C.byref(bad), out.ctypes.data, 4096, C.byref(n)) == -1 and b"geometry" in lib.premvos_last_error()
    coef[0] = 2048                                                                            # a DC difference of 12 bits
    assert f(coef.ctypes.data, C.byref(info), out.ctypes.data, 4096, C.byref(n)) == -1 and b"baseline" in lib.premvos_last_error()
    # the device entry points check their arguments before any HIP call
    one = out.ctypes.data
    assert lib.premvos_overlay_blend_u8(None, one, one, 4, 4, one, None) == -1 and b"null" in lib.premvos_last_error()
    assert lib.premvos_overlay_blend_u8(one, one, one, 0, 4, one, None) == -1
    q = np.ones(64, np.uint16)
    g = lib.premvos_jpeg_forward_u8
    assert g(one, None, None, 4, 4, q.ctypes.data, q.ctypes.data, 1, 2, C.byref(info), None, 0, None) == -1 and b"sampling" in lib.premvos_last_error()
    assert g(one, one, None, 4, 4, q.ctypes.data, q.ctypes.data, 2, 2, C.byref(info), None, 0, None) == -1 and b"palette" in lib.premvos_last_error()
    assert g(one, None, None, 4, 4, (q * 256).ctypes.data, q.ctypes.data, 2, 2, C.byref(info), None, 0, None) == -1
    assert g(one, None, None, 4, 4, q.ctypes.data, q.ctypes.data, 2, 2, C.byref(info), one, 10, None) == -1 and b"holds" in lib.premvos_last_error()


def test_info_block_of_the_forward_entry_is_the_decoders():
    """The geometry premvos_jpeg_forward_u8 fills in is what premvos_jpeg_entropy_decode_host reads from PIL's file."""
    from premvos_amd import jpeg
    for (h, w), sub in (((37, 53), "4:2:0"), ((17, 16), "4:2:2"), ((9, 7), "4:4:4"), ((480, 854), "4:2:0")):
        mine = info_for(h, w, 90, sub)
        ref = jpeg.header(jpeg_bytes(picture(h, w), quality=90, subsampling=PIL_SUBSAMPLING[sub]))
        assert bytes(mine) == bytes(ref)


def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name, nargs, src in (("premvos_overlay_blend_u8", 7, "jpeg_enc_ops.hip"), ("premvos_jpeg_forward_u8", 13, "jpeg_enc_ops.hip"),
                             ("premvos_jpeg_entropy_encode_host", 5, "host_files.hip")):
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
        assert f'extern "C" int {name}(' in open(os.path.join(ROOT, "premvos_amd", "csrc", src)).read()
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    for cite in ("merge_functions.py:527-545", "jccolor.c", "jcsample.c", "jfdctint.c", "jcdctmgr.c", "jccoefct.c", "jchuff.c", "jcmarker.c"):
        assert cite in hdr
    assert "PREMVOS_ENOSPACE (-4)" in hdr


# ------------------------------------------------------------------------------------------------------------- the command lines
def test_overlay_flag_is_refused_where_track_is(monkeypatch):
    from premvos_amd import stream
    monkeypatch.delenv("PREMVOS_SIDECAR", raising=False)
    a = stream.parse_args(["--track", "--overlay"])
    assert a.track and a.overlay and a.reid and not stream.parse_args(["--track"]).overlay
    for argv, why in ((["--overlay"], stream.REFUSE_OVERLAY_WITHOUT_TRACK), (["--reid", "--overlay"], stream.REFUSE_OVERLAY_WITHOUT_TRACK),
                      (["--track", "--overlay", "--gather"], stream.REFUSE_OVERLAY_GATHER)):
        with pytest.raises(SystemExit) as e:
            stream.parse_args(argv)
        assert str(e.value) == why and why.startswith("premvos_amd.stream: --overlay") and "--track" in why
    monkeypatch.setenv("PREMVOS_SIDECAR", "1")
    with pytest.raises(SystemExit) as e:
        stream.parse_args(["--track", "--overlay"])
    assert str(e.value) == stream.REFUSE_OVERLAY_SIDECAR and "PREMVOS_SIDECAR" in str(e.value)
    with pytest.raises(SystemExit) as e:                                                      # without the flag: the refusal it always was
        stream.parse_args(["--track"])
    assert str(e.value) == stream.REFUSE_TRACK_SIDECAR


def test_overlay_command_names_what_is_missing(tmp_path, capsys):
    from PIL import Image
    from premvos_amd import overlay
    assert overlay.main(["--root", str(tmp_path), "--check-only"]) == 2
    out = capsys.readouterr().out
    assert "inputs are not ready" in out and "JPEGImages/480p is missing" in out and "output/final is missing" in out and "premvos_amd.track" in out
    (tmp_path / "data" / "DAVIS" / "JPEGImages" / "480p" / "bear").mkdir(parents=True)
    (tmp_path / "output" / "final" / "bear").mkdir(parents=True)
    Image.fromarray(np.zeros((8, 8), np.uint8)).save(tmp_path / "output" / "final" / "bear" / "00000.png")
    assert overlay.main(["--root", str(tmp_path), "--check-only"]) == 2
    assert "bear/00000.jpg is missing" in capsys.readouterr().out
    assert overlay.main(["--root", str(tmp_path), "--videos", "camel", "--check-only"]) == 2
    assert "final/camel is missing" in capsys.readouterr().out
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "data" / "DAVIS" / "JPEGImages" / "480p" / "bear" / "00000.jpg")
    assert overlay.main(["--root", str(tmp_path), "--check-only"]) == 0
    assert "inputs are in place" in capsys.readouterr().out
