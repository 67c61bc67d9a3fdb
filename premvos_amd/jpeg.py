"""Optional GPU JPEG decode (``PREMVOS_GPU_JPEG=1``): the frame a stage reads arrives in HBM as the bytes
its reference reader would have produced -- ``cv2.imread`` (proposal_net/train.py:500, BGR), ``scipy.ndimage.imread`` = PIL
(optical_flow_net-PWC-Net/script_pwc_multi.py:34) or PIL (ReID_net/prepare_input.py:38) -- without the CPU running the inverse
DCT, the chroma up-sampling and the colour conversion, and with ONE upload per frame for all stages.

Two halves, matching the C-ABI (include/premvos_hip.h, csrc/jpeg_ops.hip):

  ``host_stage(fn_or_bytes)``   marker parsing + Huffman decoding on a host thread (plain C++, the GIL is released during
                                the call; the bit stream is serial) into pinned quantised coefficients;
  ``device_stage(decoded)``     upload + ``premvos_jpeg_reconstruct_u8`` on the current HIP stream -> uint8 [H,W,3] in HBM.

Files the decoder does not cover (progressive, arithmetic-coded, 12-bit, CMYK / RGB-coded, multi-scan, 4:4:0 / 4:1:1) keep the
default reader: ``host_stage`` returns the PIL-decoded array for them and ``device_stage`` uploads it.  The default of every
driver is unchanged (PIL on the host); this is the optional fast path SURVEY asks to keep optional.

The mirror image, for pictures that are made in HBM (premvos_amd.overlay): ``forward(rgb)`` (``premvos_jpeg_forward_u8``: colour
conversion, down-sampling, forward DCT, quantisation -> coefficients on their way into a pinned buffer), ``entropy_encode(encoded)``
(``premvos_jpeg_entropy_encode_host``: markers + Huffman coding on a host thread) and ``encode`` = both: the file PIL writes.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, List, Tuple, Union

import numpy as np
import torch

from . import _lib

EUNSUPPORTED = -3


class JpegInfo(C.Structure):
    """premvos_jpeg_info of include/premvos_hip.h."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32),
                ("mcux", C.c_int32), ("mcuy", C.c_int32), ("blocks_w", C.c_int32 * 3), ("blocks_h", C.c_int32 * 3),
                ("reserved", C.c_int32), ("coef_offset", C.c_int64 * 3), ("coef_count", C.c_int64),
                ("quant", (C.c_uint16 * 64) * 3)]


class Unsupported(ValueError):
    """A valid JPEG outside what the GPU decoder covers."""


def enabled(default: str = "0") -> bool:
    """PREMVOS_GPU_JPEG=1 / 0; unset: ``default`` (the stage drivers keep the library reader of the reference's scripts, the
    streaming driver turns the GPU path on -- same bytes either way, tests/test_gpu_jpeg.py)."""
    return os.environ.get("PREMVOS_GPU_JPEG", default) not in ("", "0")


class _PinnedPool:
    """Pinned int16 staging buffers, reused once the upload that read them has finished."""

    def __init__(self):
        self.lock = threading.Lock()
        self.free: Dict[int, List[Tuple[torch.Tensor, object]]] = {}

    def get(self, count: int) -> torch.Tensor:
        size = max(1 << 16, 1 << (int(count) - 1).bit_length())
        with self.lock:
            lst = self.free.get(size, [])
            for i, (t, ev) in enumerate(lst):
                if ev is None or ev.query():
                    lst.pop(i)
                    return t
        pin = torch.cuda.is_available()
        return torch.empty(size, dtype=torch.int16, pin_memory=pin)

    def put(self, t: torch.Tensor, ev) -> None:
        with self.lock:
            lst = self.free.setdefault(t.numel(), [])
            if len(lst) < 64:
                lst.append((t, ev))


_POOL = _PinnedPool()


class Decoded:
    """The host half's result: geometry / tables and the quantised coefficients in a pinned buffer."""
    __slots__ = ("info", "coef")

    def __init__(self, info: JpegInfo, coef: torch.Tensor):
        self.info, self.coef = info, coef

    @property
    def shape(self) -> Tuple[int, int, int]:
        return (self.info.height, self.info.width, 3)


def _read(src: Union[str, bytes, bytearray, memoryview]) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def header(data: bytes) -> JpegInfo:
    info = JpegInfo()
    rc = _lib.load().premvos_jpeg_entropy_decode_host(data, len(data), C.byref(info), None, 0)
    if rc == EUNSUPPORTED:
        raise Unsupported(_lib.load().premvos_last_error().decode())
    _lib.check(rc, "premvos_jpeg_entropy_decode_host")
    return info


def entropy_decode(data: bytes) -> Decoded:
    """Huffman-decode a baseline JPEG on the host.  Raises ``Unsupported`` for files the decoder does not cover."""
    lib = _lib.load()
    info = header(data)
    coef = _POOL.get(info.coef_count)
    rc = lib.premvos_jpeg_entropy_decode_host(data, len(data), C.byref(info), coef.data_ptr(), coef.numel())
    if rc != 0:
        _POOL.put(coef, None)
        _lib.check(rc, "premvos_jpeg_entropy_decode_host")
    return Decoded(info, coef)


def reconstruct(d: Decoded, device=None, bgr: bool = False) -> torch.Tensor:
    """Upload the coefficients and run the two kernels on the current stream of ``device``: uint8 [H,W,3]."""
    device = _lib.resolve_device(device)
    _lib.require_gpu()
    lib, info = _lib.load(), d.info
    if d.coef is None:
        raise ValueError("this frame's coefficients were already handed to the GPU (reconstruct() consumes a Decoded)")
    n = int(info.coef_count)
    coef_dev = torch.empty(n, dtype=torch.int16, device=device)
    coef_dev.copy_(d.coef[:n], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _POOL.put(d.coef, ev)
    d.coef = None
    ws = torch.empty(max(8, lib.premvos_jpeg_workspace_bytes(C.byref(info))), dtype=torch.uint8, device=device)
    out = torch.empty((info.height, info.width, 3), dtype=torch.uint8, device=device)
    _lib.check(lib.premvos_jpeg_reconstruct_u8(coef_dev.data_ptr(), C.byref(info), ws.data_ptr(), out.data_ptr(), int(bool(bgr)),
                                               _lib.current_stream()), "premvos_jpeg_reconstruct_u8")
    return out


def decode(data: bytes, device=None, bgr: bool = False) -> torch.Tensor:
    return reconstruct(entropy_decode(data), device, bgr)


# ---- the encoder: the mirror image (csrc/jpeg_enc_ops.hip on the device, premvos_jpeg_entropy_encode_host on the host) -----------
ENOSPACE = -4
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# T.81 annex K.1 / K.2 (natural order), the tables jpeg_set_quality scales
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
              100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
                99) + (99,) * 32


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """jcparam.c jpeg_set_quality(quality, force_baseline=TRUE): the luma and chroma tables, uint16 [64] in natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(b, np.int64) * scale + 50) // 100, 1, 255).astype(np.uint16) for b in (_BASE_LUMA, _BASE_CHROMA))


class Encoded:
    """The device half's result: geometry / tables, and the quantised coefficients on their way into a pinned host buffer
    (``ready``: the event behind the copy)."""
    __slots__ = ("info", "coef", "ready")

    def __init__(self, info: JpegInfo, coef: torch.Tensor, ready):
        self.info, self.coef, self.ready = info, coef, ready


def forward(rgb: torch.Tensor, quality: int = 95, subsampling: str = "4:2:0", idmap: torch.Tensor = None,
            palette: torch.Tensor = None) -> Encoded:
    """uint8 [H,W,3] RGB in HBM -> quantised coefficients (``premvos_jpeg_forward_u8`` on the current stream, then an asynchronous
    copy into a pinned buffer).  With ``idmap`` (uint8 [H,W]) and ``palette`` (uint8 [256,3]), both in HBM, the picture encoded is
    ``overlay.blend(rgb, idmap, palette)`` -- blended while the kernel loads its pixels, never stored."""
    _lib.require_gpu()
    if subsampling not in SAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: one of {sorted(SAMPLING)}")
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or not rgb.is_cuda:
        raise ValueError("forward() takes a uint8 [H,W,3] tensor in HBM")
    if (idmap is None) != (palette is None):
        raise ValueError("idmap and palette come together")
    lib, rgb = _lib.load(), rgb.contiguous()
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    if idmap is not None:
        if idmap.dtype != torch.uint8 or tuple(idmap.shape) != (h, w) or idmap.device != rgb.device:
            raise ValueError("idmap: a uint8 [H,W] tensor on the frame's device")
        if palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3) or palette.device != rgb.device:
            raise ValueError("palette: a uint8 [256,3] tensor on the frame's device")
        idmap, palette = idmap.contiguous(), palette.contiguous()
    (hs, vs), (ql, qc) = SAMPLING[subsampling], quant_tables(quality)
    info = JpegInfo()
    args = (rgb.data_ptr(), idmap.data_ptr() if idmap is not None else None, palette.data_ptr() if palette is not None else None,
            h, w, ql.ctypes.data, qc.ctypes.data, hs, vs, C.byref(info))
    _lib.check(lib.premvos_jpeg_forward_u8(*args, None, 0, None), "premvos_jpeg_forward_u8")
    n = int(info.coef_count)
    with torch.cuda.device(rgb.device):
        coef_dev = torch.empty(n, dtype=torch.int16, device=rgb.device)
        _lib.check(lib.premvos_jpeg_forward_u8(*args, coef_dev.data_ptr(), n, _lib.current_stream()), "premvos_jpeg_forward_u8")
        host = _POOL.get(n)
        host[:n].copy_(coef_dev, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record()
    return Encoded(info, host, ready)


def entropy_encode(e: Encoded) -> bytes:
    """The host half: wait for the coefficients, Huffman-code them (plain C, the GIL is released during the call) -> the file."""
    if e.coef is None:
        raise ValueError("this frame's coefficients were already encoded (entropy_encode() consumes an Encoded)")
    lib, n = _lib.load(), int(e.info.coef_count)
    if e.ready is not None:
        e.ready.synchronize()
    written = C.c_int64(0)
    try:
        for cap in (2 * n + 4096, 8 * n + 4096):         # (a coefficient costs at most 26 bits, 52 with every byte stuffed)
            out = np.empty(cap, np.uint8)
            rc = lib.premvos_jpeg_entropy_encode_host(e.coef.data_ptr(), C.byref(e.info), out.ctypes.data, cap, C.byref(written))
            if rc != ENOSPACE:
                break
        _lib.check(rc, "premvos_jpeg_entropy_encode_host")
    finally:
        _POOL.put(e.coef, None)
        e.coef = None
    return out[:written.value].tobytes()


def encode(rgb: torch.Tensor, quality: int = 95, subsampling: str = "4:2:0", idmap: torch.Tensor = None,
           palette: torch.Tensor = None) -> bytes:
    """The bytes ``PIL.Image.save(f, "JPEG", quality=quality, subsampling=subsampling)`` writes for the same pixels."""
    return entropy_encode(forward(rgb, quality, subsampling, idmap, palette))


# ---- the two halves as the drivers use them -------------------------------------------------------------------------------
def _pil_rgb(src) -> np.ndarray:
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(src) if isinstance(src, (bytes, bytearray)) else src)
    return np.array(im.convert("RGB"))[:, :, :3]        # (a writable copy: torch.from_numpy wants one)


def host_stage(src: Union[str, bytes]) -> Union[Decoded, np.ndarray]:
    """What a decode-ahead thread does for one frame: the entropy decode (GPU path) or, for a file the GPU decoder does not cover
    (and for anything that is not a JPEG), the default reader's RGB array."""
    data = _read(src)
    if data[:2] != b"\xff\xd8":
        return _pil_rgb(data)
    try:
        return entropy_decode(data)
    except Unsupported:
        return _pil_rgb(data)


def device_stage(item: Union[Decoded, np.ndarray], device=None, bgr: bool = False) -> torch.Tensor:
    """uint8 [H,W,3] in HBM on the current stream, RGB (or BGR, the cv2.imread order)."""
    if isinstance(item, Decoded):
        return reconstruct(item, device, bgr)
    t = torch.from_numpy(item).to(_lib.resolve_device(device))
    return t.flip(2).contiguous() if bgr else t


def imread(src: Union[str, bytes], device=None, bgr: bool = False) -> torch.Tensor:
    return device_stage(host_stage(src), device, bgr)


def to_device(item, device=None, bgr: bool = False) -> torch.Tensor:
    """One frame as the drivers hold it -- a host RGB array, a ``Decoded`` (entropy-decoded, not yet reconstructed) or a uint8 tensor
    already in HBM -- as uint8 [H,W,3] on ``device`` (current stream)."""
    if isinstance(item, torch.Tensor):
        t = item if item.is_cuda else item.to(_lib.resolve_device(device))
        if item.is_cuda:
            # decoded on another stream (and complete: its producer synchronised); tell the allocator this stream reads it too,
            # so the block is not handed out again while a kernel of this stream is still in flight
            item.record_stream(torch.cuda.current_stream(item.device))
        return t.flip(2).contiguous() if bgr else t
    if isinstance(item, Decoded):
        return reconstruct(item, device, bgr)
    return device_stage(np.array(item[:, :, :3], dtype=np.uint8, order="C"), device, bgr)


def stack_frames(items, device=None, bgr: bool = False) -> torch.Tensor:
    """Frames of equal size -> uint8 [n,H,W,3] on ``device``: ONE upload for host arrays, the GPU decode for ``Decoded`` items."""
    items = list(items)
    if all(isinstance(i, np.ndarray) for i in items):
        t = torch.from_numpy(np.stack([np.array(i[:, :, :3], dtype=np.uint8, order="C") for i in items])).to(_lib.resolve_device(device))
        return t.flip(3).contiguous() if bgr else t
    return torch.stack([to_device(i, device, bgr) for i in items])


def loader(default: str = "0"):
    """The per-frame function of a driver's decode-ahead pool: file name -> host RGB array (default) or, with PREMVOS_GPU_JPEG=1,
    the entropy-decoded frame for ``stack_frames`` / ``to_device`` to finish on the GPU."""
    return host_stage if enabled(default) else _pil_rgb
