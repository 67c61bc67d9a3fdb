"""TEST INFRASTRUCTURE ONLY: numpy restatement of the forward half of a baseline JPEG encoder, pixels -> quantised coefficients,
next to davis_restated.py and track_restated.py.

Written from the published rules of the libjpeg compressor (jccolor.c colour conversion, jcprepct.c / jcsample.c edge expansion
and down-sampling, jfdctint.c forward DCT, jcdctmgr.c quantisation, jccoefct.c dummy blocks of an edge MCU), NOT from library
source; tests/test_cpu_jpeg_encode.py pins it against the coefficients the library itself writes (PIL's libjpeg-turbo, read back
with oracle/jpeg_oracle.entropy_decode).  The layout of the result is the one ``jpeg_oracle.entropy_decode`` and
``premvos_jpeg_entropy_decode_host`` produce: per component int16 [block_rows][block_cols][64], natural order, dummy blocks included.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# T.81 annex K.1 / K.2, natural (row-major) order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                      87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                      101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                        99, 99, 99, 99] + [99] * 32, np.int64)


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """jpeg_set_quality(quality, force_baseline=TRUE): the two tables in natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def blend(frame: np.ndarray, idmap: np.ndarray, palette: np.ndarray) -> np.ndarray:
    """merge_functions.py:527-539 draw_mask at alpha 0.5 on every object at once: (frame + colour) >> 1 where id > 0."""
    out = frame.copy()
    on = idmap > 0
    out[on] = ((frame[on].astype(np.int64) + palette[idmap[on]].astype(np.int64)) >> 1).astype(np.uint8)
    return out


def rgb_to_ycc(rgb: np.ndarray) -> List[np.ndarray]:
    r, g, b = (rgb[:, :, k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def _expand(p: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """Replicate the last row / column out to rows x cols."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def component_plane(p: np.ndarray, he: int, ve: int, vmax: int, wb: int, hb: int) -> np.ndarray:
    """One full-resolution component -> its [hb*8][wb*8] sample plane: edge expansion, down-sampling by he x ve, bottom expansion."""
    h = p.shape[0]
    p = _expand(p, -(-h // vmax) * vmax, wb * 8 * he)
    if (he, ve) == (2, 2):
        bias = np.tile(np.array([1, 2]), p.shape[1] // 4 + 1)[:p.shape[1] // 2]
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    elif (he, ve) == (2, 1):
        bias = np.tile(np.array([0, 1]), p.shape[1] // 4 + 1)[:p.shape[1] // 2]
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    else:
        assert (he, ve) == (1, 1)
    return _expand(p[:hb * 8], hb * 8, p.shape[1])


def _fdct_1d(d: List[np.ndarray], first: bool) -> List[np.ndarray]:
    """One pass of the Loeffler-Ligtenberg-Moshovitz forward DCT in 13-bit fixed point over eight int64 arrays; the first pass
    leaves its results scaled up by 2 bits, the second removes them."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    n = 13 - 2 if first else 13 + 2
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, n)
    o[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return o


def fdct_quantise(plane: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """[hb*8][wb*8] samples -> int16 [hb][wb][64]."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    x = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128             # [hb][wb][row][col]
    x = np.stack(_fdct_1d([x[:, :, :, c] for c in range(8)], True), axis=3)                   # rows
    x = np.stack(_fdct_1d([x[:, :, r, :] for r in range(8)], False), axis=2)                  # columns
    x = x.reshape(hb, wb, 64)
    q = quant.astype(np.int64) << 3
    return (np.sign(x) * ((np.abs(x) + (q >> 1)) // q)).astype(np.int16)


def forward(rgb: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", tables=None) -> List[np.ndarray]:
    """uint8 [H][W][3] -> the three components' quantised coefficients, dummy blocks of the edge MCUs included."""
    hmax, vmax = SAMPLING[subsampling]
    h, w = rgb.shape[:2]
    qt = quant_tables(quality) if tables is None else tables
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    out = []
    for ci, p in enumerate(rgb_to_ycc(rgb)):
        hs, vs = (hmax, vmax) if ci == 0 else (1, 1)
        wb, hb = -(-w * hs // (8 * hmax)), -(-h * vs // (8 * vmax))
        real = fdct_quantise(component_plane(p, hmax // hs, vmax // vs, vmax, wb, hb), qt[min(ci, 1)])
        full = np.zeros((mcuy * vs, mcux * hs, 64), np.int16)
        full[:hb, :wb] = real
        for by in range(mcuy * vs):                            # in the order the MCU's blocks are coded: rows, then columns
            for bx in range(mcux * hs):
                if by < hb and bx >= wb:
                    full[by, bx, 0] = full[by, bx - 1, 0]      # right of a real block row: the DC of the block on its left
                elif by >= hb:                                 # a dummy block row: the DC of the last block of the row above, same MCU
                    full[by, bx, 0] = full[by - 1, (bx // hs) * hs + hs - 1, 0]
        out.append(full)
    return out
