// GPU baseline JPEG encode, the mirror image of jpeg_ops.hip: uint8 RGB frame in HBM -> quantised DCT coefficients in the layout
// premvos_jpeg_entropy_decode_host produces; the serial Huffman pass runs on the host (premvos_jpeg_entropy_encode_host,
// host_files.hip).  Built for the overlay pictures of the merge loop (merge_functions.py:527-545 draw_mask + save_jpg): the frame
// and the id map the loop just painted are both in HBM, so the blend is fused into the encoder's load and the blended picture is
// never stored.
//
// The arithmetic restates libjpeg's compressor with its defaults, all of it in integers -- equal or wrong, nothing to tolerate:
//   jccolor.c   rgb_ycc_convert          16-bit fixed-point RGB -> YCbCr
//   jcprepct.c  expand_bottom_edge, jcsample.c expand_right_edge / h2v1_downsample / h2v2_downsample
//   jfdctint.c  jpeg_fdct_islow          (CONST_BITS 13, PASS1_BITS 2: rows, then columns)
//   jcdctmgr.c  quantize                 (the DCT leaves its results scaled by 8)
//   jccoefct.c  compress_data            (dummy blocks of an edge MCU: zero AC, the DC of their predecessor)
// tests/test_gpu_jpeg_encode.py compares with tests/jpeg_forward_restated.py, which tests/test_cpu_jpeg_encode.py pins to the
// coefficients PIL's libjpeg-turbo writes.
//
// One workgroup per strip of STRIP_MCUS MCUs of one MCU row.  Stage 1: all threads load the strip's pixels (edge pixels replicated),
// blend, convert, and leave full-resolution Y / Cb / Cr samples in LDS.  Stage 2: one thread per 8x8 block gathers its samples
// (chroma: averaged on the way), runs both DCT passes in registers, quantises and stores the block's 128 bytes.
#include "common.h"

#include <string.h>

namespace {

constexpr int THREADS = 256;
constexpr int STRIP_MCUS = 8;
constexpr int PITCH = STRIP_MCUS * 16 + 8;       // bytes per LDS sample row (a multiple of 8: blocks are read 8 bytes at a time)

struct EncQuant {
  uint16_t q[2][64];                             // luma, chroma; natural order
};

struct EncGeom {
  int32_t h, w, mcux;
  int32_t real_w[3], real_h[3];                  // real (non-dummy) blocks across / down
  int32_t blocks_w[3];
  int64_t coef_offset[3];
};

constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
              FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
              FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// One pass of jfdctint.c (jpeg_fdct_islow) over eight values, in place.  FIRST: the row pass (results scaled up by PASS1_BITS).
template <bool FIRST>
__device__ inline void fdct8(int (&d)[8]) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2, R = 1 << (N - 1);
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if constexpr (FIRST) {
    d[0] = (tmp10 + tmp11) * 4;
    d[4] = (tmp10 - tmp11) * 4;
  } else {
    d[0] = (tmp10 + tmp11 + 2) >> 2;
    d[4] = (tmp10 - tmp11 + 2) >> 2;
  }
  int z1 = (tmp12 + tmp13) * FIX_0_541196100;
  d[2] = (z1 + tmp13 * FIX_0_765366865 + R) >> N;
  d[6] = (z1 + tmp12 * (-FIX_1_847759065) + R) >> N;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * FIX_1_175875602;
  const int t4 = tmp4 * FIX_0_298631336, t5 = tmp5 * FIX_2_053119869, t6 = tmp6 * FIX_3_072711026, t7 = tmp7 * FIX_1_501321110;
  z1 *= -FIX_0_899976223;
  z2 *= -FIX_2_562915447;
  z3 = z3 * (-FIX_1_961570560) + z5;
  z4 = z4 * (-FIX_0_390180644) + z5;
  d[7] = (t4 + z1 + z3 + R) >> N;
  d[5] = (t5 + z2 + z4 + R) >> N;
  d[3] = (t6 + z2 + z3 + R) >> N;
  d[1] = (t7 + z1 + z4 + R) >> N;
}

__device__ inline void load_pixel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ idmap, const uint8_t* __restrict__ palette,
                                  long pix, bool blend, int& r, int& g, int& b) {
  const uint8_t* p = rgb + pix * 3;
  r = p[0];
  g = p[1];
  b = p[2];
  if (blend) {
    const int id = idmap[pix];
    if (id) {                                     // merge_functions.py:527-539 at alpha 0.5: truncation of the float = the shift
      r = (r + palette[id * 3]) >> 1;
      g = (g + palette[id * 3 + 1]) >> 1;
      b = (b + palette[id * 3 + 2]) >> 1;
    }
  }
}

// HS x VS: luma samples per chroma sample (1x1, 2x1, 2x2).
template <int HS, int VS>
__global__ void __launch_bounds__(THREADS) jpeg_forward_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ idmap,
                                                               const uint8_t* __restrict__ palette, EncQuant qt, EncGeom g,
                                                               int16_t* __restrict__ coef) {
  constexpr int MW = 8 * HS, MH = 8 * VS, NB = HS * VS + 2;
  __shared__ __attribute__((aligned(8))) uint8_t smp[3][MH][PITCH];
  const int m0 = blockIdx.x * STRIP_MCUS, my = blockIdx.y;
  const int nm = min(STRIP_MCUS, g.mcux - m0);
  const int x0 = m0 * MW, y0 = my * MH, sw = nm * MW;
  const bool blend = idmap != nullptr;

  for (int i = threadIdx.x; i < MH * sw; i += THREADS) {
    const int yy = i / sw, xx = i - yy * sw;
    const int gx = min(x0 + xx, g.w - 1);                              // right edge: the last column again
    const int ly = min(y0 + yy, g.h - 1);                              // bottom edge: the last row again
    int r, gg, b;
    load_pixel(rgb, idmap, palette, (long)ly * g.w + gx, blend, r, gg, b);
    smp[0][yy][xx] = (uint8_t)((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16);
    if constexpr (VS == 2) {
      // rows are replicated to an even count BEFORE down-sampling, the down-sampled plane's last row AFTER it: below the last
      // real chroma row the source is that row's pair of image rows, not the image's last row twice
      const int cy = min((y0 + yy) >> 1, ((g.h + 1) >> 1) - 1);
      const int cyy = min(2 * cy + (yy & 1), g.h - 1);
      if (cyy != ly) load_pixel(rgb, idmap, palette, (long)cyy * g.w + gx, blend, r, gg, b);
    }
    smp[1][yy][xx] = (uint8_t)((-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16);
    smp[2][yy][xx] = (uint8_t)((32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16);
  }
  __syncthreads();

  for (int blk = threadIdx.x; blk < nm * NB; blk += THREADS) {
    const int m = blk / NB, k = blk - m * NB;
    const int c = k < HS * VS ? 0 : 1 + (k - HS * VS);
    int by = 0, bx = 0;
    if (c == 0) {
      by = k / HS;
      bx = k - by * HS;
    }
    const int cw = c == 0 ? HS : 1, cv = c == 0 ? VS : 1;
    const int gby = my * cv + by, gbx = (m0 + m) * cw + bx;
    // a dummy block carries only a DC: that of the block coded before it in its MCU row, or, in a dummy block row, of the last
    // block of the row above (itself a copy when that one is a dummy) -- compute that real block again and keep its DC
    int sby = by, sbx = bx;
    const bool dummy = gby >= g.real_h[c] || gbx >= g.real_w[c];
    if (gby >= g.real_h[c]) {
      sby = by - 1;
      sbx = cw - 1;
    }
    while ((m0 + m) * cw + sbx >= g.real_w[c]) --sbx;                  // (block 0 of an MCU's first row is always real)

    int ws[8][8];
    if (c == 0) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint2 v = *reinterpret_cast<const uint2*>(&smp[0][sby * 8 + r][(m * HS + sbx) * 8]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ws[r][j] = (int)((v.x >> (8 * j)) & 0xFF) - 128;
          ws[r][4 + j] = (int)((v.y >> (8 * j)) & 0xFF) - 128;
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        int row[8 * HS];
#pragma unroll
        for (int j = 0; j < 8 * HS; ++j) row[j] = 0;
#pragma unroll
        for (int v = 0; v < VS; ++v) {
          const uint2* src = reinterpret_cast<const uint2*>(&smp[c][r * VS + v][m * MW]);
#pragma unroll
          for (int q = 0; q < HS; ++q) {
            const uint2 t = src[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              row[q * 8 + j] += (int)((t.x >> (8 * j)) & 0xFF);
              row[q * 8 + 4 + j] += (int)((t.y >> (8 * j)) & 0xFF);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (HS == 2 && VS == 2) ws[r][j] = ((row[2 * j] + row[2 * j + 1] + 1 + (j & 1)) >> 2) - 128;
          else if constexpr (HS == 2) ws[r][j] = ((row[2 * j] + row[2 * j + 1] + (j & 1)) >> 1) - 128;
          else ws[r][j] = row[j] - 128;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) fdct8<true>(ws[r]);
#pragma unroll
    for (int col = 0; col < 8; ++col) {
      int d[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) d[r] = ws[r][col];
      fdct8<false>(d);
#pragma unroll
      for (int r = 0; r < 8; ++r) ws[r][col] = d[r];
    }
    int4* dst = reinterpret_cast<int4*>(coef + g.coef_offset[c] + ((long)gby * g.blocks_w[c] + gbx) * 64);
    const uint16_t* q = qt.q[c == 0 ? 0 : 1];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint32_t o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = ws[r][j];
        const unsigned div = (unsigned)q[r * 8 + j] << 3;
        const int mag = (int)(((unsigned)(v < 0 ? -v : v) + (div >> 1)) / div);
        o[j] = (uint32_t)(v < 0 ? -mag : mag) & 0xFFFFu;
        if (dummy && (r | j)) o[j] = 0;
      }
      dst[r] = make_int4((int)(o[0] | (o[1] << 16)), (int)(o[2] | (o[3] << 16)), (int)(o[4] | (o[5] << 16)), (int)(o[6] | (o[7] << 16)));
    }
  }
}

__global__ void __launch_bounds__(THREADS) overlay_blend_kernel(const uint8_t* __restrict__ frame, const uint8_t* __restrict__ idmap,
                                                                const uint8_t* __restrict__ palette, long npix,
                                                                uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= npix) return;
  int r, g, b;
  load_pixel(frame, idmap, palette, i, true, r, g, b);
  out[i * 3] = (uint8_t)r;
  out[i * 3 + 1] = (uint8_t)g;
  out[i * 3 + 2] = (uint8_t)b;
}

constexpr int64_t kMaxPixels = 64LL << 20;       // what the decoder accepts (jpeg_ops.hip)

}  // namespace

extern "C" int premvos_overlay_blend_u8(const uint8_t* frame, const uint8_t* idmap, const uint8_t* palette, int32_t h, int32_t w,
                                        uint8_t* out, void* stream) {
  PV_REQUIRE(frame && idmap && palette && out, "overlay_blend: null argument");
  PV_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= kMaxPixels, "overlay_blend: frame of %d x %d pixels", h, w);
  const long npix = (long)h * w;
  hipLaunchKernelGGL(overlay_blend_kernel, dim3((unsigned)((npix + THREADS - 1) / THREADS)), dim3(THREADS), 0,
                     static_cast<hipStream_t>(stream), frame, idmap, palette, npix, out);
  return premvos::check_launch("overlay_blend");
}

extern "C" int premvos_jpeg_forward_u8(const uint8_t* rgb, const uint8_t* idmap, const uint8_t* palette, int32_t h, int32_t w,
                                       const uint16_t* quant_luma, const uint16_t* quant_chroma, int32_t hs, int32_t vs,
                                       premvos_jpeg_info* info, int16_t* coef, int64_t coef_capacity, void* stream) {
  PV_REQUIRE(info && quant_luma && quant_chroma, "jpeg_forward: null argument");
  PV_REQUIRE(h > 0 && w > 0 && h <= 65535 && w <= 65535 && (int64_t)h * w <= kMaxPixels, "jpeg_forward: frame of %d x %d pixels", h, w);
  PV_REQUIRE((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2),
             "jpeg_forward: sampling %dx%d (4:4:4 = 1x1, 4:2:2 = 2x1, 4:2:0 = 2x2)", hs, vs);
  PV_REQUIRE((idmap == nullptr) == (palette == nullptr), "jpeg_forward: the id map and the palette come together");
  EncQuant qt;
  for (int k = 0; k < 64; ++k) {
    PV_REQUIRE(quant_luma[k] >= 1 && quant_luma[k] <= 255 && quant_chroma[k] >= 1 && quant_chroma[k] <= 255,
               "jpeg_forward: quantisation values must be 1 ... 255 (baseline)");
    qt.q[0][k] = quant_luma[k];
    qt.q[1][k] = quant_chroma[k];
  }
  premvos_jpeg_info& I = *info;
  memset(&I, 0, sizeof(I));
  I.width = w;
  I.height = h;
  I.ncomp = 3;
  I.hs = hs;
  I.vs = vs;
  I.mcux = premvos::cdiv(w, 8 * hs);
  I.mcuy = premvos::cdiv(h, 8 * vs);
  EncGeom g;
  g.h = h;
  g.w = w;
  g.mcux = I.mcux;
  int64_t off = 0;
  for (int c = 0; c < 3; ++c) {
    const int ch = c == 0 ? hs : 1, cv = c == 0 ? vs : 1;
    I.blocks_w[c] = g.blocks_w[c] = I.mcux * ch;
    I.blocks_h[c] = I.mcuy * cv;
    I.coef_offset[c] = g.coef_offset[c] = off;
    off += (int64_t)I.blocks_w[c] * I.blocks_h[c] * 64;
    g.real_w[c] = (int)(((int64_t)w * ch + 8 * hs - 1) / (8 * hs));
    g.real_h[c] = (int)(((int64_t)h * cv + 8 * vs - 1) / (8 * vs));
    memcpy(I.quant[c], qt.q[c == 0 ? 0 : 1], sizeof(I.quant[c]));
  }
  I.coef_count = off;
  if (!coef) return PREMVOS_OK;                    // geometry only
  PV_REQUIRE(rgb, "jpeg_forward: null argument");
  PV_REQUIRE(premvos::aligned16(coef), "jpeg_forward: the coefficient buffer must be 16-byte aligned");
  PV_REQUIRE(coef_capacity >= I.coef_count, "jpeg_forward: coefficient buffer holds %lld values, the frame needs %lld",
             (long long)coef_capacity, (long long)I.coef_count);
  const dim3 grid(premvos::cdiv(I.mcux, STRIP_MCUS), I.mcuy), block(THREADS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hs == 1) hipLaunchKernelGGL((jpeg_forward_kernel<1, 1>), grid, block, 0, s, rgb, idmap, palette, qt, g, coef);
  else if (vs == 1) hipLaunchKernelGGL((jpeg_forward_kernel<2, 1>), grid, block, 0, s, rgb, idmap, palette, qt, g, coef);
  else hipLaunchKernelGGL((jpeg_forward_kernel<2, 2>), grid, block, 0, s, rgb, idmap, palette, qt, g, coef);
  return premvos::check_launch("jpeg_forward");
}
