// The tap arithmetic of the mask warp (MergeTrack/merge_functions.py:209-217 warp_flow), shared by merge_ops.hip (the byte-mask
// warps) and prewarp_ingest_ops.hip (the fused warp + bit-pack), so that both produce the same bits from one statement of it.
//
// cv2.remap(img_u8, map_f32x2, None, INTER_LINEAR), border constant 0, restated from OpenCV's fixed-point path:
// map -> 1/32-pixel fixed point with round-half-even (cvRound), integer cell (arithmetic >> 5, saturated to int16) and
// 5-bit fractions; tap weights = (32-ay|ay)*(32-ax|ax)*32 (sum 32768); value = (sum w*v + 2^14) >> 15.
// The map is built as merge_functions.py:211-214 does: -flow (float32), then "+= arange" which numpy evaluates in
// float64 and stores back as float32.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace premvos {

// where pixel p of the output reads: the upper-left tap's offset, the four weights, which taps lie inside the mask
struct MaskWarpTaps {
  long o00;
  int w00, w01, w10, w11;
  bool x0, x1, y0, y1;
};

// flow: float [h][w][2] = (u, v); p < h * w
__device__ __forceinline__ MaskWarpTaps mask_warp_taps(const float* __restrict__ flow, const long p, const int h, const int w) {
  const int y = (int)(p / w), x = (int)(p - (long)y * w);
  const float mx = (float)((double)(-flow[2 * p]) + (double)x);
  const float my = (float)((double)(-flow[2 * p + 1]) + (double)y);
  const int sx = __float2int_rn(mx * 32.f), sy = __float2int_rn(my * 32.f);
  int ix = sx >> 5, iy = sy >> 5;
  ix = ix < -32768 ? -32768 : (ix > 32767 ? 32767 : ix);
  iy = iy < -32768 ? -32768 : (iy > 32767 ? 32767 : iy);
  const int ax = sx & 31, ay = sy & 31;
  MaskWarpTaps t;
  t.w00 = (32 - ay) * (32 - ax) * 32;
  t.w01 = (32 - ay) * ax * 32;
  t.w10 = ay * (32 - ax) * 32;
  t.w11 = ay * ax * 32;
  t.x0 = (unsigned)ix < (unsigned)w;
  t.x1 = (unsigned)(ix + 1) < (unsigned)w;
  t.y0 = (unsigned)iy < (unsigned)h;
  t.y1 = (unsigned)(iy + 1) < (unsigned)h;
  t.o00 = (long)iy * w + ix;
  return t;
}

// the remapped value (0 .. 255) of one mask (uint8 [h][w]) at the pixel whose taps are t; a tap outside the mask is not read
__device__ __forceinline__ int mask_warp_value(const uint8_t* __restrict__ m, const MaskWarpTaps& t, const int w) {
  int acc = 1 << 14;
  if (t.y0 && t.x0) acc += t.w00 * m[t.o00];
  if (t.y0 && t.x1) acc += t.w01 * m[t.o00 + 1];
  if (t.y1 && t.x0) acc += t.w10 * m[t.o00 + w];
  if (t.y1 && t.x1) acc += t.w11 * m[t.o00 + w + 1];
  const int v = acc >> 15;
  return v > 255 ? 255 : v;
}

}  // namespace premvos
