// hipcc-flags: -ffp-contract=off
// The two diagnostics of MergeTrack that are not part of its loop, on the GPU:
//   * viz_scores                  one score sheet per frame (merge_functions.py:547-611): every candidate's crop with its mask tinted,
//                                 under it per template the five score planes, the weighted score and the ground-truth IoU as colour
//                                 cells, a mark on the candidate the weights chose and on the one the annotation would choose; then
//                                 scipy's bytescale with the GLOBAL minimum and maximum of the float canvas
//   * print_max_reid_distance.py  per template the largest ReID distance to any proposal of a video (the number MAX_REID_DISTANCE of
//                                 merge_functions.py:12 was read from)
// float64 like the reference's numpy; no contraction (flag above).  The canvas' extremes are found on the device: every workgroup of
// the first launch writes the extremes of its own tile (or of the scores) to its own workspace slot, every workgroup of the second
// launch folds the slots -- minimum and maximum do not depend on the order, there is no atomic in this file, two launches give the
// same bits.  The distance sums run over the embedding index ascending, one lane per sum.
#include "common.h"
#include "resize_cv.h"
#include "track_select.h"

#include <math.h>

namespace {

constexpr int BOX = 100;                 // box_size (merge_functions.py:559)
constexpr int CELL_H = BOX / 5;          // a plane's cell: 20 rows x 50 columns
constexpr int HALF = BOX / 2;
constexpr int MARK0 = BOX / 8;           // the marks: rows / columns [12, 37) of the weighted cell and of the gt cell
constexpr int MARK1 = BOX / 4 + BOX / 8;
constexpr double ALPHA = 0.3;            // draw_mask(..., alpha=0.3, ...) (merge_functions.py:580)
constexpr int EMB = 128;
constexpr double MAX_REID_DISTANCE = 25; // merge_functions.py:12

struct Tint {
  int c[3];
};

// the source taps and 11-bit weights of the 100 destination columns (rows) of a crop `ssize` wide (high)
__device__ __forceinline__ void stage_coefs(const int tid, const int ssize, int* s0, int* s1, short* a0, short* a1) {
  if (tid < BOX) {
    const double scale = 1.0 / ((double)BOX / (double)ssize);
    premvos::cv_lin_coef(tid, scale, ssize, &s0[tid], &s1[tid], &a0[tid], &a1[tid]);
  }
}

// VResizeLinear of two HResizeLinear rows (csrc/resize_cv.h cv_resize_u8_px, on values already loaded)
__device__ __forceinline__ int cv_mix(const int p00, const int p01, const int p10, const int p11, const int a0, const int a1,
                                      const int b0, const int b1) {
  const int r0 = p00 * a0 + p01 * a1;
  const int r1 = p10 * a0 + p11 * a1;
  const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

__device__ __forceinline__ double dmin(const double a, const double b) { return b < a ? b : a; }
__device__ __forceinline__ double dmax(const double a, const double b) { return b > a ? b : a; }

// minimum and maximum over the workgroup (256 lanes); the result is valid in every lane
__device__ __forceinline__ void block_minmax(double& lo, double& hi, double* s_lo, double* s_hi) {
  const int tid = threadIdx.x;
  s_lo[tid] = lo;
  s_hi[tid] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      s_lo[tid] = dmin(s_lo[tid], s_lo[tid + s]);
      s_hi[tid] = dmax(s_hi[tid], s_hi[tid + s]);
    }
    __syncthreads();
  }
  lo = s_lo[0];
  hi = s_hi[0];
  __syncthreads();
}

// the two colour values of a score cell, c(s) * 255 = ((1 - s) * 255, s * 255, 0) (merge_functions.py:547-551, 590)
__device__ __forceinline__ double cell_value(const double s, const int ch) {
  return ch == 0 ? (1 - s) * 255 : ch == 1 ? s * 255 : 0.0;
}

// First launch, P + 1 workgroups.
// Workgroup j < P: candidate j's tile.  The box is truncated toward zero; with min(h, w) >= 2 the crop is frame[y : y + h - 1,
// x : x + w - 1] clipped to the frame, resized to 100 x 100 with cv2's fixed-point bilinear rule (the mask's crop likewise, as 0 / 1),
// and where the resized mask is > 0 the pixel becomes (uint8)(im * (1 - 0.3) + tint * 0.3).  The tile's bytes go to the sheet's top
// row UNSCALED (they are uint8 already; the second launch rescales them in place); its extremes, without column 0 (the separator
// zeroes it), go to minmax[2j], minmax[2j + 1].
// Workgroup P: the extremes of every colour value a score cell holds -> minmax[2P], minmax[2P + 1]; non-finite plane / gt values
// are left out, a non-finite weighted score counts as 0.  Lane t < T: the first maximum of template t's weighted row and of its gt
// row (non-finite = 0) -> marks[2t], marks[2t + 1].
__global__ __launch_bounds__(256) void viz_tiles_kernel(const uint8_t* __restrict__ frame, const uint8_t* __restrict__ masks,
                                                        const double* __restrict__ boxes, const int h, const int w, const int P,
                                                        const int T, const double* __restrict__ planes,
                                                        const double* __restrict__ weighted, const long wstride,
                                                        const double* __restrict__ gt, const Tint tint, uint8_t* __restrict__ sheet,
                                                        double* __restrict__ minmax, int* __restrict__ marks) {
  __shared__ int s_x0[BOX], s_x1[BOX], s_y0[BOX], s_y1[BOX];
  __shared__ short s_a0[BOX], s_a1[BOX], s_b0[BOX], s_b1[BOX];
  __shared__ double s_lo[256], s_hi[256];
  const int tid = threadIdx.x;
  const int j = blockIdx.x;
  double lo = 0.0, hi = 0.0;                           // (the canvas always holds a zero: the separators)
  if (j == P) {
    const long TP = (long)T * P;
    for (long i = tid; i < 7 * TP; i += 256) {
      double s;
      if (i < 5 * TP) {
        s = planes[i];
      } else if (i < 6 * TP) {
        const long k = i - 5 * TP;
        s = weighted[(k / P) * wstride + k % P];
        if (!isfinite(s)) s = 0;
      } else {
        s = gt[i - 6 * TP];
      }
      if (!isfinite(s)) continue;
      const double r = (1 - s) * 255, g = s * 255;
      lo = dmin(lo, dmin(r, g));
      hi = dmax(hi, dmax(r, g));
    }
    block_minmax(lo, hi, s_lo, s_hi);
    if (tid == 0) {
      minmax[2 * P] = lo;
      minmax[2 * P + 1] = hi;
    }
    if (tid < T) {
      double bw = -INFINITY, bg = -INFINITY;
      int iw = 0, ig = 0;
      for (int p = 0; p < P; ++p) {
        double a = weighted[(long)tid * wstride + p], b = gt[(long)tid * P + p];
        if (!isfinite(a)) a = 0;
        if (!isfinite(b)) b = 0;
        if (a > bw) { bw = a; iw = p; }
        if (b > bg) { bg = b; ig = p; }
      }
      marks[2 * tid] = iw;
      marks[2 * tid + 1] = ig;
    }
    return;
  }
  const double* box = boxes + 4 * (long)j;
  bool ok = isfinite(box[0]) && isfinite(box[1]) && isfinite(box[2]) && isfinite(box[3]);
  int cx0 = 0, cy0 = 0, cw = 0, ch = 0;
  if (ok) {
    const double lim = 1073741824.0;                  // (boxes beyond 2^30 are outside every frame; keeps the casts defined)
    const int bx = (int)fmax(-lim, fmin(lim, box[0])), by = (int)fmax(-lim, fmin(lim, box[1]));
    const int bw = (int)fmax(-lim, fmin(lim, box[2])), bh = (int)fmax(-lim, fmin(lim, box[3]));
    ok = min(bh, bw) >= 2;
    if (ok) {
      const long x1 = min((long)w, max(0L, (long)bx + bw - 1)), y1 = min((long)h, max(0L, (long)by + bh - 1));
      cx0 = min(w, max(0, bx));
      cy0 = min(h, max(0, by));
      cw = (int)x1 - cx0;
      ch = (int)y1 - cy0;
      ok = cw >= 1 && ch >= 1;
    }
  }
  const long sheet_w = (long)BOX * P;
  uint8_t* dst = sheet + (long)BOX * j * 3;
  if (!ok) {                                            // (uniform over the workgroup) a black tile
    for (int i = tid; i < BOX * BOX * 3; i += 256) dst[(i / (BOX * 3)) * sheet_w * 3 + i % (BOX * 3)] = 0;
    if (tid == 0) {
      minmax[2 * j] = 0.0;
      minmax[2 * j + 1] = 0.0;
    }
    return;
  }
  stage_coefs(tid, cw, s_x0, s_x1, s_a0, s_a1);
  if (tid >= 128) stage_coefs(tid - 128, ch, s_y0, s_y1, s_b0, s_b1);
  __syncthreads();
  const uint8_t* im = frame + ((long)cy0 * w + cx0) * 3;
  const uint8_t* mk = masks + (long)j * h * w + (long)cy0 * w + cx0;
  const double keep = 1 - ALPHA;
  int ilo = 0, ihi = 0;
  for (int i = tid; i < BOX * BOX; i += 256) {
    const int r = i / BOX, x = i - r * BOX;
    const long o00 = (long)s_y0[r] * w + s_x0[x], o01 = (long)s_y0[r] * w + s_x1[x];
    const long o10 = (long)s_y1[r] * w + s_x0[x], o11 = (long)s_y1[r] * w + s_x1[x];
    const int a0 = s_a0[x], a1 = s_a1[x], b0 = s_b0[r], b1 = s_b1[r];
    const int m = cv_mix(mk[o00] != 0, mk[o01] != 0, mk[o10] != 0, mk[o11] != 0, a0, a1, b0, b1);
    uint8_t* out = dst + (long)r * sheet_w * 3 + x * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int v = cv_mix(im[o00 * 3 + c], im[o01 * 3 + c], im[o10 * 3 + c], im[o11 * 3 + c], a0, a1, b0, b1);
      if (m > 0) v = (int)((double)v * keep + (double)tint.c[c] * ALPHA);
      v = v > 255 ? 255 : v;
      out[c] = (uint8_t)v;
      if (x) {
        ilo = min(ilo, v);
        ihi = max(ihi, v);
      }
    }
  }
  lo = (double)ilo;
  hi = (double)ihi;
  block_minmax(lo, hi, s_lo, s_hi);
  if (tid == 0) {
    minmax[2 * j] = lo;
    minmax[2 * j + 1] = hi;
  }
}

// Second launch, a workgroup per 100 x 100 tile of the sheet (blockIdx.x = candidate, blockIdx.y = 0: the crops, i + 1: template i),
// lanes along the tile's rows of 300 bytes.  Folds the P + 1 pairs of extremes, then writes scipy's bytescale of the canvas:
//   scale = 255 / (cmax - cmin) (a zero range counts as 1);  out = (uint8)(clip((v - cmin) * scale, 0, 255) + 0.5)
// Row i + 1: planes k = 0 .. 4 in the left half (rows 20k .. 20k + 20), the weighted score top right, gt bottom right; column 0 and
// row 0 of every tile are the separators; the two 25 x 25 marks (merge_functions.py:604-609).  A non-finite value is written as 0.
__global__ __launch_bounds__(256) void viz_sheet_kernel(const int P, const int T, const double* __restrict__ planes,
                                                        const double* __restrict__ weighted, const long wstride,
                                                        const double* __restrict__ gt, const double* __restrict__ minmax,
                                                        const int* __restrict__ marks, uint8_t* __restrict__ sheet) {
  __shared__ double s_lo[256], s_hi[256];
  const int tid = threadIdx.x;
  const int j = blockIdx.x, ty = blockIdx.y;
  double cmin = 0.0, cmax = 0.0;
  for (int i = tid; i <= P; i += 256) {
    cmin = dmin(cmin, minmax[2 * i]);
    cmax = dmax(cmax, minmax[2 * i + 1]);
  }
  block_minmax(cmin, cmax, s_lo, s_hi);
  double range = cmax - cmin;
  if (range == 0) range = 1;
  const double scale = 255.0 / range;
  const long sheet_w = (long)BOX * P;
  uint8_t* dst = sheet + ((long)ty * BOX * sheet_w + (long)BOX * j) * 3;
  double cell[7];
  bool mark_w = false, mark_g = false;
  if (ty > 0) {
    const int t = ty - 1;
    const long TP = (long)T * P, at = (long)t * P + j;
#pragma unroll
    for (int k = 0; k < 5; ++k) cell[k] = planes[k * TP + at];
    cell[5] = weighted[(long)t * wstride + j];
    if (!isfinite(cell[5])) cell[5] = 0;
    cell[6] = gt[at];
    mark_w = marks[2 * t] == j;
    mark_g = marks[2 * t + 1] == j;
  }
  for (int i = tid; i < BOX * BOX * 3; i += 256) {
    const int r = i / (BOX * 3), b = i - r * (BOX * 3), x = b / 3, c = b - x * 3;
    uint8_t* out = dst + (long)r * sheet_w * 3 + b;
    double v;
    if (ty == 0) {
      v = x == 0 ? 0.0 : (double)*out;
    } else if (x == 0 || r == 0) {
      v = 0.0;
    } else if (x >= HALF + MARK0 && x < HALF + MARK1 &&
               ((mark_w && r >= MARK0 && r < MARK1) || (mark_g && r >= HALF + MARK0 && r < HALF + MARK1))) {
      v = 0.0;
    } else {
      const int k = x < HALF ? r / CELL_H : (r < HALF ? 5 : 6);
      double s = cell[0];
#pragma unroll
      for (int q = 1; q < 7; ++q) s = k == q ? cell[q] : s;
      v = cell_value(s, c);
    }
    uint8_t o = 0;
    if (isfinite(v)) {
      double u = (v - cmin) * scale;
      u = u < 0 ? 0 : u > 255 ? 255 : u;
      o = (uint8_t)(int)(u + 0.5);
    }
    *out = o;
  }
}

// A workgroup per template, a lane per proposal n = lane, lane + 256, ...: dist = sqrt(sum_k (c[k] - t[k])^2), k ascending; an
// infinite distance counts as 0 (print_max_reid_distance.py:42-46); the maximum starts at 0 (a frame without proposals contributes
// zeros) and a NaN wins it, as in numpy's max.  over[t] counts the pairs beyond MAX_REID_DISTANCE (integer sums).
__global__ __launch_bounds__(256) void reid_max_distance_kernel(const double* __restrict__ templ, const double* __restrict__ props,
                                                                const long N, double* __restrict__ out, long long* __restrict__ over) {
  __shared__ double s_t[EMB];
  __shared__ double s_v[256];
  __shared__ unsigned long long s_n[256];
  const int tid = threadIdx.x, t = blockIdx.x;
  if (tid < EMB) s_t[tid] = templ[(long)t * EMB + tid];
  __syncthreads();
  double best = 0.0;
  unsigned long long cnt = 0;
  for (long n = tid; n < N; n += 256) {
    const double* c = props + n * EMB;
    double acc = 0.0;
    for (int k = 0; k < EMB; ++k) {
      const double d = c[k] - s_t[k];
      acc += d * d;
    }
    double dist = sqrt(acc);
    if (isinf(dist)) dist = 0;
    cnt += dist > MAX_REID_DISTANCE ? 1u : 0u;
    best = premvos::nanmax(best, dist);
  }
  s_v[tid] = best;
  s_n[tid] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      s_v[tid] = premvos::nanmax(s_v[tid], s_v[tid + s]);
      s_n[tid] += s_n[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[t] = s_v[0];
    if (over) over[t] = (long long)s_n[0];
  }
}

}  // namespace

// the workspace: P + 1 pairs of extremes (double), then T pairs of marks (int32)
static int64_t viz_workspace_bytes(int32_t T, int32_t P) {
  return (int64_t)sizeof(double) * 2 * ((int64_t)P + 1) + (int64_t)sizeof(int32_t) * 2 * (int64_t)T;
}

extern "C" int premvos_viz_scores_u8(const uint8_t* frame, int32_t h, int32_t w, const uint8_t* masks, const double* boxes, int32_t P,
                                     const double* planes, const double* weighted, int64_t weighted_stride, const double* gt, int32_t T,
                                     const uint8_t* tint3, void* workspace, int64_t workspace_bytes, uint8_t* sheet, void* stream) {
  PV_REQUIRE(frame && masks && boxes && planes && weighted && gt && tint3 && workspace && sheet, "viz_scores: null pointer");
  PV_REQUIRE(h >= 1 && w >= 1 && (long)h * w < (1L << 31), "viz_scores: bad dims (h %d, w %d)", h, w);
  PV_REQUIRE(T >= 1 && T <= 255, "viz_scores: 1 to 255 templates (got %d)", T);
  PV_REQUIRE(P >= 1, "viz_scores: at least one candidate (got %d)", P);
  PV_REQUIRE((long)BOX * P <= 65535, "viz_scores: a sheet of %d candidates is %ld pixels wide, a JPEG holds at most 65535", P, (long)BOX * P);
  PV_REQUIRE((long)BOX * (T + 1) * BOX * P <= (64L << 20), "viz_scores: a sheet of %ld x %ld pixels is beyond the JPEG encoder's 64 Mi",
             (long)BOX * P, (long)BOX * (T + 1));
  PV_REQUIRE(weighted_stride >= P, "viz_scores: the weighted rows' stride %ld is shorter than their %d scores", (long)weighted_stride, P);
  PV_REQUIRE(workspace_bytes >= viz_workspace_bytes(T, P) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
             "viz_scores: the workspace needs %ld bytes, 8-byte aligned (got %ld)", (long)viz_workspace_bytes(T, P),
             (long)workspace_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* minmax = static_cast<double*>(workspace);
  int* marks = reinterpret_cast<int*>(minmax + 2 * ((long)P + 1));
  Tint tint;
  for (int c = 0; c < 3; ++c) tint.c[c] = tint3[c];
  hipLaunchKernelGGL(viz_tiles_kernel, dim3((unsigned)P + 1), dim3(256), 0, s, frame, masks, boxes, h, w, P, T, planes, weighted,
                     (long)weighted_stride, gt, tint, sheet, minmax, marks);
  if (const int rc = premvos::check_launch("viz_scores (tiles)")) return rc;
  hipLaunchKernelGGL(viz_sheet_kernel, dim3((unsigned)P, (unsigned)T + 1), dim3(256), 0, s, P, T, planes, weighted, (long)weighted_stride, gt,
                     minmax, marks, sheet);
  return premvos::check_launch("viz_scores");
}

extern "C" int premvos_reid_max_distance_f64(const double* templates, int32_t T, const double* proposals, int64_t N, double* max_distance,
                                             int64_t* over, void* stream) {
  PV_REQUIRE(templates && max_distance, "reid_max_distance: null pointer");
  PV_REQUIRE(T >= 1 && T <= 65535 && N >= 0 && N < (1L << 31), "reid_max_distance: bad dims (T %d, N %ld)", T, (long)N);
  PV_REQUIRE(proposals || N == 0, "reid_max_distance: null pointer (%ld proposals)", (long)N);
  hipLaunchKernelGGL(reid_max_distance_kernel, dim3((unsigned)T), dim3(256), 0, static_cast<hipStream_t>(stream), templates, proposals,
                     (long)N, max_distance, reinterpret_cast<long long*>(over));
  return premvos::check_launch("reid_max_distance");
}
