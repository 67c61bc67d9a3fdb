// The fully connected CRF of ReID_net/scripts/postproc/crf/crf_davis.py:43-60 (apply_crf: a Gaussian and a bilateral pairwise kernel under
// Potts compatibility, symmetric normalisation, mean-field rounds, argmax), with the two Gaussian filters computed EXACTLY over a truncated
// square window (|dy|, |dx| <= R, clipped at the frame's borders) instead of on pydensecrf's permutohedral lattice:
//   k_g(i,j) = exp(-(dy^2 + dx^2) / (2 gsxy^2)),   k_b(i,j) = exp(-(dy^2 + dx^2) / (2 sxy^2) - |I_i - I_j|^2 / (2 srgb^2))
//   n_m(i) = 1 / sqrt(sum_j k_m(i,j) + 1e-20),   Q~_m[l,i] = n_m(i) sum_j k_m(i,j) n_m(j) Q[l,j],   Q <- softmax_l(-U + sum_m w_m Q~_m)
//
// One walk serves the normaliser and both kernels of a round (`walk`).  A workgroup of 256 threads owns a 64 x 16 tile of output pixels, a
// wave 64 x 4 of it, a lane FOUR neighbouring pixels of one row.  The window's rows are walked in bands of up to 8 source rows staged
// through LDS as planes of floats: the three colour channels and the L channels Q[l,j] n(j), multiplied once while they are staged, zero
// where the frame ends -- so a tap outside the frame adds nothing and no read leaves the planes.  Per band row a lane walks the columns in
// chunks of four: one 16-byte LDS read per plane gives four source pixels, and the 16 (own pixel, source pixel) pairs of the chunk share
// them.  The pair weight does not depend on the label: per tap it is three differences, their squares' sum, one FMA onto the spatial
// exponent and ONE v_exp_f32 (everything is kept as a power of two); then L FMAs.  The spatial exponent is separable: the row's part is one
// number per lane and band row, the column's part comes from a (2R + 1 + 6)-entry table in the kernel's arguments, indexed by dx -- the
// same for every lane, so it is read by scalar loads -- and is -inf beyond R, which makes the weight of the chunks' overhang exactly 0.
// A band row's sum is kept apart and added to the pixel's total once per row: a sum of 12 769 taps is then 113 + 113 additions deep, not
// 12 769 (the normaliser is held to 1e-6).  fp32 throughout, no atomics on floats: two launches give the same bits, and a frame's result
// does not depend on the frames it is stacked with.
#include <math.h>

#include "common.h"

namespace {

constexpr int CRF_MIN_L = 2, CRF_MAX_L = 16, CRF_MAX_R = 64;
constexpr int CRF_THREADS = 256, CRF_TILE_W = 64, CRF_TILE_H = 16, CRF_PX = 4;          // a lane: CRF_PX pixels; a wave: 16 lanes x 4 rows
constexpr int CRF_TAB_OFF = CRF_MAX_R + CRF_PX - 1, CRF_TAB_N = 2 * CRF_TAB_OFF + 2;   // dx = -67 .. 67 (+ one entry of padding)
constexpr int CRF_LDS_BYTES = 64 * 1024, CRF_MAX_BAND = 8;
constexpr int CRF_MAX_PIXELS = 1 << 26;                                                // L * h * w stays an int

// log2 of a kernel's spatial factor along one axis: v[dx + CRF_TAB_OFF] = -dx^2 log2(e) / (2 sxy^2) for |dx| <= R, -inf beyond
struct AxisTab {
  float v[CRF_TAB_N];
};

AxisTab axis_tab(const float sxy, const int R) {
  AxisTab t;
  for (int i = 0; i < CRF_TAB_N; ++i) {
    const int dx = i - CRF_TAB_OFF;
    t.v[i] = (dx < -R || dx > R) ? -INFINITY : (float)(-(double)(dx * dx) * 1.4426950408889634 / (2.0 * (double)sxy * (double)sxy));
  }
  return t;
}

float axis_scale(const float sigma) { return (float)(1.4426950408889634 / (2.0 * (double)sigma * (double)sigma)); }

__host__ __device__ inline int chunks_of(const int R) { return (R + CRF_PX - 1) / CRF_PX; }

// the floats of one band row of one plane, at most
int band_width(const int R) { return CRF_TILE_W + 2 * CRF_PX * chunks_of(R); }

// acc[p][l] += post[p] * sum_j k(i_p, j) src[l, j] over the window of radius R around each of the lane's CRF_PX pixels i_p, where
// src[l, j] = (q ? q[l, j] : 1) * (nrm ? nrm[j] : 1) for l < L inside the frame and 0 elsewhere.  `tab` / `cs`: the spatial factor along x
// (the table) and along y (exponent = -dy^2 cs); `cc`: the colour exponent's scale (COLOUR), own[p]: the lane's own pixels' colours.
// Every thread of the workgroup calls it (it synchronises); lds: band_rows * (3 * COLOUR + LC) * band_width(R) floats.
template <int LC, bool COLOUR>
__device__ __forceinline__ void walk(const AxisTab& tab, const float cs, const float cc, const int R, const uint8_t* __restrict__ frame,
                                     const float* __restrict__ q, const int L, const float* __restrict__ nrm, const int H, const int W,
                                     const int x0, const int y0, const int band_rows, float* __restrict__ lds,
                                     const float (&own)[CRF_PX][3], const float (&post)[CRF_PX], float (&acc)[CRF_PX][LC]) {
  constexpr int CB = COLOUR ? 3 : 0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cx = (lane & 15) * CRF_PX;                                   // the lane's first column inside the tile
  const int yw = y0 + 4 * wave, y = yw + (lane >> 4);
  const int rq = chunks_of(R);
  // chunk m of the lane = the source columns x0 + cx + 4 m .. + 3; the chunks that touch the frame for some lane of the tile
  const int m_lo = max(-rq, -((x0 + CRF_TILE_W + CRF_PX - 2) / CRF_PX)), m_hi = min(rq, (W - 1 - x0) / CRF_PX);
  const int wb = CRF_TILE_W + CRF_PX * (m_hi - m_lo), bx0 = x0 + CRF_PX * m_lo;      // the band: columns bx0 .. bx0 + wb - 1
  const int sy_lo = max(0, y0 - R), sy_hi = min(H, y0 + CRF_TILE_H + R);              // its rows, all inside the frame
  const int plane = band_rows * wb, HW = H * W;
  for (int b0 = sy_lo; b0 < sy_hi; b0 += band_rows) {
    const int nb = min(band_rows, sy_hi - b0);
    __syncthreads();                                                     // the band before this one has been read
    for (int idx = tid; idx < nb * wb; idx += CRF_THREADS) {
      const int r = idx / wb, sx = bx0 + idx - r * wb;
      const bool in = sx >= 0 && sx < W;
      const int pix = (b0 + r) * W + sx;                                 // (used only when `in`)
      const float nj = in ? (nrm != nullptr ? nrm[pix] : 1.f) : 0.f;
      if (COLOUR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) lds[k * plane + idx] = in ? (float)frame[3 * (long)pix + k] : 0.f;
      }
#pragma unroll
      for (int l = 0; l < LC; ++l) lds[(CB + l) * plane + idx] = (in && l < L) ? (q != nullptr ? q[l * HW + pix] : 1.f) * nj : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < nb; ++r) {
      const int sy = b0 + r;
      if (sy < yw - R || sy > yw + 3 + R) continue;                      // (the same for the whole wave) no row of the wave sees it
      const int dy = sy - y;
      const float ly = (dy >= -R && dy <= R) ? -(float)(dy * dy) * cs : -INFINITY;
      float row[CRF_PX][LC];
#pragma unroll
      for (int p = 0; p < CRF_PX; ++p)
#pragma unroll
        for (int l = 0; l < LC; ++l) row[p][l] = 0.f;
      const float* band = lds + r * wb + cx;
      for (int m = m_lo; m <= m_hi; ++m) {
        const float* s = band + CRF_PX * (m - m_lo);
        float col[3][CRF_PX], v[LC][CRF_PX], e0[2 * CRF_PX - 1];
        if (COLOUR) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float4 t = premvos::ld4(s + k * plane);
            col[k][0] = t.x; col[k][1] = t.y; col[k][2] = t.z; col[k][3] = t.w;
          }
        }
#pragma unroll
        for (int l = 0; l < LC; ++l) {
          const float4 t = premvos::ld4(s + (CB + l) * plane);
          v[l][0] = t.x; v[l][1] = t.y; v[l][2] = t.z; v[l][3] = t.w;
        }
#pragma unroll
        for (int i = 0; i < 2 * CRF_PX - 1; ++i) e0[i] = ly + tab.v[CRF_PX * m - (CRF_PX - 1) + i + CRF_TAB_OFF];      // dx = 4 m - 3 + i
#pragma unroll
        for (int p = 0; p < CRF_PX; ++p)
#pragma unroll
          for (int j = 0; j < CRF_PX; ++j) {                              // own pixel p, source pixel j of the chunk: dx = 4 m + j - p
            float e = e0[j - p + CRF_PX - 1];
            if (COLOUR) {
              const float dr = col[0][j] - own[p][0], dg = col[1][j] - own[p][1], db = col[2][j] - own[p][2];
              e = fmaf(fmaf(db, db, fmaf(dg, dg, dr * dr)), -cc, e);
            }
            const float wgt = __builtin_amdgcn_exp2f(e);                  // v_exp_f32: 2^-inf = 0, results below 2^-126 flush to 0
#pragma unroll
            for (int l = 0; l < LC; ++l) row[p][l] = fmaf(wgt, v[l][j], row[p][l]);
          }
      }
#pragma unroll
      for (int p = 0; p < CRF_PX; ++p)
#pragma unroll
        for (int l = 0; l < LC; ++l) acc[p][l] = fmaf(row[p][l], post[p], acc[p][l]);
    }
  }
}

extern __shared__ __attribute__((aligned(16))) float crf_lds[];

struct Geometry {
  int n, h, w, band_rows;
};

template <bool COLOUR>
__global__ __launch_bounds__(CRF_THREADS) void crf_norm_kernel(const uint8_t* __restrict__ frames, const Geometry g, const AxisTab tab,
                                                               const float cs, const float cc, const int R, float* __restrict__ norm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * CRF_TILE_W, y0 = blockIdx.y * CRF_TILE_H;
  const int x = x0 + (lane & 15) * CRF_PX, y = y0 + 4 * wave + (lane >> 4);
  const long f = blockIdx.z, HW = (long)g.h * g.w;
  const uint8_t* frame = frames + 3 * f * HW;
  float own[CRF_PX][3], post[CRF_PX], acc[CRF_PX][1];
#pragma unroll
  for (int p = 0; p < CRF_PX; ++p) {
    const bool in = y < g.h && x + p < g.w;
#pragma unroll
    for (int k = 0; k < 3; ++k) own[p][k] = (COLOUR && in) ? (float)frame[3 * ((long)y * g.w + x + p) + k] : 0.f;
    post[p] = 1.f;
    acc[p][0] = 0.f;
  }
  walk<1, COLOUR>(tab, cs, cc, R, frame, nullptr, 1, nullptr, g.h, g.w, x0, y0, g.band_rows, crf_lds, own, post, acc);
#pragma unroll
  for (int p = 0; p < CRF_PX; ++p)
    if (y < g.h && x + p < g.w) norm[f * HW + (long)y * g.w + x + p] = 1.f / sqrtf(acc[p][0] + 1e-20f);
}

struct StepArgs {
  const uint8_t* frames;
  const float *unary, *q_in, *n_g, *n_b;
  float* q_out;
  int L, gR, R;
  float gcs, gcompat, cs, cc, compat;
};

template <int LC>
__global__ __launch_bounds__(CRF_THREADS) void crf_step_kernel(const StepArgs a, const Geometry g, const AxisTab tab_g, const AxisTab tab_b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * CRF_TILE_W, y0 = blockIdx.y * CRF_TILE_H;
  const int x = x0 + (lane & 15) * CRF_PX, y = y0 + 4 * wave + (lane >> 4);
  const long f = blockIdx.z, HW = (long)g.h * g.w;
  const uint8_t* frame = a.frames + 3 * f * HW;
  float own[CRF_PX][3], post_g[CRF_PX], post_b[CRF_PX], acc[CRF_PX][LC];
#pragma unroll
  for (int p = 0; p < CRF_PX; ++p) {
    const bool in = y < g.h && x + p < g.w;
    const long pix = (long)y * g.w + x + p;
#pragma unroll
    for (int k = 0; k < 3; ++k) own[p][k] = in ? (float)frame[3 * pix + k] : 0.f;
    post_g[p] = in ? a.gcompat * a.n_g[f * HW + pix] : 0.f;               // w_m n_m(i): the message arrives weighted
    post_b[p] = in ? a.compat * a.n_b[f * HW + pix] : 0.f;
#pragma unroll
    for (int l = 0; l < LC; ++l) acc[p][l] = 0.f;
  }
  if (a.q_in != nullptr) {
    const float* q = a.q_in + f * a.L * HW;
    walk<LC, true>(tab_b, a.cs, a.cc, a.R, frame, q, a.L, a.n_b + f * HW, g.h, g.w, x0, y0, g.band_rows, crf_lds, own, post_b, acc);
    walk<LC, false>(tab_g, a.gcs, 0.f, a.gR, frame, q, a.L, a.n_g + f * HW, g.h, g.w, x0, y0, g.band_rows, crf_lds, own, post_g, acc);
  }
  const float* u = a.unary + f * a.L * HW;
  float* out = a.q_out + f * a.L * HW;
#pragma unroll
  for (int p = 0; p < CRF_PX; ++p) {
    if (!(y < g.h && x + p < g.w)) continue;
    const long pix = (long)y * g.w + x + p;
    float top = -INFINITY, sum = 0.f;
#pragma unroll
    for (int l = 0; l < LC; ++l)
      if (l < a.L) {
        acc[p][l] -= u[l * HW + pix];
        top = fmaxf(top, acc[p][l]);
      }
#pragma unroll
    for (int l = 0; l < LC; ++l)
      if (l < a.L) {
        acc[p][l] = expf(acc[p][l] - top);
        sum += acc[p][l];
      }
    const float inv = 1.f / sum;
#pragma unroll
    for (int l = 0; l < LC; ++l)
      if (l < a.L) out[l * HW + pix] = acc[p][l] * inv;
  }
}

__global__ __launch_bounds__(CRF_THREADS) void crf_label_check_kernel(const uint8_t* __restrict__ maps, const long total, const int L,
                                                                      int* __restrict__ flag) {
  bool bad = false;
  for (long i = (long)blockIdx.x * CRF_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * CRF_THREADS) bad |= maps[i] >= L;
  if (bad) atomicOr(flag, 1);
}

// (after crf_label_check_kernel on the same stream: with the flag up nothing is written)
__global__ __launch_bounds__(CRF_THREADS) void crf_unary_kernel(const uint8_t* __restrict__ maps, const long HW, const long total, const int L,
                                                                const float u_own, const float u_other, const float q_own, const float q_other,
                                                                float* __restrict__ unary, float* __restrict__ q0, const int* __restrict__ flag) {
  if (*flag != 0) return;
  for (long i = (long)blockIdx.x * CRF_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * CRF_THREADS) {
    const long f = i / HW, at = f * L * HW + (i - f * HW);
    const int lab = maps[i];
    for (int l = 0; l < L; ++l) {
      unary[at + l * HW] = l == lab ? u_own : u_other;
      q0[at + l * HW] = l == lab ? q_own : q_other;
    }
  }
}

// grid (blocks over a frame's pixels, frames); the differing pixels are counted per wave and added as integers
__global__ __launch_bounds__(CRF_THREADS) void crf_argmax_kernel(const float* __restrict__ q, const long HW, const int L,
                                                                 const uint8_t* __restrict__ before, uint8_t* __restrict__ idmap,
                                                                 int* __restrict__ changed) {
  const long f = blockIdx.y;
  q += f * L * HW;
  int mine = 0;
  for (long i = (long)blockIdx.x * CRF_THREADS + threadIdx.x; i < HW; i += (long)gridDim.x * CRF_THREADS) {
    int lab = 0;
    float top = q[i];
    for (int l = 1; l < L; ++l) {
      const float v = q[l * HW + i];
      if (v > top) {                                                     // strictly: a tie stays with the lower label
        top = v;
        lab = l;
      }
    }
    idmap[f * HW + i] = (uint8_t)lab;
    mine += lab != before[f * HW + i];
  }
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&changed[f], mine);
}

int check_dims(const char* who, const int n, const int h, const int w) {
  PV_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: n, h, w >= 1 (got %d, %d, %d)", who, n, h, w);
  PV_REQUIRE(n <= 65535 && h <= 32768 && w <= 32768 && (long)h * w <= CRF_MAX_PIXELS, "%s: bad dims (%d frames of %d x %d)", who, n, h, w);
  return PREMVOS_OK;
}

int check_labels(const char* who, const int L) {
  PV_REQUIRE(L >= CRF_MIN_L && L <= CRF_MAX_L, "%s: %d to %d labels (got %d)", who, CRF_MIN_L, CRF_MAX_L, L);
  return PREMVOS_OK;
}

int check_radius(const char* who, const int R) {
  PV_REQUIRE(R >= 0 && R <= CRF_MAX_R, "%s: radius 0 to %d (got %d)", who, CRF_MAX_R, R);
  return PREMVOS_OK;
}

dim3 tile_grid(const int n, const int h, const int w) {
  return dim3((unsigned)premvos::cdiv(w, CRF_TILE_W), (unsigned)premvos::cdiv(h, CRF_TILE_H), (unsigned)n);
}

// the band rows that fit the LDS budget when a band row takes `row_floats` floats
int band_rows_for(const int row_floats) {
  const int rows = CRF_LDS_BYTES / (4 * row_floats);
  return rows < 1 ? 1 : rows > CRF_MAX_BAND ? CRF_MAX_BAND : rows;
}

unsigned stride_blocks(const long items) {
  const long blocks = (items + CRF_THREADS - 1) / CRF_THREADS;
  return (unsigned)(blocks < 2048 ? blocks : 2048);
}

template <int LC>
void launch_step(const StepArgs& a, Geometry g, const AxisTab& tg, const AxisTab& tb, hipStream_t s) {
  const int row_b = (3 + LC) * band_width(a.R), row_g = LC * band_width(a.gR), row = row_b > row_g ? row_b : row_g;
  g.band_rows = band_rows_for(row);
  hipLaunchKernelGGL(crf_step_kernel<LC>, tile_grid(g.n, g.h, g.w), dim3(CRF_THREADS), (size_t)4 * row * g.band_rows, s, a, g, tg, tb);
}

}  // namespace

extern "C" int premvos_crf_unary_labels_f32(const uint8_t* idmaps, int32_t n, int32_t h, int32_t w, int32_t L, float gt_prob, float* unary,
                                            float* q0, int32_t* flag, void* stream) {
  PV_REQUIRE(idmaps && unary && q0 && flag, "crf_unary_labels: null pointer");
  if (int rc = check_dims("crf_unary_labels", n, h, w)) return rc;
  if (int rc = check_labels("crf_unary_labels", L)) return rc;
  PV_REQUIRE(gt_prob > 0.f && gt_prob < 1.f, "crf_unary_labels: gt_prob inside (0, 1) (got %g)", (double)gt_prob);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long HW = (long)h * w, total = HW * n;
  const double p = gt_prob, rest = (1.0 - p) / (L - 1);
  const float u_own = (float)-log(p), u_other = (float)-log(rest);
  const double e_own = exp(-(double)u_own), e_other = exp(-(double)u_other), sum = e_own + (L - 1) * e_other;      // Q0 = softmax(-U)
  if (hipMemsetAsync(flag, 0, sizeof(int32_t), s) != hipSuccess) return premvos::fail(PREMVOS_ELAUNCH, "crf_unary_labels: memset failed");
  hipLaunchKernelGGL(crf_label_check_kernel, dim3(stride_blocks(total)), dim3(CRF_THREADS), 0, s, idmaps, total, L, flag);
  hipLaunchKernelGGL(crf_unary_kernel, dim3(stride_blocks(total)), dim3(CRF_THREADS), 0, s, idmaps, HW, total, L, u_own, u_other,
                     (float)(e_own / sum), (float)(e_other / sum), unary, q0, flag);
  if (int rc = premvos::check_launch("crf_unary_labels")) return rc;
  int32_t up = 0;                                                        // the one place this file waits: the caller learns of a bad label
  if (hipMemcpyAsync(&up, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return premvos::fail(PREMVOS_ELAUNCH, "crf_unary_labels: reading the flag failed");
  PV_REQUIRE(up == 0, "crf_unary_labels: an id map holds a label >= L (%d): nothing was written", L);
  return PREMVOS_OK;
}

extern "C" int premvos_crf_norm_f32(const uint8_t* frames, int32_t n, int32_t h, int32_t w, float sxy, float srgb, int32_t R, float* norm,
                                    void* stream) {
  PV_REQUIRE(frames && norm, "crf_norm: null pointer");
  if (int rc = check_dims("crf_norm", n, h, w)) return rc;
  if (int rc = check_radius("crf_norm", R)) return rc;
  PV_REQUIRE(sxy > 0.f && srgb >= 0.f, "crf_norm: sxy > 0, srgb > 0 or 0 for no colour term (got %g, %g)", (double)sxy, (double)srgb);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool colour = srgb > 0.f;
  Geometry g{n, h, w, band_rows_for((colour ? 4 : 1) * band_width(R))};
  const size_t lds = (size_t)4 * (colour ? 4 : 1) * band_width(R) * g.band_rows;
  const AxisTab tab = axis_tab(sxy, R);
  if (colour)
    hipLaunchKernelGGL(crf_norm_kernel<true>, tile_grid(n, h, w), dim3(CRF_THREADS), lds, s, frames, g, tab, axis_scale(sxy), axis_scale(srgb), R, norm);
  else
    hipLaunchKernelGGL(crf_norm_kernel<false>, tile_grid(n, h, w), dim3(CRF_THREADS), lds, s, frames, g, tab, axis_scale(sxy), 0.f, R, norm);
  return premvos::check_launch("crf_norm");
}

extern "C" int premvos_crf_step_f32(const uint8_t* frames, const float* unary, const float* q_in, const float* n_g, const float* n_b, int32_t n,
                                    int32_t h, int32_t w, int32_t L, float gsxy, int32_t gR, float gcompat, float sxy, float srgb, int32_t R,
                                    float compat, float* q_out, void* stream) {
  PV_REQUIRE(frames && unary && n_g && n_b && q_out, "crf_step: null pointer");
  if (int rc = check_dims("crf_step", n, h, w)) return rc;
  if (int rc = check_labels("crf_step", L)) return rc;
  if (int rc = check_radius("crf_step", gR)) return rc;
  if (int rc = check_radius("crf_step", R)) return rc;
  PV_REQUIRE(gsxy > 0.f && sxy > 0.f && srgb > 0.f, "crf_step: gsxy, sxy, srgb > 0 (got %g, %g, %g)", (double)gsxy, (double)sxy, (double)srgb);
  PV_REQUIRE(isfinite(gcompat) && isfinite(compat), "crf_step: gcompat and compat finite");
  const size_t bytes = sizeof(float) * (size_t)n * L * h * w;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(q_in), b0 = reinterpret_cast<uintptr_t>(q_out);
  PV_REQUIRE(!q_in || (a0 + bytes <= b0 || b0 + bytes <= a0), "crf_step: q_out overlaps q_in");
  const StepArgs a{frames, unary, q_in, n_g, n_b, q_out, L, gR, R, axis_scale(gsxy), gcompat, axis_scale(sxy), axis_scale(srgb), compat};
  const Geometry g{n, h, w, 0};
  const AxisTab tg = axis_tab(gsxy, gR), tb = axis_tab(sxy, R);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (L <= 2) launch_step<2>(a, g, tg, tb, s);
  else if (L <= 4) launch_step<4>(a, g, tg, tb, s);
  else if (L <= 8) launch_step<8>(a, g, tg, tb, s);
  else launch_step<16>(a, g, tg, tb, s);
  return premvos::check_launch("crf_step");
}

extern "C" int premvos_crf_argmax_u8(const float* q, int32_t n, int32_t h, int32_t w, int32_t L, const uint8_t* before, uint8_t* idmap,
                                     int32_t* changed, void* stream) {
  PV_REQUIRE(q && before && idmap && changed, "crf_argmax: null pointer");
  if (int rc = check_dims("crf_argmax", n, h, w)) return rc;
  if (int rc = check_labels("crf_argmax", L)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long HW = (long)h * w;
  if (hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)n, s) != hipSuccess) return premvos::fail(PREMVOS_ELAUNCH, "crf_argmax: memset failed");
  const unsigned bx = stride_blocks(HW);
  hipLaunchKernelGGL(crf_argmax_kernel, dim3(bx < 64 ? bx : 64, (unsigned)n), dim3(CRF_THREADS), 0, s, q, HW, L, before, idmap, changed);
  return premvos::check_launch("crf_argmax");
}
