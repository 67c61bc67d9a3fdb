// hipcc-flags: -ffp-contract=off
// The pre-warp merge of a whole video (MergeTrack/oldmerge.py:87-218, "PREMVOS 1 uses pre-warp") and the objective of its weight
// search (merge_functions.py:613-634 eval_video).  Every proposal carries its mask already warped to the next frame, so no network
// runs in the loop and almost all of the work is independent of the weights and of the previous frame:
//   * premvos_bits_overlap_i32       every intersection and area the warp plane can ask for, one launch   (oldmerge.py:114-116)
//   * premvos_prewarp_reid_f64       both ReID planes of every frame                                      (oldmerge.py:87-110)
//   * premvos_prewarp_chain_f64      what stays sequential, one workgroup per weight set                  (oldmerge.py:112-127,150-197)
//   * premvos_prewarp_paint_bits_u8  the id maps and / or the integer counts of the objective             (oldmerge.py:176-208, eval_video)
// and, for the reference's use_ff_negative_props switch (oldmerge.py:43,63-85,137-138,147: frame 0's proposals that touch neither an
// annotated object nor one another become label-0 templates behind the annotated ones):
//   * premvos_prewarp_negatives_i32     the greedy walk in descending score, integers and float64 compares only  (oldmerge.py:63-85)
//   * premvos_prewarp_gather_neg_u8     their mask rows and embeddings into the templates' places, inside HBM    (oldmerge.py:138,147)
//   * premvos_prewarp_chain_neg_f64 / premvos_prewarp_paint_neg_bits_u8: the two entries above with n_neg trailing templates that no
//     frame annotates (the old entries are their n_neg = 0 call: one kernel each)
// All masks of a video live bit-packed in ONE pool (premvos_mask_pack_bits_u8's layout, a row of `stride` bytes per mask, stride a
// multiple of 8): 64 pixels are one popcount.  float64 like the reference's numpy, no contraction (flag above), every sum in a fixed
// order, only integer atomics: two launches give the same bits.
// A "block table" (int32 [B][8], the same values in host memory for the checks and in device memory for the kernels) names, per
// frame t: a0, na = the P_t current masks; b0, nb and c0, nc = the candidates for a template's current mask in that frame (frame 0:
// the masks of the objects annotated in it; later: the forward masks of frame t-1's proposals, then of the objects annotated in
// t-1); where the block's [na][nb+nc] intersections begin in `inter`; where its na + nb + nc areas begin in `areas`.
#include "common.h"

#include <math.h>

namespace {

constexpr int EMB = 128;        // the ReID embedding (ReID_net: 128-d)
constexpr int MAX_T = 64;       // templates of a video
constexpr int MAX_P = 256;      // proposals of a frame: one lane of the chain's workgroup each
constexpr int MAX_TP = 8000;    // T x P_t doubles = 62.5 KiB of LDS for the snapped scores (admits T = 40 with P = 200, T = 64 with P = 125)
constexpr int OV_TILE = 16, OV_CHUNK = 32;

// bits of word k of a mask of hw pixels that are pixels
__device__ __forceinline__ unsigned long long tail_mask(const long k, const long hw) {
  const long left = hw - 64 * k;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

// grid (tiles, B): a workgroup = 16 x 16 pairs of one block; thread (i, j) owns pair (row i, column j).  Both sides are staged once
// per tile, OV_CHUNK words at a time (rows padded by one word: the 16 columns of a wave fall into different banks).
__global__ __launch_bounds__(256) void bits_overlap_kernel(const unsigned long long* __restrict__ bits, const long words, const long hw,
                                                           const int* __restrict__ blocks, int* __restrict__ inter,
                                                           int* __restrict__ areas) {
  __shared__ unsigned long long s_a[OV_TILE][OV_CHUNK + 1], s_b[OV_TILE][OV_CHUNK + 1];
  const int* blk = blocks + 8 * blockIdx.y;
  const int a0 = blk[0], na = blk[1], b0 = blk[2], nb = blk[3], c0 = blk[4], nc = blk[5], ioff = blk[6], aoff = blk[7];
  const int ncols = nb + nc;
  // (a block without columns still has its rows' areas counted, and the other way round: at least one tile per side)
  const int tr = max(1, (na + OV_TILE - 1) / OV_TILE), tc = max(1, (ncols + OV_TILE - 1) / OV_TILE);
  if (na + ncols == 0 || (int)blockIdx.x >= tr * tc) return;   // (the whole workgroup: before any barrier)
  const int ti = blockIdx.x / tc, tj = blockIdx.x - ti * tc;
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15;
  int cnt = 0, aa = 0, ab = 0;
  for (long k0 = 0; k0 < words; k0 += OV_CHUNK) {
    for (int q = tid; q < 2 * OV_TILE * OV_CHUNK; q += 256) {
      const int r = q / OV_CHUNK, kk = q - r * OV_CHUNK;
      const long k = k0 + kk;
      long slot = -1;
      if (r < OV_TILE) {
        const int row = ti * OV_TILE + r;
        if (row < na) slot = a0 + row;
      } else {
        const int col = tj * OV_TILE + r - OV_TILE;
        if (col < ncols) slot = col < nb ? b0 + col : c0 + col - nb;
      }
      unsigned long long v = 0;
      if (slot >= 0 && k < words) v = bits[slot * words + k] & tail_mask(k, hw);
      if (r < OV_TILE) s_a[r][kk] = v; else s_b[r - OV_TILE][kk] = v;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < OV_CHUNK; ++kk) {
      const unsigned long long a = s_a[i][kk], b = s_b[j][kk];
      cnt += __popcll(a & b);
      aa += __popcll(a);
      ab += __popcll(b);
    }
    __syncthreads();
  }
  const int row = ti * OV_TILE + i, col = tj * OV_TILE + j;
  if (row < na && col < ncols) inter[(long)ioff + (long)row * ncols + col] = cnt;
  if (j == 0 && tj == 0 && row < na) areas[(long)aoff + row] = aa;
  if (i == 0 && ti == 0 && col < ncols) areas[(long)aoff + na + col] = ab;
}

// numpy's max of two: a NaN wins
__device__ __forceinline__ double nanmax(const double a, const double b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

// One workgroup per template: its distance to every proposal of the video (sum of squares in index order, then the root), the
// largest of them with the infinite ones counted as 0, then 1 - d / max with a non-finite result set to 0, into flat[T][sumP].
__global__ __launch_bounds__(256) void prewarp_reid_dist_kernel(const double* __restrict__ emb_p, const double* __restrict__ emb_t,
                                                                const int sumP, double* __restrict__ flat, double* __restrict__ maxd) {
  __shared__ double s_m[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const double* et = emb_t + (long)t * EMB;
  double m = 0.0;
  for (int j = tid; j < sumP; j += 256) {
    const double* ep = emb_p + (long)j * EMB;
    double acc = 0.0;
    for (int k = 0; k < EMB; ++k) {
      const double d = ep[k] - et[k];
      acc += d * d;
    }
    const double d = sqrt(acc);
    flat[(long)t * sumP + j] = d;
    m = nanmax(m, isinf(d) ? 0.0 : d);
  }
  s_m[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_m[tid] = nanmax(s_m[tid], s_m[tid + s]);     // (a maximum: the order does not change it)
    __syncthreads();
  }
  m = s_m[0];
  if (tid == 0) maxd[t] = m;
  for (int j = tid; j < sumP; j += 256) {                       // (each lane reads back what it wrote itself)
    double s = 1 - flat[(long)t * sumP + j] / m;
    if (!isfinite(s)) s = 0;
    flat[(long)t * sumP + j] = s;
  }
}

// One lane per proposal of the video: its column of the ReID plane into the frame's [T][P_t] block, and 1 - the maximum over the
// OTHER templates beside it (the scores are finite: first and second maximum of the column do it; all ones for one template).
__global__ __launch_bounds__(256) void prewarp_reid_planes_kernel(const double* __restrict__ flat, const int* __restrict__ poff, const int N,
                                                                  const int sumP, const int T, double* __restrict__ reid,
                                                                  double* __restrict__ oreid) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= sumP) return;
  int lo = 0, hi = N - 1;                                       // the frame f with poff[f] <= j < poff[f + 1]
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (poff[mid] <= j) lo = mid; else hi = mid - 1;
  }
  const int p0 = poff[lo], P = poff[lo + 1] - p0, p = j - p0;
  double m1 = -INFINITY, m2 = -INFINITY;
  int i1 = -1;
  for (int t = 0; t < T; ++t) {
    const double s = flat[(long)t * sumP + j];
    if (s > m1) { m2 = m1; m1 = s; i1 = t; } else if (s > m2) m2 = s;
  }
  double* r = reid + (long)T * p0 + p;
  double* o = oreid + (long)T * p0 + p;
  for (int t = 0; t < T; ++t) {
    r[(long)t * P] = flat[(long)t * sumP + j];
    o[(long)t * P] = T > 1 ? 1 - (t == i1 ? m2 : m1) : 1.0;
  }
}

struct ChainArgs {
  const int* inter; const int* areas; const int* blocks; const int* poff; const int* first;
  const double* pscore; const double* reid; const double* oreid; const double* weights;
  int N, T;
  int* chosen; double* best; double* weighted;
  int n_neg;                    // the last n_neg templates are negatives: column first[1] + j of frame 0, annotated in no frame
};

// numpy's argmax over (value, index) pairs: a NaN beats a number, a larger number a smaller one, the lower index an equal
__device__ __forceinline__ bool takes_over(const double av, const int ai, const double bv, const int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an) return bn && bi < ai;
  return bn || bv > av || (bv == av && bi < ai);
}

// One workgroup per weight set walks the frames in order.  Lane p owns column p of the frame's [T][P_t] planes: the warp plane from
// the integer counts and the templates' current columns, its inverse from the column's first and second maximum (an IoU is never a
// NaN), the weighted sum in the order of the restatement, the column's first maximum ("snapping"); the snapped scores go to LDS,
// where a wave takes the first maximum of a row.  Then the objects annotated in this frame take their annotation.  A negative
// (oldmerge.py:147) starts on its own mask, block 0's column first[1] + j, and is never forced: `first` ends below it.
__global__ __launch_bounds__(256) void prewarp_chain_kernel(const ChainArgs a) {
  __shared__ double s_w[MAX_TP];
  __shared__ double s_best[MAX_T];
  __shared__ int s_cur[MAX_T], s_chosen[MAX_T];
  const int tid = threadIdx.x, set = blockIdx.x, T = a.T, N = a.N;
  const double* wt = a.weights + 5 * set;
  const double w0 = wt[0], w1 = wt[1], w2 = wt[2], w3 = wt[3], w4 = wt[4];
  if (tid < T) s_cur[tid] = tid < a.first[1] ? tid : (tid >= T - a.n_neg ? a.first[1] + tid - (T - a.n_neg) : -1);
  __syncthreads();
  for (int t = 0; t < N; ++t) {
    const int* blk = a.blocks + 8 * t;
    const int P = blk[1], ncols = blk[3] + blk[5];
    const long ioff = blk[6], aoff = blk[7], p0 = a.poff[t];
    if (tid < P) {
      const int p = tid;
      const double obj = a.pscore[p0 + p];
      const long ap = a.areas[aoff + p];
      double m1 = -INFINITY, m2 = -INFINITY;
      int i1 = -1;
      for (int k = 0; k < T; ++k) {
        const int c = s_cur[k];
        double iou = 0.0;
        if (c >= 0 && c < ncols) {
          const long i = a.inter[ioff + (long)p * ncols + c];
          if (i != 0) iou = (double)i / (double)(ap + a.areas[aoff + P + c] - i);
        }
        if (iou > m1) { m2 = m1; m1 = iou; i1 = k; } else if (iou > m2) m2 = iou;
      }
      double cb = 0.0;
      int ci = 0;
      for (int k = 0; k < T; ++k) {
        const int c = s_cur[k];
        double iou = 0.0;
        if (c >= 0 && c < ncols) {
          const long i = a.inter[ioff + (long)p * ncols + c];
          if (i != 0) iou = (double)i / (double)(ap + a.areas[aoff + P + c] - i);
        }
        const double ow = T > 1 ? 1 - (k == i1 ? m2 : m1) : 1.0;
        const long e = (long)T * p0 + (long)k * P + p;
        double ws = w0 * obj;
        ws += w1 * a.reid[e];
        ws += w2 * a.oreid[e];
        ws += w3 * iou;
        ws += w4 * ow;
        s_w[k * P + p] = ws;
        if (a.weighted) a.weighted[e] = ws;
        if (k == 0) { cb = ws; ci = 0; } else if (cb == cb && (ws != ws || ws > cb)) { cb = ws; ci = k; }
      }
      for (int k = 0; k < T; ++k) s_w[k * P + p] = s_w[k * P + p] * (ci == k ? 1.0 : 0.0);       // (a NaN or an infinity times 0 is a NaN, as in numpy)
    }
    __syncthreads();
    if (P > 0) {
      const int lane = tid & 63;
      for (int k = tid >> 6; k < T; k += 4) {
        double bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int p = lane; p < P; p += 64) {
          const double v = s_w[k * P + p];
          if (takes_over(bv, bi, v, p)) { bv = v; bi = p; }
        }
        for (int off = 32; off > 0; off >>= 1) {
          const double ov = __shfl_xor(bv, off, 64);
          const int oi = __shfl_xor(bi, off, 64);
          if (takes_over(bv, bi, ov, oi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_best[k] = bv; s_chosen[k] = bi; }
      }
    } else if (tid < T) {
      s_best[tid] = 0.0;                                        // a frame without proposals: the empty mask, score 0
      s_chosen[tid] = -1;
    }
    __syncthreads();
    if (tid < T) {
      const int f0 = a.first[t], f1 = a.first[t + 1];
      double b = s_best[tid];
      int c = s_chosen[tid];
      if (tid >= f0 && tid < f1) { b = 1.0; c = P + tid - f0; } // annotated IN this frame
      const long o = ((long)set * N + t) * T + tid;
      a.chosen[o] = c;
      a.best[o] = b;
      s_cur[tid] = c;                                           // the next block's column: its forward mask is carried
    }
    __syncthreads();
  }
}

struct PaintArgs {
  const unsigned long long* bits; long words, hw; int S;
  const int* blocks; const int* first; const int* ids; int ann_slot0;
  const int* chosen; const double* best; int N, T;
  uint8_t* idmap; int vec;
  const unsigned long long* gt; int T0; int* counts;
};

// grid (word blocks, N, W); a lane resolves the 64 pixels of one word: the T chosen masks from the LAST painted (highest score; equal
// scores: the higher index; a NaN last of all) down, each claiming what is still free.  A template not annotated yet has label 0: it
// writes nothing but still claims.  For a scored object (template k < T0, annotation id k + 1) the lane's |R and G|, |R or G|, |R| are
// summed over the wave and added with one integer atomic each.
__global__ __launch_bounds__(256) void prewarp_paint_kernel(const PaintArgs a) {
  __shared__ int s_slot[MAX_T];
  __shared__ uint8_t s_order[MAX_T], s_label[MAX_T];
  const int tid = threadIdx.x, t = blockIdx.y, set = blockIdx.z, T = a.T;
  const long o = ((long)set * a.N + t) * T;
  if (tid < T) {
    double key = a.best[o + tid];
    if (key != key) key = INFINITY;
    int rank = 0;
    for (int q = 0; q < T; ++q) {
      double kq = a.best[o + q];
      if (kq != kq) kq = INFINITY;
      rank += kq < key || (kq == key && q < tid);
    }
    s_order[rank] = (uint8_t)tid;
    const int* blk = a.blocks + 8 * t;
    const int P = blk[1], f0 = a.first[t], f1 = a.first[t + 1], c = a.chosen[o + tid];
    long slot = -1;
    if (c >= 0 && c < P) slot = (long)blk[0] + c;
    else if (c >= P && c - P < f1 - f0) slot = (long)a.ann_slot0 + f0 + (c - P);
    s_slot[tid] = (slot >= 0 && slot < a.S) ? (int)slot : -1;
    s_label[tid] = tid < f1 ? (uint8_t)a.ids[tid] : (uint8_t)0;
  }
  __syncthreads();
  const long k = (long)blockIdx.x * 256 + tid;
  const bool active = k < a.words;
  const unsigned long long tm = active ? tail_mask(k, a.hw) : 0ull;
  unsigned long long free_px = tm;
  uint32_t out[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) out[q] = 0;
  for (int r = T - 1; r >= 0; --r) {
    const int kt = s_order[r], slot = s_slot[kt];
    unsigned long long m = 0;
    if (active && slot >= 0) m = a.bits[(long)slot * a.words + k];
    const unsigned long long claimed = m & free_px;
    free_px &= ~m;
    const uint32_t lab = s_label[kt];
    if (a.idmap && claimed && lab) {
      const uint32_t lv = lab * 0x01010101u;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const uint32_t nib = (uint32_t)(claimed >> (4 * q)) & 0xfu;
        const uint32_t spread = ((nib * 0x00204081u) & 0x01010101u) * 0xffu;
        out[q] |= spread & lv;
      }
    }
    if (a.counts && kt < a.T0) {                                // (kt is the same for the whole workgroup)
      const unsigned long long g = active ? a.gt[((long)t * a.T0 + kt) * a.words + k] & tm : 0ull;
      unsigned long long c3 = (unsigned long long)__popcll(claimed & g) | ((unsigned long long)__popcll(claimed | g) << 20) |
                              ((unsigned long long)__popcll(claimed) << 40);       // <= 64 each per lane, 4096 per wave: 20 bits do
      for (int off = 32; off > 0; off >>= 1) c3 += __shfl_down(c3, off, 64);
      if ((tid & 63) == 0 && c3) {
        int* dst = a.counts + (((long)set * a.N + t) * a.T0 + kt) * 3;
        const int ci = (int)(c3 & 0xfffffu), cu = (int)((c3 >> 20) & 0xfffffu), cr = (int)(c3 >> 40);
        if (ci) atomicAdd(dst, ci);
        if (cu) atomicAdd(dst + 1, cu);
        if (cr) atomicAdd(dst + 2, cr);
      }
    }
  }
  if (a.idmap && active) {
    uint8_t* dst = a.idmap + (long)t * a.hw + 64 * k;
    const long left = a.hw - 64 * k;
    if (a.vec && left >= 64) {
#pragma unroll
      for (int q = 0; q < 4; ++q) reinterpret_cast<uint4*>(dst)[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (4 * q + b < left) dst[4 * q + b] = (uint8_t)(out[q] >> (8 * b));
    }
  }
}

}  // namespace

// The checks every entry shares (before any HIP call): the pool, and with `blocks` the block table against the pool and the outputs.
static int pool_check(const char* what, const void* bits, const int32_t S, const int64_t stride, const int64_t hw) {
  if (!bits) return premvos::fail(PREMVOS_EINVAL, "%s: null pointer", what);
  if (S < 1 || hw < 1 || hw >= (1L << 31)) return premvos::fail(PREMVOS_EINVAL, "%s: bad dims", what);
  if (stride < 8 || stride % 8 != 0 || stride * 8 < hw || (reinterpret_cast<uintptr_t>(bits) & 7u))
    return premvos::fail(PREMVOS_EINVAL, "%s: a mask is a row of `stride` bytes, a multiple of 8 that holds h*w bits, 8-byte aligned (got %ld for %ld bits)",
                         what, (long)stride, (long)hw);
  return PREMVOS_OK;
}

static int range_check(const char* what, const int b, const char* side, const long lo, const long n, const long S) {
  if (n < 0 || (n > 0 && (lo < 0 || lo + n > S)))
    return premvos::fail(PREMVOS_EINVAL, "%s: block %d: %s masks %ld + %ld outside the pool's %ld", what, b, side, lo, n, S);
  return PREMVOS_OK;
}

static int table_check(const char* what, const int32_t* blocks, const int32_t B, const long S, const int64_t n_inter, const int64_t n_areas,
                       int& max_tiles) {
  max_tiles = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* r = blocks + 8 * b;
    if (const int rc = range_check(what, b, "row", r[0], r[1], S)) return rc;
    if (const int rc = range_check(what, b, "column", r[2], r[3], S)) return rc;
    if (const int rc = range_check(what, b, "column", r[4], r[5], S)) return rc;
    const long na = r[1], ncols = (long)r[3] + r[5];
    if (r[6] < 0 || r[7] < 0 || r[6] + na * ncols > n_inter || r[7] + na + ncols > n_areas)
      return premvos::fail(PREMVOS_EINVAL, "%s: block %d: its %ld x %ld counts at %d / areas at %d do not fit the outputs (%ld, %ld)", what, b, na,
                           ncols, r[6], r[7], (long)n_inter, (long)n_areas);
    const long tr = (na + OV_TILE - 1) / OV_TILE, tc = (ncols + OV_TILE - 1) / OV_TILE;
    const long tiles = na + ncols == 0 ? 0 : (tr > 1 ? tr : 1) * (tc > 1 ? tc : 1);
    if (tiles > max_tiles) max_tiles = (int)tiles;
  }
  return PREMVOS_OK;
}

extern "C" int premvos_bits_overlap_i32(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                                        const int32_t* blocks_dev, int32_t B, int32_t* inter, int64_t n_inter, int32_t* areas,
                                        int64_t n_areas, void* stream) {
  if (const int rc = pool_check("bits_overlap", bits, S, stride, hw)) return rc;
  PV_REQUIRE(B >= 0 && n_inter >= 0 && n_areas >= 0, "bits_overlap: bad dims");
  if (B == 0) return PREMVOS_OK;
  PV_REQUIRE(blocks_host && blocks_dev && (inter || n_inter == 0) && (areas || n_areas == 0), "bits_overlap: null pointer");
  PV_REQUIRE(B <= 65535, "bits_overlap: at most 65535 blocks (got %d)", B);
  int max_tiles = 0;
  if (const int rc = table_check("bits_overlap", blocks_host, B, S, n_inter, n_areas, max_tiles)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((n_inter && hipMemsetAsync(inter, 0, sizeof(int32_t) * (size_t)n_inter, s) != hipSuccess) ||
      (n_areas && hipMemsetAsync(areas, 0, sizeof(int32_t) * (size_t)n_areas, s) != hipSuccess))
    return premvos::fail(PREMVOS_ELAUNCH, "bits_overlap: memset failed");
  if (max_tiles == 0) return PREMVOS_OK;                        // empty blocks only
  hipLaunchKernelGGL(bits_overlap_kernel, dim3((unsigned)max_tiles, (unsigned)B), dim3(256), 0, s,
                     reinterpret_cast<const unsigned long long*>(bits), (long)(stride / 8), (long)hw, blocks_dev, inter, areas);
  return premvos::check_launch("bits_overlap");
}

// poff [N+1]: ascending from 0 to sumP; first [N+1]: ascending from 0 to T
static int offsets_check(const char* what, const char* name, const int32_t* v, const int32_t N, const long total) {
  if (v[0] != 0 || v[N] != total) return premvos::fail(PREMVOS_EINVAL, "%s: %s runs from %d to %d, not from 0 to %ld", what, name, v[0], v[N], total);
  for (int t = 0; t < N; ++t)
    if (v[t + 1] < v[t]) return premvos::fail(PREMVOS_EINVAL, "%s: %s descends at frame %d", what, name, t);
  return PREMVOS_OK;
}

extern "C" int premvos_prewarp_reid_f64(const double* emb_p, const double* emb_t, int32_t sumP, int32_t T, const int32_t* poff_host,
                                        const int32_t* poff_dev, int32_t N, double* flat, double* maxd, double* reid, double* oreid,
                                        void* stream) {
  PV_REQUIRE(sumP >= 0 && T >= 1 && N >= 1, "prewarp_reid: bad dims");
  PV_REQUIRE(T <= MAX_T, "prewarp_reid: at most %d templates (got %d)", MAX_T, T);
  PV_REQUIRE(emb_t && poff_host && poff_dev && maxd && (sumP == 0 || (emb_p && flat && reid && oreid)), "prewarp_reid: null pointer");
  PV_REQUIRE((long)sumP * T < (1L << 31), "prewarp_reid: too many proposals");
  if (const int rc = offsets_check("prewarp_reid", "poff", poff_host, N, sumP)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(prewarp_reid_dist_kernel, dim3(T), dim3(256), 0, s, emb_p, emb_t, sumP, flat, maxd);
  if (sumP > 0)
    hipLaunchKernelGGL(prewarp_reid_planes_kernel, dim3((unsigned)((sumP + 255) / 256)), dim3(256), 0, s, flat, poff_dev, N, sumP, T, reid, oreid);
  return premvos::check_launch("prewarp_reid");
}

// what the chain and the paint require of a video's tables: block t's rows are frame t's P_t proposals, its columns the candidates
// of the header's rule
static int video_check(const char* what, const int32_t* blocks, const int32_t* poff, const int32_t* first, const int32_t N, const int32_t T,
                       const int32_t n_neg, const long sumP, const bool caps) {
  if (const int rc = offsets_check(what, "poff", poff, N, sumP)) return rc;
  if (const int rc = offsets_check(what, "first", first, N, T - n_neg)) return rc;
  for (int t = 0; t < N; ++t) {
    const int P = poff[t + 1] - poff[t];
    const int want = t == 0 ? first[1] + n_neg : (poff[t] - poff[t - 1]) + (first[t] - first[t - 1]);
    if (blocks[8 * t + 1] != P || blocks[8 * t + 3] + blocks[8 * t + 5] != want)
      return premvos::fail(PREMVOS_EINVAL, "%s: block %d is %d x %d, the video's tables ask for %d x %d", what, t, blocks[8 * t + 1],
                           blocks[8 * t + 3] + blocks[8 * t + 5], P, want);
    if (caps && (P > MAX_P || (long)P * T > MAX_TP))
      return premvos::fail(PREMVOS_EINVAL, "%s: frame %d: %d proposals x %d templates; at most %d proposals and %d scores fit the workgroup's LDS",
                           what, t, P, T, MAX_P, MAX_TP);
  }
  return PREMVOS_OK;
}

static int chain_launch(const char* what, const int32_t* inter, int64_t n_inter, const int32_t* areas, int64_t n_areas,
                        const int32_t* blocks_host, const int32_t* blocks_dev, const int32_t* poff_host, const int32_t* poff_dev,
                        const int32_t* first_host, const int32_t* first_dev, int32_t N, int32_t T, int32_t n_neg,
                        const double* proposal_score, const double* reid, const double* oreid, const double* weights, int32_t W,
                        int32_t* chosen, double* best, double* weighted, void* stream) {
  PV_REQUIRE(N >= 1 && T >= 1 && W >= 1 && n_inter >= 0 && n_areas >= 0, "%s: bad dims", what);
  PV_REQUIRE(T <= MAX_T, "%s: at most %d templates (got %d)", what, MAX_T, T);
  PV_REQUIRE(n_neg >= 0 && n_neg <= T, "%s: %d negatives among %d templates", what, n_neg, T);
  PV_REQUIRE(blocks_host && blocks_dev && poff_host && poff_dev && first_host && first_dev && weights && chosen && best,
             "%s: null pointer", what);
  PV_REQUIRE(weighted == nullptr || W == 1, "%s: the weighted scores are written for one weight set only (got %d)", what, W);
  const long sumP = poff_host[N];
  PV_REQUIRE(sumP == 0 || (inter && areas && proposal_score && reid && oreid), "%s: null pointer", what);
  if (const int rc = video_check(what, blocks_host, poff_host, first_host, N, T, n_neg, sumP, true)) return rc;
  int max_tiles = 0;
  if (const int rc = table_check(what, blocks_host, N, 1L << 31, n_inter, n_areas, max_tiles)) return rc;
  ChainArgs a{inter, areas, blocks_dev, poff_dev, first_dev, proposal_score, reid, oreid, weights, N, T, chosen, best, weighted, n_neg};
  hipLaunchKernelGGL(prewarp_chain_kernel, dim3((unsigned)W), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return premvos::check_launch(what);
}

extern "C" int premvos_prewarp_chain_f64(const int32_t* inter, int64_t n_inter, const int32_t* areas, int64_t n_areas,
                                         const int32_t* blocks_host, const int32_t* blocks_dev, const int32_t* poff_host,
                                         const int32_t* poff_dev, const int32_t* first_host, const int32_t* first_dev, int32_t N, int32_t T,
                                         const double* proposal_score, const double* reid, const double* oreid, const double* weights,
                                         int32_t W, int32_t* chosen, double* best, double* weighted, void* stream) {
  return chain_launch("prewarp_chain", inter, n_inter, areas, n_areas, blocks_host, blocks_dev, poff_host, poff_dev, first_host, first_dev, N, T,
                      0, proposal_score, reid, oreid, weights, W, chosen, best, weighted, stream);
}

extern "C" int premvos_prewarp_chain_neg_f64(const int32_t* inter, int64_t n_inter, const int32_t* areas, int64_t n_areas,
                                             const int32_t* blocks_host, const int32_t* blocks_dev, const int32_t* poff_host,
                                             const int32_t* poff_dev, const int32_t* first_host, const int32_t* first_dev, int32_t N,
                                             int32_t T, int32_t n_neg, const double* proposal_score, const double* reid,
                                             const double* oreid, const double* weights, int32_t W, int32_t* chosen, double* best,
                                             double* weighted, void* stream) {
  return chain_launch("prewarp_chain_neg", inter, n_inter, areas, n_areas, blocks_host, blocks_dev, poff_host, poff_dev, first_host, first_dev, N,
                      T, n_neg, proposal_score, reid, oreid, weights, W, chosen, best, weighted, stream);
}

static int paint_launch(const char* what, const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                        const int32_t* blocks_dev, const int32_t* first_host, const int32_t* first_dev, const int32_t* ids,
                        int32_t ann_slot0, const int32_t* chosen, const double* best, int32_t N, int32_t T, int32_t n_neg, int32_t W,
                        uint8_t* idmap, const uint8_t* gt_bits, int32_t T0, int32_t* counts, void* stream) {
  if (const int rc = pool_check(what, bits, S, stride, hw)) return rc;
  PV_REQUIRE(N >= 1 && T >= 1 && W >= 1, "%s: bad dims", what);
  PV_REQUIRE(T <= MAX_T, "%s: at most %d templates (got %d)", what, MAX_T, T);
  PV_REQUIRE(n_neg >= 0 && n_neg <= T, "%s: %d negatives among %d templates", what, n_neg, T);
  PV_REQUIRE(N <= 65535 && W <= 65535, "%s: at most 65535 frames and weight sets (got %d, %d)", what, N, W);
  PV_REQUIRE(blocks_host && blocks_dev && first_host && first_dev && ids && chosen && best, "%s: null pointer", what);
  PV_REQUIRE(idmap || counts, "%s: neither id maps nor counts asked for", what);
  PV_REQUIRE(idmap == nullptr || W == 1, "%s: id maps are written for one weight set only (got %d)", what, W);
  PV_REQUIRE(counts == nullptr || (gt_bits && T0 >= 1 && T0 <= T - n_neg && (reinterpret_cast<uintptr_t>(gt_bits) & 7u) == 0),
             "%s: the counts need the annotations' bit planes and 1 <= T0 <= T (got %d)", what, T0);
  if (const int rc = offsets_check(what, "first", first_host, N, T - n_neg)) return rc;
  PV_REQUIRE(ann_slot0 >= 0 && ann_slot0 + (long)(T - n_neg) <= S, "%s: annotation masks %d + %d outside the pool's %d", what, ann_slot0,
             T - n_neg, S);
  for (int t = 0; t < N; ++t)
    if (const int rc = range_check(what, t, "row", blocks_host[8 * t], blocks_host[8 * t + 1], S)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (counts && hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)W * N * T0 * 3, s) != hipSuccess)
    return premvos::fail(PREMVOS_ELAUNCH, "%s: memset failed", what);
  const long words = stride / 8;
  PaintArgs a{reinterpret_cast<const unsigned long long*>(bits), words, (long)hw, S, blocks_dev, first_dev, ids, ann_slot0, chosen, best, N, T,
              idmap, (int)(hw % 16 == 0 && premvos::aligned16(idmap)), reinterpret_cast<const unsigned long long*>(gt_bits),
              counts ? T0 : 0, counts};
  hipLaunchKernelGGL(prewarp_paint_kernel, dim3((unsigned)((words + 255) / 256), (unsigned)N, (unsigned)W), dim3(256), 0, s, a);
  return premvos::check_launch(what);
}

extern "C" int premvos_prewarp_paint_bits_u8(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                                             const int32_t* blocks_dev, const int32_t* first_host, const int32_t* first_dev,
                                             const int32_t* ids, int32_t ann_slot0, const int32_t* chosen, const double* best, int32_t N,
                                             int32_t T, int32_t W, uint8_t* idmap, const uint8_t* gt_bits, int32_t T0, int32_t* counts,
                                             void* stream) {
  return paint_launch("prewarp_paint", bits, S, stride, hw, blocks_host, blocks_dev, first_host, first_dev, ids, ann_slot0, chosen, best, N, T, 0, W,
                      idmap, gt_bits, T0, counts, stream);
}

// The paint kernel reads a template's label as `k < first[t + 1] ? ids[k] : 0` and an annotation slot only for a column beyond the
// frame's proposals: a negative (k >= first[N]) is label 0 in every frame and only ever holds a proposal, so the kernel is the same.
extern "C" int premvos_prewarp_paint_neg_bits_u8(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                                                 const int32_t* blocks_dev, const int32_t* first_host, const int32_t* first_dev,
                                                 const int32_t* ids, int32_t ann_slot0, const int32_t* chosen, const double* best,
                                                 int32_t N, int32_t T, int32_t n_neg, int32_t W, uint8_t* idmap, const uint8_t* gt_bits,
                                                 int32_t T0, int32_t* counts, void* stream) {
  return paint_launch("prewarp_paint_neg", bits, S, stride, hw, blocks_host, blocks_dev, first_host, first_dev, ids, ann_slot0, chosen, best, N, T,
                      n_neg, W, idmap, gt_bits, T0, counts, stream);
}

// ---- the negative first-frame templates (oldmerge.py:63-85 get_negative_ff_props) ------------------------------------------------------
namespace {

// grid (tiles): 16 x 16 pairs as in bits_overlap_kernel, but a pair only asks whether the two masks share a pixel (oldmerge.py:74-75
// `iou(...) > 0` is exactly that).  Rows: frame 0's P0 proposals; columns: the A0 objects annotated in frame 0, then the P0 proposals.
__global__ __launch_bounds__(256) void neg_conflict_kernel(const unsigned long long* __restrict__ bits, const long words, const long hw,
                                                           const int cur0, const int P0, const int ann0, const int A0,
                                                           uint8_t* __restrict__ conflict) {
  __shared__ unsigned long long s_a[OV_TILE][OV_CHUNK + 1], s_b[OV_TILE][OV_CHUNK + 1];
  const int ncols = A0 + P0, tc = (ncols + OV_TILE - 1) / OV_TILE;
  const int ti = blockIdx.x / tc, tj = blockIdx.x - ti * tc;
  const int tid = threadIdx.x, i = tid >> 4, j = tid & 15;
  unsigned long long any = 0;
  for (long k0 = 0; k0 < words; k0 += OV_CHUNK) {
    for (int q = tid; q < 2 * OV_TILE * OV_CHUNK; q += 256) {
      const int r = q / OV_CHUNK, kk = q - r * OV_CHUNK;
      const long k = k0 + kk;
      long slot = -1;
      if (r < OV_TILE) {
        const int row = ti * OV_TILE + r;
        if (row < P0) slot = cur0 + row;
      } else {
        const int col = tj * OV_TILE + r - OV_TILE;
        if (col < ncols) slot = col < A0 ? ann0 + col : cur0 + col - A0;
      }
      unsigned long long v = 0;
      if (slot >= 0 && k < words) v = bits[slot * words + k] & tail_mask(k, hw);
      if (r < OV_TILE) s_a[r][kk] = v; else s_b[r - OV_TILE][kk] = v;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < OV_CHUNK; ++kk) any |= s_a[i][kk] & s_b[j][kk];
    __syncthreads();
  }
  const int row = ti * OV_TILE + i, col = tj * OV_TILE + j;
  if (row < P0 && col < ncols) conflict[(long)row * ncols + col] = any != 0;
}

// One workgroup.  Lane i ranks candidate i by counting (#{score_j > score_i} + #{score_j == score_i, j < i}: Python's stable sort
// with reverse=True, oldmerge.py:69; a NaN score is left out: a rule of our own) and packs its conflict row into LDS, a bit per
// column (A0 + P0 <= 320 columns = 10 words a row, 10 KiB).  Wave 0 then walks the ranks: lane q keeps word q of the current set,
// a step is one AND per lane and one ballot.
constexpr int NEG_WORDS = (MAX_T + MAX_P) / 32;
__global__ __launch_bounds__(256) void neg_walk_kernel(const uint8_t* __restrict__ conflict, const double* __restrict__ score, const int P0,
                                                       const int A0, const int K, int* __restrict__ taken, int* __restrict__ count) {
  __shared__ double s_score[MAX_P];
  __shared__ int s_order[MAX_P];
  __shared__ unsigned s_conf[MAX_P][NEG_WORDS];
  const int tid = threadIdx.x, ncols = A0 + P0;
  if (tid < P0) {
    s_score[tid] = score[tid];
    const uint8_t* row = conflict + (long)tid * ncols;
    for (int q = 0; q < NEG_WORDS; ++q) {
      unsigned word = 0;
      for (int b = 0; b < 32; ++b) {
        const int c = 32 * q + b;
        if (c < ncols && row[c]) word |= 1u << b;
      }
      s_conf[tid][q] = word;
    }
  }
  __syncthreads();
  bool valid = false;
  if (tid < P0) {
    const double v = s_score[tid];
    valid = v == v;
    if (valid) {
      int rank = 0;
      for (int q = 0; q < P0; ++q) {
        const double sq = s_score[q];
        rank += sq > v || (sq == v && q < tid);
      }
      s_order[rank] = tid;
    }
  }
  const int nvalid = __syncthreads_count(valid);
  if (tid >= 64) return;
  const int lane = tid;
  unsigned in_set = 0;                                          // columns 32 lane .. 32 lane + 31 of the current set: the annotated objects first
  if (lane < NEG_WORDS) in_set = A0 >= 32 * (lane + 1) ? ~0u : (A0 > 32 * lane ? (1u << (A0 - 32 * lane)) - 1u : 0u);
  int n = 0;
  for (int r = 0; r < nvalid && (K < 0 || n < K); ++r) {
    const int i = s_order[r];
    const bool hit = lane < NEG_WORDS && (s_conf[i][lane] & in_set) != 0;
    if (!__any(hit)) {
      if (lane == 0) taken[n] = i;
      ++n;
      const int c = A0 + i;
      if ((c >> 5) == lane) in_set |= 1u << (c & 31);
    }
  }
  for (int q = n + lane; q < P0; q += 64) taken[q] = -1;
  if (lane == 0) count[0] = n;
}

// grid (n_neg): workgroup n copies the mask row of proposal taken[n] into slot neg0 + n and its embedding into row n of emb_neg
__global__ __launch_bounds__(256) void neg_gather_kernel(unsigned long long* __restrict__ bits, const long words, const int cur0, const int P0,
                                                         const int neg0, const int* __restrict__ taken, const double* __restrict__ emb_p,
                                                         double* __restrict__ emb_neg) {
  const int n = blockIdx.x, src = taken[n];
  if (src < 0 || src >= P0) return;                             // (the whole workgroup; the entry's caller sized n_neg by `count`)
  const unsigned long long* from = bits + (long)(cur0 + src) * words;
  unsigned long long* to = bits + (long)(neg0 + n) * words;
  for (long k = threadIdx.x; k < words; k += 256) to[k] = from[k];
  if (threadIdx.x < EMB) emb_neg[(long)n * EMB + threadIdx.x] = emb_p[(long)src * EMB + threadIdx.x];
}

}  // namespace

extern "C" int premvos_prewarp_negatives_i32(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, int32_t cur_slot0, int32_t P0,
                                             int32_t ann_slot0, int32_t A0, const double* score, int32_t K, uint8_t* conflict,
                                             int32_t* taken, int32_t* count, void* stream) {
  if (const int rc = pool_check("prewarp_negatives", bits, S, stride, hw)) return rc;
  PV_REQUIRE(P0 >= 0 && A0 >= 0, "prewarp_negatives: bad dims");
  PV_REQUIRE(P0 <= MAX_P && A0 <= MAX_T, "prewarp_negatives: at most %d proposals in frame 0 and %d annotated objects (got %d, %d)", MAX_P, MAX_T,
             P0, A0);
  PV_REQUIRE(count && (P0 == 0 || (score && conflict && taken)), "prewarp_negatives: null pointer");
  if (const int rc = range_check("prewarp_negatives", 0, "row", cur_slot0, P0, S)) return rc;
  if (const int rc = range_check("prewarp_negatives", 0, "column", ann_slot0, A0, S)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P0 == 0 || K == 0) {                                      // nothing to walk: count = 0, every place of `taken` is -1
    if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess || (P0 && hipMemsetAsync(taken, 0xff, sizeof(int32_t) * (size_t)P0, s) != hipSuccess))
      return premvos::fail(PREMVOS_ELAUNCH, "prewarp_negatives: memset failed");
    return PREMVOS_OK;
  }
  const int tr = (P0 + OV_TILE - 1) / OV_TILE, tc = (A0 + P0 + OV_TILE - 1) / OV_TILE;
  hipLaunchKernelGGL(neg_conflict_kernel, dim3((unsigned)(tr * tc)), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(bits),
                     (long)(stride / 8), (long)hw, cur_slot0, P0, ann_slot0, A0, conflict);
  hipLaunchKernelGGL(neg_walk_kernel, dim3(1), dim3(256), 0, s, conflict, score, P0, A0, K, taken, count);
  return premvos::check_launch("prewarp_negatives");
}

extern "C" int premvos_prewarp_gather_neg_u8(uint8_t* bits, int32_t S, int64_t stride, int32_t cur_slot0, int32_t P0, int32_t neg_slot0,
                                             int32_t n_neg, const int32_t* taken, const double* emb_p, double* emb_neg, void* stream) {
  if (const int rc = pool_check("prewarp_gather_neg", bits, S, stride, stride)) return rc;
  PV_REQUIRE(P0 >= 0 && n_neg >= 0 && n_neg <= P0, "prewarp_gather_neg: bad dims (%d negatives of %d proposals)", n_neg, P0);
  if (n_neg == 0) return PREMVOS_OK;
  PV_REQUIRE(taken && emb_p && emb_neg, "prewarp_gather_neg: null pointer");
  if (const int rc = range_check("prewarp_gather_neg", 0, "row", cur_slot0, P0, S)) return rc;
  if (const int rc = range_check("prewarp_gather_neg", 0, "column", neg_slot0, n_neg, S)) return rc;
  PV_REQUIRE((long)neg_slot0 >= (long)cur_slot0 + P0 || (long)neg_slot0 + n_neg <= cur_slot0,
             "prewarp_gather_neg: the negatives' slots %d + %d overlap the proposals' %d + %d", neg_slot0, n_neg, cur_slot0, P0);
  hipLaunchKernelGGL(neg_gather_kernel, dim3((unsigned)n_neg), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<unsigned long long*>(bits), (long)(stride / 8), cur_slot0, P0, neg_slot0, taken, emb_p, emb_neg);
  return premvos::check_launch("prewarp_gather_neg");
}
