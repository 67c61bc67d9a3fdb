// hipcc-flags: -ffp-contract=off
// The two swaps MergeTrack/merge.py imports next to the functions of its loop (merge.py:50-52), on the GPU:
//   * calculate_gt_scores        the oracle merge: every plane is the IoU of a candidate with the annotation of the template's object
//                                (merge_functions.py:78-94) -- one pass over the masks against the frame's label map, then the scores
//   * probabilitic_combination   the soft merge instead of argmax + remove_mask_overlap: a softmax over the candidates at
//                                temperature 0.1, a per-pixel weighted average of ALL candidate masks, the argmax over
//                                {background, objects} (merge_functions.py:151-195)
// float64 like the reference's numpy; no contraction (flag above); every floating-point sum runs in a fixed order (p ascending, one
// lane per sum), the only atomics are integer counts: two launches give the same bits.
#include "common.h"
#include "track_select.h"

#include <math.h>

namespace {

// 0x01 in every byte of `m` that is nonzero
__device__ __forceinline__ uint32_t nonzero_bytes(const uint32_t m) {
  return ((m | ((m & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;
}

// 16 bytes at p[0..16) of which only the first `valid` exist; `vec`: the 16 are there and 16-byte aligned
__device__ __forceinline__ void load16(const uint8_t* p, const int valid, const bool vec, uint32_t (&v)[4]) {
  if (vec) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * j + b < valid) word |= (uint32_t)p[4 * j + b] << (8 * b);
      v[j] = word;
    }
  }
}

// A workgroup = one candidate x 4096 pixels: the candidate's bytes and the label map's are read once and met in an LDS histogram over
// the labels 1 .. T (a lane adds a run of equal labels with one LDS atomic), then one integer atomic per label the tile met.
// Candidate 0's workgroups also count the labels' areas.
__global__ __launch_bounds__(256) void label_overlap_kernel(const uint8_t* __restrict__ masks, const uint8_t* __restrict__ labels,
                                                            const long hw, const int gx, const int P, const int T, const int vec_m,
                                                            const int vec_l, unsigned long long* __restrict__ inter,
                                                            unsigned long long* __restrict__ area_p,
                                                            unsigned long long* __restrict__ area_l) {
  __shared__ unsigned s_inter[256], s_area_l[256], s_area_p;
  const int tid = threadIdx.x;
  const int p = blockIdx.x / gx, chunk = blockIdx.x - p * gx;
  s_inter[tid] = 0;
  s_area_l[tid] = 0;
  if (tid == 0) s_area_p = 0;
  __syncthreads();
  const long p0 = ((long)chunk * 256 + tid) * 16;
  const int valid = p0 >= hw ? 0 : (hw - p0 < 16 ? (int)(hw - p0) : 16);
  uint32_t m[4] = {0, 0, 0, 0}, l[4] = {0, 0, 0, 0};
  if (valid) {
    load16(masks + (long)p * hw + p0, valid, vec_m && valid == 16, m);
    load16(labels + p0, valid, vec_l && valid == 16, l);
  }
  unsigned ca = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m[k] = nonzero_bytes(m[k]);
    ca += __popc(m[k]);
  }
  for (int off = 32; off > 0; off >>= 1) ca += __shfl_down(ca, off, 64);
  if ((tid & 63) == 0 && ca) atomicAdd(&s_area_p, ca);
  int cur = 0;                                   // the label of the run at hand (0: none, or one that does not count)
  unsigned ni = 0, na = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {                 // (bytes beyond `valid` are 0: label 0)
    const int lab = (int)((l[k >> 2] >> (8 * (k & 3))) & 0xffu);
    const int use = (lab >= 1 && lab <= T) ? lab : 0;
    if (use != cur) {
      if (cur) {
        if (ni) atomicAdd(&s_inter[cur - 1], ni);
        if (p == 0) atomicAdd(&s_area_l[cur - 1], na);
      }
      cur = use;
      ni = 0;
      na = 0;
    }
    ni += (m[k >> 2] >> (8 * (k & 3))) & 1u;
    na += 1;
  }
  if (cur) {
    if (ni) atomicAdd(&s_inter[cur - 1], ni);
    if (p == 0) atomicAdd(&s_area_l[cur - 1], na);
  }
  __syncthreads();
  if (tid < T) {
    if (s_inter[tid]) atomicAdd(&inter[(long)tid * P + p], (unsigned long long)s_inter[tid]);
    if (p == 0 && s_area_l[tid]) atomicAdd(&area_l[tid], (unsigned long long)s_area_l[tid]);
  }
  if (tid == 0 && s_area_p) atomicAdd(&area_p[p], (unsigned long long)s_area_p);
}

struct GtParams {
  double w[5];
  double thresh;
};

// One workgroup; a lane owns the columns p = lane, lane + 256, ... (track_scores_body's layout, so the selection pass of
// track_select.h reads back what the lane wrote).  IoU = 0 where the intersection is empty (pycocotools' iou of disjoint masks, and of
// the empty mask that stands for an object the annotation lacks); the five planes are the same number, the weighted sum adds
// them in plane order.
__global__ __launch_bounds__(256) void gt_scores_kernel(const long long* __restrict__ inter, const long long* __restrict__ area_p,
                                                        const long long* __restrict__ area_l, const int T, const int P,
                                                        const GtParams prm, double* __restrict__ planes, double* __restrict__ weighted,
                                                        int* __restrict__ selected, double* __restrict__ final_score,
                                                        double* __restrict__ object_score) {
  const int tid = threadIdx.x;
  const long TP = (long)T * P;
  for (int p = tid; p <= P; p += 256) {
    for (int t = 0; t < T; ++t) {
      double ws = prm.thresh;
      if (p < P) {
        const long long i = inter[(long)t * P + p];
        const long long u = i == 0 ? 1 : area_p[p] + area_l[t] - i;
        const double iou = (double)i / (double)u;
        for (int k = 0; k < 5; ++k) planes[k * TP + (long)t * P + p] = iou;
        ws = prm.w[0] * iou;
        ws += prm.w[1] * iou;
        ws += prm.w[2] * iou;
        ws += prm.w[3] * iou;
        ws += prm.w[4] * iou;
      }
      if (!isfinite(ws)) ws = 0;
      weighted[(long)t * (P + 1) + p] = ws;
    }
  }
  premvos::track_select_rows(weighted, planes, planes + TP, T, P, selected, final_score, object_score);
}

constexpr double TEMPERATURE = 0.1;      // merge_functions.py:153

// One workgroup, one lane per template (T <= 255): the row's softmax over the candidates, p ascending, without subtracting the
// maximum (merge_functions.py:156-158), the sum of the probabilities (np.average's divisor) and the row's best score
// (merge_functions.py:181).  A non-finite weighted score counts as 0, as in the live loop.
__global__ __launch_bounds__(256) void combine_probs_kernel(const double* __restrict__ weighted, const long wstride, const int T,
                                                            const int P, double* __restrict__ probs, double* __restrict__ denom,
                                                            double* __restrict__ final_score) {
  const int t = threadIdx.x;
  if (t >= T) return;
  const double* row = weighted + (long)t * wstride;
  double* out = probs + (long)t * P;
  double part = 0.0, best = -INFINITY;
  for (int p = 0; p < P; ++p) {
    double ws = row[p];
    if (!isfinite(ws)) ws = 0;
    if (ws > best) best = ws;
    const double e = exp(ws / TEMPERATURE);
    out[p] = e;
    part += e;
  }
  double sum = 0.0;
  for (int p = 0; p < P; ++p) {
    const double pr = out[p] / part;
    out[p] = pr;
    sum += pr;
  }
  denom[t] = sum;
  final_score[t] = best;
}

constexpr int TILE = 256;                // pixels per workgroup: one per lane
constexpr int PCHUNK = 1024;             // candidates whose tile bits are in LDS at a time (32 KB)
constexpr int TCHUNK = 8;                // templates whose sums a lane holds at a time

// A workgroup = 256 pixels.  The candidates' bytes of the tile are staged once as bits in LDS (a wave's ballot = 64 pixels of one
// candidate); then a lane sums, for 8 templates at a time and p ascending, the probabilities of the candidates that cover its pixel
// (merge_functions.py:162-166: np.average adds p sequentially; a candidate that does not cover the pixel adds 0, which changes
// nothing), divides by the row's divisor and keeps the first maximum.  background = 1 - that maximum; the label is the first maximum
// of [background, objects] (merge_functions.py:167-177: the second softmax is monotone, so its argmax is the argmax of its input).
// More than PCHUNK candidates: the bits are staged chunk by chunk inside each group of 8 templates.
__global__ __launch_bounds__(256) void combine_paint_kernel(const uint8_t* __restrict__ masks, const int P, const long hw,
                                                            const double* __restrict__ probs, const double* __restrict__ denom,
                                                            const int* __restrict__ ids, const int T, uint8_t* __restrict__ labels,
                                                            uint8_t* __restrict__ idmap, uint8_t* __restrict__ refined) {
  __shared__ uint32_t s_bits[PCHUNK][TILE / 32];
  __shared__ uint8_t s_id[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long tile0 = (long)blockIdx.x * TILE;
  const long pix = tile0 + tid;
  if (tid < T) s_id[tid] = (uint8_t)ids[tid];
  const int nchunks = (P + PCHUNK - 1) / PCHUNK;
  const int word = tid >> 5, bit = tid & 31;
  double mx = -INFINITY;
  int mi = -1;
  for (int t0 = 0; t0 < T; t0 += TCHUNK) {
    double acc[TCHUNK];
#pragma unroll
    for (int j = 0; j < TCHUNK; ++j) acc[j] = 0.0;
    for (int c = 0; c < nchunks; ++c) {
      const int pc0 = c * PCHUNK, pn = min(PCHUNK, P - pc0);
      if (nchunks > 1 || t0 == 0) {                                   // (uniform over the workgroup)
        __syncthreads();
        for (int q = wave; q < pn * (TILE / 64); q += 4) {            // q = candidate x 64-pixel group
          const int pl = q >> 2, g = q & 3;
          const long px = tile0 + g * 64 + lane;
          const int on = px < hw ? (masks[(long)(pc0 + pl) * hw + px] != 0) : 0;
          const unsigned long long b = __ballot(on);
          if (lane == 0) {
            s_bits[pl][2 * g] = (uint32_t)b;
            s_bits[pl][2 * g + 1] = (uint32_t)(b >> 32);
          }
        }
        __syncthreads();
      }
      for (int pl = 0; pl < pn; ++pl) {
        const bool on = (s_bits[pl][word] >> bit) & 1u;
#pragma unroll
        for (int j = 0; j < TCHUNK; ++j)
          if (t0 + j < T) acc[j] += on ? probs[(long)(t0 + j) * P + pc0 + pl] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < TCHUNK; ++j)
      if (t0 + j < T) {
        const double cmb = acc[j] / denom[t0 + j];
        if (cmb > mx) { mx = cmb; mi = t0 + j; }
      }
  }
  __syncthreads();                                                    // (s_id; T may be smaller than one staging round)
  if (pix >= hw) return;
  const double bg = 1.0 - mx;
  const int lab = (mi < 0 || bg >= mx) ? 0 : mi + 1;
  labels[pix] = (uint8_t)lab;
  idmap[pix] = lab ? s_id[lab - 1] : (uint8_t)0;
  for (int t = 0; t < T; ++t) refined[(long)t * hw + pix] = (uint8_t)(lab == t + 1);
}

}  // namespace

extern "C" int premvos_mask_label_overlap_u8(const uint8_t* masks, int32_t P, const uint8_t* labels, int32_t T, int64_t hw,
                                             int64_t* inter, int64_t* area_p, int64_t* area_l, void* stream) {
  PV_REQUIRE(masks && labels && inter && area_p && area_l, "mask_label_overlap: null pointer");
  PV_REQUIRE(P >= 1 && T >= 1 && hw >= 1 && hw < (1L << 31), "mask_label_overlap: bad dims (P %d, T %d, hw %ld)", P, T, (long)hw);
  PV_REQUIRE(T <= 255, "mask_label_overlap: at most 255 labels fit a uint8 map (got %d)", T);
  const long gx = (hw + 4095) / 4096;
  PV_REQUIRE(gx * P < (1L << 31), "mask_label_overlap: too many candidates for masks of this size");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(inter, 0, sizeof(int64_t) * (size_t)T * (size_t)P, s) != hipSuccess ||
      hipMemsetAsync(area_p, 0, sizeof(int64_t) * (size_t)P, s) != hipSuccess ||
      hipMemsetAsync(area_l, 0, sizeof(int64_t) * (size_t)T, s) != hipSuccess)
    return premvos::fail(PREMVOS_ELAUNCH, "mask_label_overlap: memset failed");
  hipLaunchKernelGGL(label_overlap_kernel, dim3((unsigned)(gx * P)), dim3(256), 0, s, masks, labels, (long)hw, (int)gx, P, T,
                     (int)(hw % 16 == 0 && premvos::aligned16(masks)), (int)premvos::aligned16(labels),
                     reinterpret_cast<unsigned long long*>(inter), reinterpret_cast<unsigned long long*>(area_p),
                     reinterpret_cast<unsigned long long*>(area_l));
  return premvos::check_launch("mask_label_overlap");
}

extern "C" int premvos_track_gt_scores_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_l, int32_t T, int32_t P,
                                           const double* weights5, double score_thresh, double* planes, double* weighted,
                                           int32_t* selected, double* final_score, double* object_score, void* stream) {
  PV_REQUIRE(inter && area_p && area_l && weights5 && planes && weighted && selected && final_score && object_score,
             "track_gt_scores: null pointer");
  PV_REQUIRE(T >= 1 && P >= 1, "track_gt_scores: bad dims (T %d, P %d)", T, P);
  PV_REQUIRE(T <= 255 && P <= 65535, "track_gt_scores: at most 255 templates and 65535 proposals (got %d, %d)", T, P);
  GtParams prm;
  for (int k = 0; k < 5; ++k) prm.w[k] = weights5[k];
  prm.thresh = score_thresh;
  hipLaunchKernelGGL(gt_scores_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(inter), reinterpret_cast<const long long*>(area_p),
                     reinterpret_cast<const long long*>(area_l), T, P, prm, planes, weighted, selected, final_score, object_score);
  return premvos::check_launch("track_gt_scores");
}

extern "C" int premvos_track_combine_f64(const uint8_t* masks, int32_t P, int32_t h, int32_t w, const double* weighted,
                                         int64_t weighted_stride, const int32_t* ids, int32_t T, double* probs, double* denom,
                                         double* final_score, uint8_t* labels, uint8_t* idmap, uint8_t* refined, void* stream) {
  PV_REQUIRE(masks && weighted && ids && probs && denom && final_score && labels && idmap && refined, "track_combine: null pointer");
  PV_REQUIRE(P >= 1 && h >= 1 && w >= 1 && T >= 1 && (long)h * w < (1L << 31), "track_combine: bad dims (P %d, h %d, w %d, T %d)", P, h, w,
             T);
  PV_REQUIRE(T <= 255, "track_combine: at most 255 objects fit uint8 labels (got %d)", T);
  PV_REQUIRE(weighted_stride >= P, "track_combine: the weighted rows' stride %ld is shorter than their %d scores", (long)weighted_stride, P);
  const long hw = (long)h * w;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(combine_probs_kernel, dim3(1), dim3(256), 0, s, weighted, (long)weighted_stride, T, P, probs, denom, final_score);
  if (const int rc = premvos::check_launch("track_combine (probabilities)")) return rc;
  hipLaunchKernelGGL(combine_paint_kernel, dim3((unsigned)((hw + TILE - 1) / TILE)), dim3(256), 0, s, masks, P, hw, probs, denom, ids, T,
                     labels, idmap, refined);
  return premvos::check_launch("track_combine");
}
