// The selection pass of the merge loop's score kernels (merge_functions.py:107-113: argmax of the weighted row with its threshold
// column, the maximum of plane 0 + plane 1), shared by track_ops.hip (calculate_scores) and merge_modes_ops.hip (calculate_gt_scores):
// one text, so the same rows give the same selection whichever scores filled them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace premvos {

// numpy's max of two: a NaN wins
__device__ __forceinline__ double nanmax(const double a, const double b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }

// One workgroup of 256 lanes.  Per template t: the first maximum of weighted[t][0 .. P] (P + 1 entries; index P = the empty proposal)
// and the NaN-propagating maximum of plane0[t][p] + plane1[t][p].  A lane reads the columns p = lane, lane + 256, ...: those it wrote
// itself in the caller's passes, so no barrier is needed before the call.
__device__ __forceinline__ void track_select_rows(const double* __restrict__ weighted, const double* __restrict__ plane0,
                                                  const double* __restrict__ plane1, const int T, const int P,
                                                  int* __restrict__ selected, double* __restrict__ final_score,
                                                  double* __restrict__ object_score) {
  const int tid = threadIdx.x;
  __shared__ double s_v[256], s_o[256];
  __shared__ int s_i[256], s_has[256];
  for (int t = 0; t < T; ++t) {
    double bv = -INFINITY, ov = 0.0;
    int bi = 0x7fffffff, has = 0;
    for (int p = tid; p <= P; p += 256) {
      const double v = weighted[(long)t * (P + 1) + p];
      if (v > bv) { bv = v; bi = p; }
      if (p < P) {
        const double o = plane0[(long)t * P + p] + plane1[(long)t * P + p];
        ov = has ? nanmax(ov, o) : o;
        has = 1;
      }
    }
    s_v[tid] = bv; s_i[tid] = bi; s_o[tid] = ov; s_has[tid] = has;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        const double v2 = s_v[tid + s];
        const int i2 = s_i[tid + s];
        if (v2 > s_v[tid] || (v2 == s_v[tid] && i2 < s_i[tid])) { s_v[tid] = v2; s_i[tid] = i2; }
        if (s_has[tid + s]) {
          s_o[tid] = s_has[tid] ? nanmax(s_o[tid], s_o[tid + s]) : s_o[tid + s];
          s_has[tid] = 1;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      selected[t] = s_i[0];
      final_score[t] = s_v[0];
      object_score[t] = s_o[0];
    }
    __syncthreads();
  }
}

}  // namespace premvos
