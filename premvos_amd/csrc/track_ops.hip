// hipcc-flags: -ffp-contract=off
// The merge loop's own logic on the GPU (MergeTrack/merge.py:69-115 do_video): between "the frame's candidates are in HBM" and "the
// label map is in HBM" nothing returns to the host -- the selected indices feed the paint kernel from device memory.
//   * RLE decode                 pycocotools decode of the proposals' "segmentation"   (merge_functions.py:125)
//   * scores + selection         calculate_scores, the two np.dot of merge.py:89-90, calculate_selected_props' argmax
//                                (merge_functions.py:38-76, 96-121)
//   * overlap removal + id map   remove_mask_overlap + save_pngs                        (merge_functions.py:123-149, 516-525)
// The loop is bound by launches, not bytes (T <= ~10 objects, P <= ~100 candidates): each piece is ONE launch.  float64 like the
// reference's numpy; no contraction (flag above), so a product stored in a plane and the same product inside a sum are one number,
// and every sum runs in a fixed order: two launches give the same bits.
// The *_seats_* forms run the same pieces for up to 8 videos ("seats") in one launch each (premvos_amd.track.TrackerGroup): scores and
// paint share their device functions with the one-video kernels, so they give the same bits per video; the seats' masks live in one
// pool, every other array is pooled in seat order at the offsets of SeatTable below (premvos_hip.h spells them out per array).
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

__device__ __forceinline__ void store16(uint8_t* p, const int valid, const bool vec, const uint32_t (&v)[4]) {
  if (vec) {
    *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (4 * j + b < valid) p[4 * j + b] = (uint8_t)(v[j] >> (8 * b));
  }
}

// The inverse of the run-boundary kernels of merge_ops.hip: the value of column-major position q = x*h + y is the parity of the
// number of boundaries <= q.  One lane = 16 consecutive row-major bytes of the [n][h][w] output (one binary search per byte over the
// mask's few hundred boundaries).
__global__ __launch_bounds__(256) void rle_decode_kernel(const int* __restrict__ pool, const int pool_len,
                                                         const int* __restrict__ offsets, const int n, const int h, const int w,
                                                         uint8_t* __restrict__ out, const int vec) {
  const long hw = (long)h * w, total = hw * n;
  const long f0 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (f0 >= total) return;
  int i = (int)(f0 / hw);
  const long r = f0 - (long)i * hw;
  int y = (int)(r / w), x = (int)(r - (long)y * w);
  int lo = min(max(offsets[i], 0), pool_len), hi = min(max(offsets[i + 1], lo), pool_len);
  const int valid = total - f0 < 16 ? (int)(total - f0) : 16;
  uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (k < valid) {
      const int q = x * h + y;
      int a = lo, b = hi;                       // first entry > q
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (pool[mid] <= q) a = mid + 1; else b = mid;
      }
      v[k >> 2] |= (uint32_t)((a - lo) & 1) << (8 * (k & 3));
      if (++x == w) {
        x = 0;
        if (++y == h) {
          y = 0;
          ++i;
          if (i < n) {
            lo = min(max(offsets[i], 0), pool_len);
            hi = min(max(offsets[i + 1], lo), pool_len);
          }
        }
      }
    }
  }
  store16(out + f0, valid, vec && valid == 16, v);
}

struct ScoreParams {
  double w[5];
  double thresh;
};

// V seats by value (premvos_hip.h: the seat table): seat v's T objects, F fresh proposals (0 for an empty seat), its first candidate
// and first fresh mask in the pool, and where its slices of the pooled arrays begin:
//   oT = sum_{u<v} T_u   oF = sum_{u<v} F_u   oP = sum_{u<v} (T_u + F_u)   oTP = sum_{u<v} T_u * (T_u + F_u)
constexpr int MAX_SEATS = 8;
struct SeatTable {
  int V;
  int T[MAX_SEATS], F[MAX_SEATS], cand[MAX_SEATS], fresh[MAX_SEATS];
  int oT[MAX_SEATS], oF[MAX_SEATS], oP[MAX_SEATS];
  long oTP[MAX_SEATS];
};

constexpr int EMB = 128;                 // the ReID embedding (ReID_net: 128-d)
constexpr double MAX_REID_DISTANCE = 25; // merge_functions.py:12

using premvos::nanmax;                   // track_select.h: numpy's max of two, a NaN wins

// One workgroup; a lane owns the columns p = lane, lane + 256, ... of every [T][P] plane, so whatever it reads back from a plane it
// wrote itself.  Pass 1: planes 0, 1, 3.  Pass 2: planes 2, 4 (1 - max over the OTHER templates of the same column), the weighted sum.
// Pass 3, per template: first maximum of the weighted row (P + 1 entries) and the NaN-propagating maximum of plane 0 + plane 1.
// The proposal side comes in two parts: rows [0, C) from pscore_c / emb_c, rows [C, P) from pscore_f / emb_f (row p - C) -- one array
// split anywhere for the single-video entry, the candidates and the fresh rows of a seat for the seats entry.
__device__ __forceinline__ void track_scores_body(const long long* __restrict__ inter, const long long* __restrict__ area_p,
                                                  const long long* __restrict__ area_t, const double* __restrict__ tscore,
                                                  const double* __restrict__ pscore_c, const double* __restrict__ emb_c, const int C,
                                                  const double* __restrict__ pscore_f, const double* __restrict__ emb_f,
                                                  const double* __restrict__ emb_t, const int T, const int P, const ScoreParams& prm,
                                                  double* __restrict__ planes, double* __restrict__ weighted, int* __restrict__ selected,
                                                  double* __restrict__ final_score, double* __restrict__ object_score) {
  const int tid = threadIdx.x;
  const long TP = (long)T * P;
  double* mask_s = planes;
  double* reid_s = planes + TP;
  double* oreid_s = planes + 2 * TP;
  double* warp_s = planes + 3 * TP;
  double* owarp_s = planes + 4 * TP;
  for (int p = tid; p < P; p += 256) {
    const double ms = fmax((p < C ? pscore_c[p] : pscore_f[p - C]) - 0.5, 0.0) / (1 - 0.5);
    const double* ep = p < C ? emb_c + (long)p * EMB : emb_f + (long)(p - C) * EMB;
    const long long ap = area_p[p];
    for (int t = 0; t < T; ++t) {
      const double* et = emb_t + (long)t * EMB;
      double acc = 0.0;
      for (int k = 0; k < EMB; ++k) {
        const double d = ep[k] - et[k];
        acc += d * d;
      }
      double rs = 1 - sqrt(acc) / MAX_REID_DISTANCE;
      if (isinf(rs)) rs = 0;
      if (rs < 0) rs = 0;
      const long long i = inter[(long)t * P + p];
      const long long u = i == 0 ? 1 : ap + area_t[t] - i;
      const double wsw = fmax(tscore[t] - 0.5, 0.0) / (1 - 0.5);
      mask_s[(long)t * P + p] = ms;
      reid_s[(long)t * P + p] = rs;
      warp_s[(long)t * P + p] = ((double)i / (double)u) * wsw;
    }
  }
  for (int p = tid; p <= P; p += 256) {
    for (int t = 0; t < T; ++t) {
      double ws = prm.thresh;
      if (p < P) {
        double orr = 1.0, ow = 1.0;
        if (T > 1) {
          const int first = t == 0 ? 1 : 0;
          double mr = reid_s[(long)first * P + p], mw = warp_s[(long)first * P + p];
          for (int o = first + 1; o < T; ++o)
            if (o != t) {
              mr = nanmax(mr, reid_s[(long)o * P + p]);
              mw = nanmax(mw, warp_s[(long)o * P + p]);
            }
          orr = 1 - mr;
          ow = 1 - mw;
        }
        oreid_s[(long)t * P + p] = orr;
        owarp_s[(long)t * P + p] = ow;
        ws = prm.w[0] * mask_s[(long)t * P + p];
        ws += prm.w[1] * reid_s[(long)t * P + p];
        ws += prm.w[2] * orr;
        ws += prm.w[3] * warp_s[(long)t * P + p];
        ws += prm.w[4] * ow;
      }
      if (!isfinite(ws)) ws = 0;
      weighted[(long)t * (P + 1) + p] = ws;
    }
  }
  premvos::track_select_rows(weighted, mask_s, reid_s, T, P, selected, final_score, object_score);      // pass 3: track_select.h
}

__global__ __launch_bounds__(256) void track_scores_kernel(const long long* __restrict__ inter, const long long* __restrict__ area_p,
                                                           const long long* __restrict__ area_t, const double* __restrict__ tscore,
                                                           const double* __restrict__ pscore, const double* __restrict__ emb_p,
                                                           const double* __restrict__ emb_t, const int T, const int P,
                                                           const ScoreParams prm, double* __restrict__ planes,
                                                           double* __restrict__ weighted, int* __restrict__ selected,
                                                           double* __restrict__ final_score, double* __restrict__ object_score) {
  track_scores_body(inter, area_p, area_t, tscore, pscore, emb_p, P, pscore, emb_p, emb_t, T, P, prm, planes, weighted, selected,
                    final_score, object_score);
}

// One workgroup per seat: the same body on the seat's slices of the pooled arrays (offsets: SeatTable).  The template score is the
// candidate score of the same slot (Tracker.step); the proposal side is the seat's candidates, then its fresh rows.
__global__ __launch_bounds__(256) void track_scores_seats_kernel(const long long* __restrict__ inter, const long long* __restrict__ area_p,
                                                                 const long long* __restrict__ area_t, const double* __restrict__ cand_score,
                                                                 const double* __restrict__ cand_emb, const double* __restrict__ templ_emb,
                                                                 const double* __restrict__ fresh_score, const double* __restrict__ fresh_emb,
                                                                 const SeatTable st, const ScoreParams prm, double* __restrict__ planes,
                                                                 double* __restrict__ weighted, int* __restrict__ selected,
                                                                 double* __restrict__ final_score, double* __restrict__ object_score) {
  const int v = blockIdx.x;
  const int T = st.T[v], P = T + st.F[v];
  if (T == 0) return;
  const long oT = st.oT[v], oF = st.oF[v], oTP = st.oTP[v];
  track_scores_body(inter + oTP, area_p + st.oP[v], area_t + oT, cand_score + oT, cand_score + oT, cand_emb + oT * EMB, T,
                    fresh_score + oF, fresh_emb + oF * EMB, templ_emb + oT * EMB, T, P, prm, planes + 5 * oTP, weighted + oTP + oT,
                    selected + oT, final_score + oT, object_score + oT);
}

// The weight search's scores (premvos_amd.track.SearchGroup): the seats run ONE video under V weight sets, so each has a weight row of
// its own (by value, like the seat table) and all of them read the SAME F fresh rows -- fresh_score / fresh_emb carry no seat offset.
// The body, its order of sums and the output layout are track_scores_seats_kernel's.
struct WeightSets {
  double w[MAX_SEATS][5];
  double thresh;
};
__global__ __launch_bounds__(256) void track_scores_sets_kernel(const long long* __restrict__ inter, const long long* __restrict__ area_p,
                                                                const long long* __restrict__ area_t, const double* __restrict__ cand_score,
                                                                const double* __restrict__ cand_emb, const double* __restrict__ templ_emb,
                                                                const double* __restrict__ fresh_score, const double* __restrict__ fresh_emb,
                                                                const SeatTable st, const WeightSets ws, double* __restrict__ planes,
                                                                double* __restrict__ weighted, int* __restrict__ selected,
                                                                double* __restrict__ final_score, double* __restrict__ object_score) {
  const int v = blockIdx.x;
  const int T = st.T[v], P = T + st.F[v];
  if (T == 0) return;
  ScoreParams prm;
  for (int k = 0; k < 5; ++k) prm.w[k] = ws.w[v][k];
  prm.thresh = ws.thresh;
  const long oT = st.oT[v], oTP = st.oTP[v];
  track_scores_body(inter + oTP, area_p + st.oP[v], area_t + oT, cand_score + oT, cand_score + oT, cand_emb + oT * EMB, T, fresh_score,
                    fresh_emb, templ_emb + oT * EMB, T, P, prm, planes + 5 * oTP, weighted + oTP + oT, selected + oT, final_score + oT,
                    object_score + oT);
}

// remove_mask_overlap paints the selections in ascending order of score, so the highest score is painted last; equal scores are
// ordered by index here (the higher index last).  The order is found per workgroup (T <= 255 keys), then a lane paints 16 pixels.
// Selection p of the object is mask cand_slot + p of `masks` for p < C, mask fresh_slot + p - C from there on.
__device__ __forceinline__ void track_paint_body(const uint8_t* __restrict__ masks, const int P, const long hw, const int cand_slot,
                                                 const int C, const int fresh_slot, const int* __restrict__ selected,
                                                 const double* __restrict__ final_score, const int* __restrict__ ids, const int T,
                                                 uint8_t* __restrict__ labels, uint8_t* __restrict__ idmap,
                                                 uint8_t* __restrict__ refined, const int vec) {
  __shared__ int s_sel[256];
  __shared__ uint8_t s_order[256], s_id[256];
  const int tid = threadIdx.x;
  if (tid < T) {
    double key = final_score[tid];
    if (key != key) key = INFINITY;
    int rank = 0;
    for (int o = 0; o < T; ++o) {
      double ko = final_score[o];
      if (ko != ko) ko = INFINITY;
      rank += ko < key || (ko == key && o < tid);
    }
    s_order[rank] = (uint8_t)tid;
    const int sel = selected[tid];
    s_sel[tid] = (sel >= 0 && sel < P) ? (sel < C ? cand_slot + sel : fresh_slot + sel - C) : -1;         // P = the empty proposal
    s_id[tid] = (uint8_t)ids[tid];
  }
  __syncthreads();
  const long p0 = ((long)blockIdx.x * 256 + tid) * 16;
  if (p0 >= hw) return;
  const int valid = hw - p0 < 16 ? (int)(hw - p0) : 16;
  const bool v16 = vec && valid == 16;
  uint32_t lab[4] = {0, 0, 0, 0};
  for (int r = 0; r < T; ++r) {
    const int t = s_order[r];
    const int sel = s_sel[t];
    if (sel < 0) continue;
    uint32_t m[4];
    load16(masks + (long)sel * hw + p0, valid, v16, m);
    const uint32_t val = (uint32_t)(t + 1) * 0x01010101u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t full = nonzero_bytes(m[j]) * 0xffu;
      lab[j] = (lab[j] & ~full) | (val & full);
    }
  }
  store16(labels + p0, valid, v16, lab);
  uint32_t idw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t l = (lab[j] >> (8 * b)) & 0xffu;
      word |= (l ? (uint32_t)s_id[l - 1] : 0u) << (8 * b);
    }
    idw[j] = word;
  }
  store16(idmap + p0, valid, v16, idw);
  for (int t = 0; t < T; ++t) {
    const uint32_t val = (uint32_t)(t + 1) * 0x01010101u;
    uint32_t eq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) eq[j] = nonzero_bytes(lab[j] ^ val) ^ 0x01010101u;
    store16(refined + (long)t * hw + p0, valid, v16, eq);
  }
}

__global__ __launch_bounds__(256) void track_paint_kernel(const uint8_t* __restrict__ masks, const int P, const long hw,
                                                          const int* __restrict__ selected, const double* __restrict__ final_score,
                                                          const int* __restrict__ ids, const int T, uint8_t* __restrict__ labels,
                                                          uint8_t* __restrict__ idmap, uint8_t* __restrict__ refined, const int vec) {
  track_paint_body(masks, P, hw, 0, P, 0, selected, final_score, ids, T, labels, idmap, refined, vec);
}

// grid (pixel blocks, V): seat v paints plane v of labels / idmap and its T planes of `refined` from refined_slot[v] on.
struct RefinedSlots { int slot[MAX_SEATS]; };
__global__ __launch_bounds__(256) void track_paint_seats_kernel(const uint8_t* __restrict__ masks, const long hw, const SeatTable st,
                                                                const RefinedSlots rs, const int* __restrict__ selected,
                                                                const double* __restrict__ final_score, const int* __restrict__ ids,
                                                                uint8_t* __restrict__ labels, uint8_t* __restrict__ idmap,
                                                                uint8_t* __restrict__ refined, const int vec) {
  const int v = blockIdx.y;
  const int T = st.T[v];
  if (T == 0) return;
  const long oT = st.oT[v];
  track_paint_body(masks, T + st.F[v], hw, st.cand[v], T, st.fresh[v], selected + oT, final_score + oT, ids + oT, T, labels + v * hw,
                   idmap + v * hw, refined + (long)rs.slot[v] * hw, vec);
}

// premvos_mask_overlap_u8's counts for the (template, proposal) pairs of each seat only.  A workgroup = one proposal of one seat x
// 4096 pixels: the proposal's bytes are read once and met with each of the seat's T templates; a wave sums its lanes' counts, the
// workgroup's sums meet in LDS, then one integer atomic per count (the result does not depend on the order of arrival).
__global__ __launch_bounds__(256) void overlap_seats_kernel(const uint8_t* __restrict__ masks, const long hw, const int gx,
                                                            const SeatTable st, const int vec, unsigned long long* __restrict__ inter,
                                                            unsigned long long* __restrict__ area_p,
                                                            unsigned long long* __restrict__ area_t) {
  __shared__ unsigned s_inter[256], s_area_t[256], s_area_p;
  const int tid = threadIdx.x;
  const int j = blockIdx.x / gx, chunk = blockIdx.x - j * gx;      // j: the proposal's place in the pooled area_p
  int v = 0;
  while (v + 1 < st.V && j >= st.oP[v] + st.T[v] + st.F[v]) ++v;
  const int T = st.T[v], P = T + st.F[v], p = j - st.oP[v];
  const uint8_t* prop = masks + (long)(p < T ? st.cand[v] + p : st.fresh[v] + p - T) * hw;
  s_inter[tid] = 0;
  s_area_t[tid] = 0;
  if (tid == 0) s_area_p = 0;
  __syncthreads();
  const long p0 = ((long)chunk * 256 + tid) * 16;
  const int valid = p0 >= hw ? 0 : (hw - p0 < 16 ? (int)(hw - p0) : 16);
  const bool v16 = vec && valid == 16;
  uint32_t a[4] = {0, 0, 0, 0};
  if (valid) load16(prop + p0, valid, v16, a);
  unsigned ca = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[k] = nonzero_bytes(a[k]);
    ca += __popc(a[k]);
  }
  for (int off = 32; off > 0; off >>= 1) ca += __shfl_down(ca, off, 64);
  if ((tid & 63) == 0 && ca) atomicAdd(&s_area_p, ca);
  for (int t = 0; t < T; ++t) {
    uint32_t b[4] = {0, 0, 0, 0};
    if (valid) load16(masks + (long)(st.cand[v] + t) * hw + p0, valid, v16, b);
    unsigned c = 0;                                                  // area in the high half, intersection in the low: <= 16 per lane
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[k] = nonzero_bytes(b[k]);
      c += (__popc(b[k]) << 16) + __popc(a[k] & b[k]);
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((tid & 63) == 0) {
      if (c & 0xffffu) atomicAdd(&s_inter[t], c & 0xffffu);
      if (p == 0 && (c >> 16)) atomicAdd(&s_area_t[t], c >> 16);
    }
  }
  __syncthreads();
  if (tid < T) {
    if (s_inter[tid]) atomicAdd(&inter[st.oTP[v] + (long)tid * P + p], (unsigned long long)s_inter[tid]);
    if (p == 0 && s_area_t[tid]) atomicAdd(&area_t[st.oT[v] + tid], (unsigned long long)s_area_t[tid]);
  }
  if (tid == 0 && s_area_p) atomicAdd(&area_p[j], (unsigned long long)s_area_p);
}

// eval_video's pixel work (merge_functions.py:613-634) for every seat of one frame: plane first[v] + k of `planes` is seat v's object
// k after overlap removal (what track_paint_seats_kernel wrote), G = (gt == k + 1).  A lane reads 16 bytes of gt once and, per seat and
// object, 16 bytes of the plane; a wave sums its lanes' popcounts, the workgroup's waves meet in LDS (one seat's 3 T0 counts at a
// time), then one integer atomic per count and workgroup: the result does not depend on the order of arrival.
struct FirstPlanes { int first[MAX_SEATS]; };
__global__ __launch_bounds__(256) void track_eval_seats_kernel(const uint8_t* __restrict__ planes, const uint8_t* __restrict__ gt,
                                                               const long hw, const int V, const int T0, const FirstPlanes fp,
                                                               const int vec, unsigned long long* __restrict__ counts,
                                                               const long seat_stride) {
  __shared__ unsigned s_cnt[3 * 256];
  const int tid = threadIdx.x;
  const long p0 = ((long)blockIdx.x * 256 + tid) * 16;
  const int valid = p0 >= hw ? 0 : (hw - p0 < 16 ? (int)(hw - p0) : 16);
  const bool v16 = vec && valid == 16;
  uint32_t g[4] = {0, 0, 0, 0};
  if (valid) load16(gt + p0, valid, v16, g);
  for (int v = 0; v < V; ++v) {
    for (int i = tid; i < 3 * T0; i += 256) s_cnt[i] = 0;
    __syncthreads();
    for (int k = 0; k < T0; ++k) {
      uint32_t r[4] = {0, 0, 0, 0};
      if (valid) load16(planes + (long)(fp.first[v] + k) * hw + p0, valid, v16, r);
      const uint32_t val = (uint32_t)(k + 1) * 0x01010101u;
      unsigned iu = 0, ar = 0;                                         // intersection in the low half, union in the high: <= 16 per lane
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t rb = nonzero_bytes(r[j]);
        const uint32_t gb = valid ? nonzero_bytes(g[j] ^ val) ^ 0x01010101u : 0u;
        iu += (__popc(rb | gb) << 16) + __popc(rb & gb);
        ar += __popc(rb);
      }
      for (int off = 32; off > 0; off >>= 1) {
        iu += __shfl_down(iu, off, 64);
        ar += __shfl_down(ar, off, 64);
      }
      if ((tid & 63) == 0) {
        if (iu & 0xffffu) atomicAdd(&s_cnt[3 * k], iu & 0xffffu);
        if (iu >> 16) atomicAdd(&s_cnt[3 * k + 1], iu >> 16);
        if (ar) atomicAdd(&s_cnt[3 * k + 2], ar);
      }
    }
    __syncthreads();
    for (int i = tid; i < 3 * T0; i += 256)
      if (s_cnt[i]) atomicAdd(&counts[v * seat_stride + i], (unsigned long long)s_cnt[i]);
    __syncthreads();
  }
}

// The proposal side of track_scores_kernel for P = T + F rows, built where the parts already are: rows [0, T) = the carried candidates
// (float64, copied), rows [T, P) = the frame's fresh proposals -- their float32 ReID rows widened (exactly what the float32 values
// printed into ReID_proposals/*.json and parsed back give), or +inf x 128 where the row's box (int32 bits in columns 130, 131) has
// w <= 0 or h <= 0: such a proposal has no "ReID" key in the file (read_props, merge_functions.py:27-36).  One lane per value.
__global__ __launch_bounds__(256) void track_inputs_kernel(const double* __restrict__ cand_score, const double* __restrict__ cand_emb,
                                                           const double* __restrict__ fresh_score, const float* __restrict__ fresh_rows,
                                                           const int T, const int F, double* __restrict__ proposal_score,
                                                           double* __restrict__ emb_p) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)(T + F) * EMB) return;
  const int p = (int)(i / EMB), k = (int)(i - (long)p * EMB);
  if (p < T) {
    emb_p[i] = cand_emb[i];
    if (k == 0) proposal_score[p] = cand_score[p];
    return;
  }
  const float* row = fresh_rows + (long)(p - T) * (EMB + 4);
  const int bw = __float_as_int(row[EMB + 2]), bh = __float_as_int(row[EMB + 3]);
  emb_p[i] = (bw <= 0 || bh <= 0) ? (double)INFINITY : (double)row[k];
  if (k == 0) proposal_score[p] = fresh_score[p - T];
}

// warp_proposals' 'score' (merge_functions.py:234: 0.5 * (final_score + 1), the sum first; no contraction in this file) and the
// refinement net's boxes (y0, x0, y1, x1) of the warped masks' rleToBbox boxes (x, y, w, h).  One lane per object.
__global__ __launch_bounds__(64) void track_next_kernel(const double* __restrict__ final_score, const int* __restrict__ bbox_xywh,
                                                        const int T, double* __restrict__ cand_score, float* __restrict__ boxes_yx) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  const double s = final_score[t] + 1;
  cand_score[t] = 0.5 * s;
  const int x = bbox_xywh[4 * t], y = bbox_xywh[4 * t + 1], w = bbox_xywh[4 * t + 2], h = bbox_xywh[4 * t + 3];
  boxes_yx[4 * t] = (float)y;
  boxes_yx[4 * t + 1] = (float)x;
  boxes_yx[4 * t + 2] = (float)(y + h);
  boxes_yx[4 * t + 3] = (float)(x + w);
}

}  // namespace

extern "C" int premvos_rle_decode_u8(const int32_t* pool, int32_t pool_len, const int32_t* offsets, int32_t n, int32_t h, int32_t w,
                                     uint8_t* out, void* stream) {
  PV_REQUIRE(n >= 0 && h > 0 && w > 0 && pool_len >= 0, "rle_decode: bad dims");
  if (n == 0) return PREMVOS_OK;
  PV_REQUIRE(offsets && out && (pool || pool_len == 0), "rle_decode: null pointer");
  PV_REQUIRE((long)h * w < (1L << 31), "rle_decode: mask too large");
  const long groups = ((long)h * w * n + 15) / 16;
  PV_REQUIRE((groups + 255) / 256 < (1L << 31), "rle_decode: too many masks");
  hipLaunchKernelGGL(rle_decode_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pool,
                     pool_len, offsets, n, h, w, out, (int)premvos::aligned16(out));
  return premvos::check_launch("rle_decode");
}

extern "C" int premvos_track_scores_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_t, const double* template_score,
                                        const double* proposal_score, const double* emb_p, const double* emb_t, int32_t T, int32_t P,
                                        const double* weights5, double score_thresh, double* planes, double* weighted,
                                        int32_t* selected, double* final_score, double* object_score, void* stream) {
  PV_REQUIRE(inter && area_p && area_t && template_score && proposal_score && emb_p && emb_t && weights5 && planes && weighted &&
                 selected && final_score && object_score, "track_scores: null pointer");
  PV_REQUIRE(T >= 1 && P >= 1, "track_scores: bad dims");
  PV_REQUIRE(T <= 255 && P <= 65535, "track_scores: at most 255 templates and 65535 proposals (got %d, %d)", T, P);
  ScoreParams prm;
  for (int k = 0; k < 5; ++k) prm.w[k] = weights5[k];
  prm.thresh = score_thresh;
  hipLaunchKernelGGL(track_scores_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(inter), reinterpret_cast<const long long*>(area_p),
                     reinterpret_cast<const long long*>(area_t), template_score, proposal_score, emb_p, emb_t, T, P, prm, planes,
                     weighted, selected, final_score, object_score);
  return premvos::check_launch("track_scores");
}

extern "C" int premvos_track_paint_u8(const uint8_t* masks, int32_t P, int32_t h, int32_t w, const int32_t* selected,
                                      const double* final_score, const int32_t* ids, int32_t T, uint8_t* labels, uint8_t* idmap,
                                      uint8_t* refined, void* stream) {
  PV_REQUIRE(selected && final_score && ids && labels && idmap && refined && (masks || P == 0), "track_paint: null pointer");
  PV_REQUIRE(P >= 0 && h > 0 && w > 0 && T >= 1, "track_paint: bad dims");
  PV_REQUIRE(T <= 255, "track_paint: at most 255 objects fit uint8 labels (got %d)", T);
  const long hw = (long)h * w;
  const int vec = hw % 16 == 0 && premvos::aligned16(masks) && premvos::aligned16(labels) && premvos::aligned16(idmap) &&
                  premvos::aligned16(refined);
  hipLaunchKernelGGL(track_paint_kernel, dim3((unsigned)((hw + 4095) / 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), masks, P,
                     hw, selected, final_score, ids, T, labels, idmap, refined, vec);
  return premvos::check_launch("track_paint");
}

// The seat table's checks, shared by the three seats entries (before any HIP call).  S < 0: the entry has no mask pool.
static int seat_table(const char* what, const int32_t* seats, const int32_t V, const long S, SeatTable& st) {
  if (!seats) return premvos::fail(PREMVOS_EINVAL, "%s: null pointer", what);
  if (V < 1 || V > MAX_SEATS) return premvos::fail(PREMVOS_EINVAL, "%s: 1 to %d seats (got %d)", what, MAX_SEATS, V);
  st.V = V;
  long oT = 0, oF = 0, oTP = 0;
  for (int v = 0; v < MAX_SEATS; ++v) {
    const int T = v < V ? seats[4 * v] : 0, F = v < V && T != 0 ? seats[4 * v + 1] : 0;      // an empty seat's F does not count
    const int cand = v < V ? seats[4 * v + 2] : 0, fresh = v < V ? seats[4 * v + 3] : 0;
    if (T < 0 || F < 0) return premvos::fail(PREMVOS_EINVAL, "%s: seat %d: negative count (T %d, F %d)", what, v, T, F);
    if (T > 255 || T + (long)F > 65535)
      return premvos::fail(PREMVOS_EINVAL, "%s: seat %d: at most 255 templates and 65535 proposals (got %d, %d)", what, v, T, T + F);
    if (T && S >= 0) {
      if (cand < 0 || (F && fresh < 0)) return premvos::fail(PREMVOS_EINVAL, "%s: seat %d: negative slot (%d, %d)", what, v, cand, fresh);
      if (cand + (long)T > S || (F && fresh + (long)F > S))
        return premvos::fail(PREMVOS_EINVAL, "%s: seat %d: slots %d + %d, %d + %d beyond the pool's %ld masks", what, v, cand, T, fresh, F, S);
    }
    st.T[v] = T; st.F[v] = F; st.cand[v] = T ? cand : 0; st.fresh[v] = F ? fresh : 0;
    st.oT[v] = (int)oT; st.oF[v] = (int)oF; st.oP[v] = (int)(oT + oF); st.oTP[v] = oTP;
    oT += T; oF += F; oTP += (long)T * (T + F);
  }
  return PREMVOS_OK;
}

extern "C" int premvos_mask_overlap_seats_u8(const uint8_t* masks, int32_t S, int64_t hw, const int32_t* seats, int32_t V, int64_t* inter,
                                             int64_t* area_p, int64_t* area_t, void* stream) {
  PV_REQUIRE(masks && seats && inter && area_p && area_t, "mask_overlap_seats: null pointer");
  PV_REQUIRE(S > 0 && hw > 0 && hw < (1L << 31), "mask_overlap_seats: bad dims");
  SeatTable st;
  if (const int rc = seat_table("mask_overlap_seats", seats, V, S, st)) return rc;
  const long nT = st.oT[MAX_SEATS - 1] + st.T[MAX_SEATS - 1], nP = st.oP[MAX_SEATS - 1] + st.T[MAX_SEATS - 1] + st.F[MAX_SEATS - 1];
  const long nTP = st.oTP[MAX_SEATS - 1] + (long)st.T[MAX_SEATS - 1] * (st.T[MAX_SEATS - 1] + st.F[MAX_SEATS - 1]);
  if (nT == 0) return PREMVOS_OK;
  const long gx = (hw + 4095) / 4096;
  PV_REQUIRE(gx * nP < (1L << 31), "mask_overlap_seats: too many proposals for masks of this size");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(inter, 0, sizeof(int64_t) * (size_t)nTP, s) != hipSuccess ||
      hipMemsetAsync(area_p, 0, sizeof(int64_t) * (size_t)nP, s) != hipSuccess ||
      hipMemsetAsync(area_t, 0, sizeof(int64_t) * (size_t)nT, s) != hipSuccess)
    return premvos::fail(PREMVOS_ELAUNCH, "mask_overlap_seats: memset failed");
  hipLaunchKernelGGL(overlap_seats_kernel, dim3((unsigned)(gx * nP)), dim3(256), 0, s, masks, (long)hw, (int)gx, st,
                     (int)(hw % 16 == 0 && premvos::aligned16(masks)), reinterpret_cast<unsigned long long*>(inter),
                     reinterpret_cast<unsigned long long*>(area_p), reinterpret_cast<unsigned long long*>(area_t));
  return premvos::check_launch("mask_overlap_seats");
}

extern "C" int premvos_track_scores_seats_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_t, const double* cand_score,
                                              const double* cand_emb, const double* templ_emb, const double* fresh_score,
                                              const double* fresh_emb, const int32_t* seats, int32_t V, const double* weights5,
                                              double score_thresh, double* planes, double* weighted, int32_t* selected,
                                              double* final_score, double* object_score, void* stream) {
  PV_REQUIRE(inter && area_p && area_t && cand_score && cand_emb && templ_emb && seats && weights5 && planes && weighted && selected &&
                 final_score && object_score, "track_scores_seats: null pointer");
  SeatTable st;
  if (const int rc = seat_table("track_scores_seats", seats, V, -1, st)) return rc;
  const long nT = st.oT[MAX_SEATS - 1] + st.T[MAX_SEATS - 1], nF = st.oF[MAX_SEATS - 1] + st.F[MAX_SEATS - 1];
  PV_REQUIRE(nF == 0 || (fresh_score && fresh_emb), "track_scores_seats: null pointer (fresh rows)");
  if (nT == 0) return PREMVOS_OK;
  ScoreParams prm;
  for (int k = 0; k < 5; ++k) prm.w[k] = weights5[k];
  prm.thresh = score_thresh;
  hipLaunchKernelGGL(track_scores_seats_kernel, dim3(V), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(inter), reinterpret_cast<const long long*>(area_p),
                     reinterpret_cast<const long long*>(area_t), cand_score, cand_emb, templ_emb, fresh_score, fresh_emb, st, prm, planes,
                     weighted, selected, final_score, object_score);
  return premvos::check_launch("track_scores_seats");
}

extern "C" int premvos_track_scores_sets_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_t, const double* cand_score,
                                             const double* cand_emb, const double* templ_emb, const double* fresh_score,
                                             const double* fresh_emb, const int32_t* seats, int32_t V, const double* weights,
                                             double score_thresh, double* planes, double* weighted, int32_t* selected,
                                             double* final_score, double* object_score, void* stream) {
  PV_REQUIRE(inter && area_p && area_t && cand_score && cand_emb && templ_emb && seats && weights && planes && weighted && selected &&
                 final_score && object_score, "track_scores_sets: null pointer");
  SeatTable st;
  if (const int rc = seat_table("track_scores_sets", seats, V, -1, st)) return rc;
  const long nT = st.oT[MAX_SEATS - 1] + st.T[MAX_SEATS - 1];
  int F = -1;
  for (int v = 0; v < V; ++v)
    if (st.T[v]) {
      PV_REQUIRE(F < 0 || st.F[v] == F, "track_scores_sets: seat %d has %d fresh rows, the seats before it %d: they share one block", v,
                 st.F[v], F);
      F = st.F[v];
    }
  PV_REQUIRE(F <= 0 || (fresh_score && fresh_emb), "track_scores_sets: null pointer (fresh rows)");
  if (nT == 0) return PREMVOS_OK;
  WeightSets ws;
  for (int v = 0; v < MAX_SEATS; ++v)
    for (int k = 0; k < 5; ++k) ws.w[v][k] = v < V ? weights[5 * v + k] : 0.0;
  ws.thresh = score_thresh;
  hipLaunchKernelGGL(track_scores_sets_kernel, dim3(V), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(inter), reinterpret_cast<const long long*>(area_p),
                     reinterpret_cast<const long long*>(area_t), cand_score, cand_emb, templ_emb, fresh_score, fresh_emb, st, ws, planes,
                     weighted, selected, final_score, object_score);
  return premvos::check_launch("track_scores_sets");
}

extern "C" int premvos_track_eval_seats_i64(const uint8_t* planes, int32_t R, int32_t h, int32_t w, const uint8_t* gt, int32_t V, int32_t T0,
                                            const int32_t* first_plane, int64_t* counts, int64_t seat_stride, void* stream) {
  PV_REQUIRE(planes && gt && first_plane && counts, "track_eval_seats: null pointer");
  PV_REQUIRE(V >= 1 && V <= MAX_SEATS, "track_eval_seats: 1 to %d seats (got %d)", MAX_SEATS, V);
  PV_REQUIRE(R > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31) && T0 >= 0, "track_eval_seats: bad dims");
  PV_REQUIRE(T0 <= 255, "track_eval_seats: at most 255 objects (got %d)", T0);
  PV_REQUIRE(seat_stride >= 3L * T0, "track_eval_seats: the seats' counts overlap (stride %ld, %d objects)", (long)seat_stride, T0);
  FirstPlanes fp;
  for (int v = 0; v < MAX_SEATS; ++v) {
    fp.first[v] = v < V ? first_plane[v] : 0;
    PV_REQUIRE(fp.first[v] >= 0 && fp.first[v] + (long)T0 <= R, "track_eval_seats: seat %d: planes %d + %d outside the %d planes", v,
               fp.first[v], T0, R);
  }
  if (T0 == 0) return PREMVOS_OK;
  const long hw = (long)h * w;
  const int vec = hw % 16 == 0 && premvos::aligned16(planes) && premvos::aligned16(gt);
  hipLaunchKernelGGL(track_eval_seats_kernel, dim3((unsigned)((hw + 4095) / 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), planes,
                     gt, hw, V, T0, fp, vec, reinterpret_cast<unsigned long long*>(counts), (long)seat_stride);
  return premvos::check_launch("track_eval_seats");
}

extern "C" int premvos_track_paint_seats_u8(const uint8_t* masks, int32_t S, int32_t h, int32_t w, const int32_t* seats, int32_t V,
                                            const int32_t* selected, const double* final_score, const int32_t* ids, uint8_t* labels,
                                            uint8_t* idmap, uint8_t* refined, int32_t R, const int32_t* refined_slots, void* stream) {
  PV_REQUIRE(masks && seats && selected && final_score && ids && labels && idmap && refined && refined_slots,
             "track_paint_seats: null pointer");
  PV_REQUIRE(S > 0 && R > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31), "track_paint_seats: bad dims");
  SeatTable st;
  if (const int rc = seat_table("track_paint_seats", seats, V, S, st)) return rc;
  RefinedSlots rs;
  long nT = 0;
  for (int v = 0; v < MAX_SEATS; ++v) {
    rs.slot[v] = v < V && st.T[v] ? refined_slots[v] : 0;
    PV_REQUIRE(rs.slot[v] >= 0 && rs.slot[v] + (long)st.T[v] <= R, "track_paint_seats: seat %d: refined slots %d + %d outside the %d planes",
               v, rs.slot[v], st.T[v], R);
    nT += st.T[v];
  }
  if (nT == 0) return PREMVOS_OK;
  const long hw = (long)h * w;
  const int vec = hw % 16 == 0 && premvos::aligned16(masks) && premvos::aligned16(labels) && premvos::aligned16(idmap) &&
                  premvos::aligned16(refined);
  hipLaunchKernelGGL(track_paint_seats_kernel, dim3((unsigned)((hw + 4095) / 4096), V), dim3(256), 0, static_cast<hipStream_t>(stream),
                     masks, hw, st, rs, selected, final_score, ids, labels, idmap, refined, vec);
  return premvos::check_launch("track_paint_seats");
}

extern "C" int premvos_track_inputs_f64(const double* cand_score, const double* cand_emb, const double* fresh_score,
                                        const float* fresh_rows, int32_t T, int32_t F, double* proposal_score, double* emb_p,
                                        void* stream) {
  PV_REQUIRE(T >= 0 && F >= 0, "track_inputs: negative count (T %d, F %d)", T, F);
  PV_REQUIRE(T <= 255 && T + (long)F <= 65535, "track_inputs: at most 255 templates and 65535 proposals (got %d, %d)", T, F);
  PV_REQUIRE(proposal_score && emb_p && (T == 0 || (cand_score && cand_emb)) && (F == 0 || (fresh_score && fresh_rows)),
             "track_inputs: null pointer");
  if (T + F == 0) return PREMVOS_OK;
  const long total = (long)(T + F) * EMB;
  hipLaunchKernelGGL(track_inputs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     cand_score, cand_emb, fresh_score, fresh_rows, T, F, proposal_score, emb_p);
  return premvos::check_launch("track_inputs");
}

extern "C" int premvos_track_next_f32(const double* final_score, const int32_t* bbox_xywh, int32_t T, double* cand_score,
                                      float* boxes_y0x0y1x1, void* stream) {
  PV_REQUIRE(T >= 0, "track_next: negative count (T %d)", T);
  PV_REQUIRE(final_score && bbox_xywh && cand_score && boxes_y0x0y1x1, "track_next: null pointer");
  if (T == 0) return PREMVOS_OK;
  hipLaunchKernelGGL(track_next_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), final_score,
                     bbox_xywh, T, cand_score, boxes_y0x0y1x1);
  return premvos::check_launch("track_next");
}
