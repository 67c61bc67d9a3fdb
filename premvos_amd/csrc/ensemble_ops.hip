// The combination of MergeTrack/oldmerge.py's ensemble runs (oldmerge.py:129-131,220-224: do_video(video_fn, ensemble_num) once per row
// of weight_set, each run's PNGs under to_ensemble/<n>/): K id maps of one video -> one, by a per-pixel vote.
//   * the winner of a pixel is the label that most of the K sets painted there; among labels with equally many votes the one of the
//     set listed first wins (callers list their best set first); label 0, the background, votes like any other
//   * votes[p] = how many sets agree with the winner, hist[v] += the number of pixels decided by v votes
// HBM-bound byte work without reuse: a lane owns 16 pixels at a time -- one 16-byte load per set, the K vectors stay in registers,
// the K (K - 1) / 2 pairs are compared four pixels per 32-bit word (<= 28 byte compares per pixel), one or two 16-byte stores.  Integers
// only; the only atomics are the integer counts of `hist` (per-lane counters, wave sums, one add per bucket and workgroup): two launches
// give the same bits.
#include "common.h"

namespace {

constexpr int MAX_SETS = 8;
constexpr int VOTE_THREADS = 256;
constexpr int VOTE_MAX_BLOCKS = 2048;                                  // 256 CUs x 8 workgroups: beyond it a workgroup strides on

// 0x01 in every byte in which a and b are equal
__device__ __forceinline__ uint32_t equal_bytes(const uint32_t a, const uint32_t b) {
  const uint32_t x = a ^ b;
  return (~(x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;
}

// 0xff in every byte in which a > b; a, b < 0x80 in every byte
__device__ __forceinline__ uint32_t greater_bytes(const uint32_t a, const uint32_t b) {
  return ((((a | 0x80808080u) - b - 0x01010101u) & 0x80808080u) >> 7) * 0xffu;
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

// A lane walks the chunks of 16 pixels c = its index, + the grid's lanes, ...; `vec`: every plane and both outputs are 16-byte aligned,
// so a whole chunk moves as one vector per plane (the last, partial chunk and every chunk of an unaligned call go byte by byte).
// ge[v - 1] counts the lane's pixels whose winner has >= v votes (ge[0]: all of them); hist[v] is the difference of two neighbours.
template <int K>
__global__ __launch_bounds__(VOTE_THREADS) void idmap_vote_kernel(const uint8_t* __restrict__ maps, const long set_stride, const long pixels,
                                                                  const int vec, uint8_t* __restrict__ voted, uint8_t* __restrict__ votes,
                                                                  unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long s_ge[MAX_SETS + 1];
  const int tid = threadIdx.x;
  const long chunks = (pixels + 15) / 16;
  unsigned ge[K];
#pragma unroll
  for (int v = 0; v < K; ++v) ge[v] = 0;
  for (long c = (long)blockIdx.x * VOTE_THREADS + tid; c < chunks; c += (long)gridDim.x * VOTE_THREADS) {
    const long p0 = c * 16;
    const int valid = pixels - p0 < 16 ? (int)(pixels - p0) : 16;
    const bool v16 = vec && valid == 16;
    uint32_t m[K][4];
#pragma unroll
    for (int k = 0; k < K; ++k) load16(maps + k * set_stride + p0, valid, v16, m[k]);
    uint32_t label[4], count[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t cnt[K];
#pragma unroll
      for (int k = 0; k < K; ++k) cnt[k] = 0x01010101u;                // a set agrees with itself
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int i = k + 1; i < K; ++i) {
          const uint32_t e = equal_bytes(m[k][j], m[i][j]);
          cnt[k] += e;
          cnt[i] += e;
        }
      uint32_t lab = m[0][j], best = cnt[0];
#pragma unroll
      for (int k = 1; k < K; ++k) {                                    // strictly more votes: the earlier set keeps a tie
        const uint32_t g = greater_bytes(cnt[k], best);
        lab = (lab & ~g) | (m[k][j] & g);
        best = (best & ~g) | (cnt[k] & g);
      }
      label[j] = lab;
      count[j] = best;
      if (hist != nullptr) {
        const int r = valid - 4 * j;                                   // the word's pixels that exist
        const uint32_t there = r >= 4 ? 0x80808080u : r <= 0 ? 0u : (0x80808080u & ((1u << (8 * r)) - 1u));
#pragma unroll
        for (int v = 1; v < K; ++v)
          ge[v] += __popc(((best | 0x80808080u) - (uint32_t)(v + 1) * 0x01010101u) & there);
      }
    }
    ge[0] += valid;
    store16(voted + p0, valid, v16, label);
    if (votes != nullptr) store16(votes + p0, valid, v16, count);
  }
  if (hist == nullptr) return;
  if (tid <= MAX_SETS) s_ge[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int v = 0; v < K; ++v) {
    unsigned n = ge[v];
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((tid & 63) == 0 && n) atomicAdd(&s_ge[v], (unsigned long long)n);
  }
  __syncthreads();
  if (tid < K) {
    const unsigned long long n = s_ge[tid] - s_ge[tid + 1];           // (s_ge[K] stays 0)
    if (n) atomicAdd(&hist[tid + 1], n);
  }
}

bool ranges_overlap(const uint8_t* a, const long na, const uint8_t* b, const long nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

template <int K>
void launch_vote(const uint8_t* maps, long set_stride, long pixels, int vec, uint8_t* voted, uint8_t* votes, int64_t* hist, void* stream) {
  const long chunks = (pixels + 15) / 16;
  const long blocks = (chunks + VOTE_THREADS - 1) / VOTE_THREADS;
  hipLaunchKernelGGL(idmap_vote_kernel<K>, dim3((unsigned)(blocks < VOTE_MAX_BLOCKS ? blocks : VOTE_MAX_BLOCKS)), dim3(VOTE_THREADS), 0,
                     static_cast<hipStream_t>(stream), maps, set_stride, pixels, vec, voted, votes,
                     reinterpret_cast<unsigned long long*>(hist));
}

}  // namespace

extern "C" int premvos_idmap_vote_u8(const uint8_t* maps, int32_t K, int64_t set_stride, int64_t pixels, uint8_t* voted, uint8_t* votes,
                                     int64_t* hist, void* stream) {
  PV_REQUIRE(maps && voted, "idmap_vote: null pointer");
  PV_REQUIRE(K >= 1 && K <= MAX_SETS, "idmap_vote: 1 to %d sets (got %d)", MAX_SETS, K);
  PV_REQUIRE(pixels >= 0, "idmap_vote: negative pixels (%ld)", (long)pixels);
  PV_REQUIRE(K == 1 || set_stride >= pixels, "idmap_vote: the sets' maps overlap (stride %ld, %ld pixels)", (long)set_stride, (long)pixels);
  PV_REQUIRE(pixels < (1L << 48) && (K == 1 || set_stride < (1L << 48)), "idmap_vote: bad dims");
  if (pixels == 0) return PREMVOS_OK;
  if (K == 1) set_stride = 0;                                          // (never added to the pointer)
  const long span = (long)(K - 1) * set_stride + pixels;
  PV_REQUIRE(!ranges_overlap(voted, pixels, maps, span), "idmap_vote: voted overlaps the maps");
  PV_REQUIRE(!votes || !ranges_overlap(votes, pixels, maps, span), "idmap_vote: votes overlaps the maps");
  PV_REQUIRE(!votes || !ranges_overlap(votes, pixels, voted, pixels), "idmap_vote: votes overlaps voted");
  const int vec = premvos::aligned16(maps) && set_stride % 16 == 0 && premvos::aligned16(voted) && (!votes || premvos::aligned16(votes));
  switch (K) {
    case 1: launch_vote<1>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    case 2: launch_vote<2>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    case 3: launch_vote<3>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    case 4: launch_vote<4>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    case 5: launch_vote<5>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    case 6: launch_vote<6>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    case 7: launch_vote<7>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
    default: launch_vote<8>(maps, set_stride, pixels, vec, voted, votes, hist, stream); break;
  }
  return premvos::check_launch("idmap_vote");
}
