// The ingest side of the pre-warp merge (MergeTrack/oldmerge.py; premvos_amd/prewarp.py VideoIngest): a chunk's byte masks, grouped
// by frame, become the two bit rows the pool keeps of every mask -- the mask itself and the mask warped to the next frame by its
// frame's flow (merge_functions.py:209-217 warp_flow, then "== 1") -- in ONE launch, so the byte masks never outlive their chunk.
//   * premvos_mask_warp_pack_bits_u8     = premvos_mask_pack_bits_u8 of the masks + of premvos_mask_warp_seats_u8(binarize) of them
// The tap arithmetic is mask_warp_taps.h's, the one merge_ops.hip's byte warps run.  Integer work behind the taps, vector stores only.
#include "common.h"
#include "mask_warp_taps.h"

namespace {

constexpr int WG_PIXELS = 1024;      // pixels of a workgroup: 256 lanes x 4, i.e. 16 words = 128 contiguous bytes of every row
constexpr int WG_WORDS = WG_PIXELS / 64;
constexpr int MASK_GROUP = 8;        // masks whose words are collected in LDS before they are stored: 8 x 2 x 16 words = one per lane

// grid (pixel blocks, V).  Frame v owns the masks [frame_first[v], frame_first[v + 1]) and moves by flows[flow_of_frame[v]] (< 0: its
// forward rows are zero).  Lane l of wave q holds the pixels base + 256 j + 64 q + l, j < 4: a ballot over a wave is the word
// 4 j + q of the workgroup's 16.  A pixel's taps are found once and serve every mask of the frame; the words of 8 masks go through
// LDS, so that 16 consecutive lanes store 128 contiguous bytes of one row.
__global__ __launch_bounds__(256) void mask_warp_pack_bits_kernel(const uint8_t* __restrict__ masks, const int n, const int h, const int w,
                                                                  const int* __restrict__ frame_first, const int* __restrict__ flow_of_frame,
                                                                  const float* __restrict__ flows, const int nflows,
                                                                  unsigned long long* __restrict__ cur_bits,
                                                                  unsigned long long* __restrict__ fwd_bits, const long words) {
  __shared__ unsigned long long s_w[MASK_GROUP][2][WG_WORDS];
  const int v = blockIdx.y;
  int i0 = frame_first[v], i1 = frame_first[v + 1];
  i0 = i0 < 0 ? 0 : i0;              // (the host table was checked; the device copy is held to the arrays' bounds all the same)
  i1 = i1 > n ? n : i1;
  if (i0 >= i1) return;              // a frame without masks: the whole workgroup, before any barrier
  int f = flow_of_frame[v];
  if (f >= nflows) f = -1;
  const long hw = (long)h * w;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long base = (long)blockIdx.x * WG_PIXELS;
  premvos::MaskWarpTaps taps[4];
  if (f >= 0) {
    const float* flow = flows + (long)f * hw * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long p = base + 256 * j + tid;
      if (p < hw) taps[j] = premvos::mask_warp_taps(flow, p, h, w);
    }
  }
  for (int g0 = i0; g0 < i1; g0 += MASK_GROUP) {
    const int ng = (i1 - g0) < MASK_GROUP ? (i1 - g0) : MASK_GROUP;
    for (int g = 0; g < ng; ++g) {
      const uint8_t* m = masks + (long)(g0 + g) * hw;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long p = base + 256 * j + tid;
        bool cur = false, fwd = false;
        if (p < hw) {
          cur = m[p] != 0;
          if (f >= 0) fwd = premvos::mask_warp_value(m, taps[j], w) == 1;
        }
        const unsigned long long bc = __ballot(cur), bf = __ballot(fwd);      // (every lane of the wave: the branch above has ended)
        if (lane == 0) {
          s_w[g][0][4 * j + wave] = bc;
          s_w[g][1][4 * j + wave] = bf;
        }
      }
    }
    __syncthreads();
    const int g = tid >> 5, which = (tid >> 4) & 1, k = tid & 15;
    const long word = (long)blockIdx.x * WG_WORDS + k;
    if (g < ng && word < words) (which ? fwd_bits : cur_bits)[(long)(g0 + g) * words + word] = s_w[g][which][k];
    __syncthreads();
  }
}

bool overlaps(const void* a, const long na, const void* b, const long nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int premvos_mask_warp_pack_bits_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, const int32_t* frame_first,
                                              const int32_t* frame_first_dev, const int32_t* flow_of_frame, const int32_t* flow_of_frame_dev,
                                              const float* flows, int32_t nflows, int32_t V, uint8_t* cur_bits, uint8_t* fwd_bits,
                                              int64_t row_bytes, void* stream) {
  PV_REQUIRE(masks && frame_first && frame_first_dev && flow_of_frame && flow_of_frame_dev && cur_bits && fwd_bits && (flows || nflows == 0),
             "mask_warp_pack_bits: null pointer");
  PV_REQUIRE(n > 0 && h > 0 && w > 0 && (long)h * w < (1L << 31) && nflows >= 0, "mask_warp_pack_bits: bad dims (n %d, h %d, w %d, nflows %d)", n,
             h, w, nflows);
  PV_REQUIRE(V >= 1 && V <= 4096, "mask_warp_pack_bits: 1 to 4096 frames (got %d)", V);
  const long hw = (long)h * w, words = (hw + 63) / 64;
  PV_REQUIRE(row_bytes == words * 8, "mask_warp_pack_bits: row_bytes %ld, but %ld pixels are %ld whole 64-bit words = %ld bytes", (long)row_bytes,
             hw, words, words * 8);
  PV_REQUIRE(((reinterpret_cast<uintptr_t>(cur_bits) | reinterpret_cast<uintptr_t>(fwd_bits)) & 7u) == 0,
             "mask_warp_pack_bits: the bit rows must be 8-byte aligned");
  PV_REQUIRE(frame_first[0] == 0 && frame_first[V] == n, "mask_warp_pack_bits: frame_first runs from %d to %d, not from 0 to %d", frame_first[0],
             frame_first[V], n);
  for (int v = 0; v < V; ++v) {
    PV_REQUIRE(frame_first[v + 1] >= frame_first[v], "mask_warp_pack_bits: frame_first descends at frame %d", v);
    PV_REQUIRE(flow_of_frame[v] >= -1 && flow_of_frame[v] < nflows, "mask_warp_pack_bits: flow_of_frame[%d] = %d is outside [-1, %d)", v,
               flow_of_frame[v], nflows);
  }
  const long mask_bytes = (long)n * hw, bit_bytes = (long)n * row_bytes;
  PV_REQUIRE(!overlaps(masks, mask_bytes, cur_bits, bit_bytes) && !overlaps(masks, mask_bytes, fwd_bits, bit_bytes),
             "mask_warp_pack_bits: the masks overlap an output");
  PV_REQUIRE(!overlaps(cur_bits, bit_bytes, fwd_bits, bit_bytes), "mask_warp_pack_bits: the two outputs overlap each other");
  hipLaunchKernelGGL(mask_warp_pack_bits_kernel, dim3((unsigned)((hw + WG_PIXELS - 1) / WG_PIXELS), (unsigned)V), dim3(256), 0,
                     static_cast<hipStream_t>(stream), masks, n, h, w, frame_first_dev, flow_of_frame_dev, flows, nflows,
                     reinterpret_cast<unsigned long long*>(cur_bits), reinterpret_cast<unsigned long long*>(fwd_bits), words);
  return premvos::check_launch("mask_warp_pack_bits");
}
