// The DAVIS-2017 measures' pixel work on the GPU (tools/davis_eval.py:25-71 db_eval_iou, seg2bmap, db_eval_boundary): for every frame
// and object the six integers J and F are made of.  All integer: the disk is dx*dx + dy*dy <= r*r, the sums are integer adds (one
// vector atomic per wave and count), so two launches give the same bits and J and F follow from the counts alone, on the host.
//
// One workgroup = one 32 x 64 tile of one frame.  The ids of both maps over the tile and its halo (r above / left, r + 1 below /
// right: a boundary bit needs the pixel's east, south and south-east neighbours) are staged in LDS once.  Per object: a wave turns 64
// pixels of a halo row into one 64-bit word of boundary bits per mask (a ballot), then a lane that owns a boundary pixel looks for a
// set bit of the OTHER mask in the 2r + 1 row windows [x - wtab[|dy|], x + wtab[|dy|]] around it, nearest rows first.  The host's
// dense dilation by a (2r + 1)^2 disk becomes a search around perimeter pixels only.  An id that occurs in neither map's staged
// region costs the tile nothing.
#include "common.h"

namespace {

constexpr int TILE_H = 32, TILE_W = 64, MAX_RADIUS = 48, THREADS = 256;

struct DavisLds {
  int ids_h, ids_w, ids_stride;      // staged ids: TILE + 2r + 1 each way, rows padded to 4 bytes
  int bits_h, bits_nw;               // boundary words: TILE_H + 2r rows of bits_nw 64-bit words (TILE_W + 2r columns)
  size_t off_g, off_bits, off_tab, bytes;
};

__host__ __device__ inline DavisLds davis_lds(const int r) {
  DavisLds L;
  L.ids_h = TILE_H + 2 * r + 1;
  L.ids_w = TILE_W + 2 * r + 1;
  L.ids_stride = (L.ids_w + 3) & ~3;
  L.bits_h = TILE_H + 2 * r;
  L.bits_nw = (TILE_W + 2 * r + 63) / 64;
  const size_t ids = ((size_t)L.ids_h * L.ids_stride + 15) & ~(size_t)15;      // every carve offset a multiple of 16 bytes
  L.off_g = ids;
  L.off_bits = 2 * ids;
  L.off_tab = L.off_bits + 2 * (size_t)L.bits_h * L.bits_nw * 8;
  L.bytes = L.off_tab + (MAX_RADIUS + 1) * 4 + 256 * 4 + 256;
  return L;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// any bit of row words `row` in the columns [a, b] (0 <= a <= b < 64 * nw)?
__device__ __forceinline__ bool any_bit(const unsigned long long* row, const int a, const int b) {
  const int wa = a >> 6, wb = b >> 6;
  const unsigned long long lo = ~0ull << (a & 63), hi = ~0ull >> (63 - (b & 63));
  if (wa == wb) return (row[wa] & lo & hi) != 0;
  if (row[wa] & lo) return true;
  for (int k = wa + 1; k < wb; ++k)
    if (row[k]) return true;
  return (row[wb] & hi) != 0;
}

// does the disk around tile pixel (ty, tx) hold a bit of `bits`?  Rows nearest first: where the masks agree the first row answers.
__device__ __forceinline__ bool disk_hit(const unsigned long long* bits, const int nw, const int* wtab, const int r, const int ty,
                                         const int tx) {
  const int cy = ty + r, cx = tx + r;
  if (any_bit(bits + (long)cy * nw, cx - r, cx + r)) return true;
  for (int dy = 1; dy <= r; ++dy) {
    const int wd = wtab[dy];
    if (any_bit(bits + (long)(cy - dy) * nw, cx - wd, cx + wd) || any_bit(bits + (long)(cy + dy) * nw, cx - wd, cx + wd)) return true;
  }
  return false;
}

__global__ __launch_bounds__(THREADS) void davis_counts_kernel(const uint8_t* __restrict__ result, const uint8_t* __restrict__ gt,
                                                               const int h, const int w, const int tiles_x, const int tiles_y,
                                                               const int* __restrict__ ids, const int T, const int r,
                                                               unsigned long long* __restrict__ counts, uint8_t* __restrict__ maps) {
  extern __shared__ __align__(16) unsigned char lds[];
  const DavisLds L = davis_lds(r);
  uint8_t* s_r = lds;
  uint8_t* s_g = lds + L.off_g;
  unsigned long long* s_br = reinterpret_cast<unsigned long long*>(lds + L.off_bits);
  unsigned long long* s_bg = s_br + (long)L.bits_h * L.bits_nw;
  int* s_wtab = reinterpret_cast<int*>(lds + L.off_tab);
  int* s_ids = s_wtab + MAX_RADIUS + 1;
  uint8_t* s_present = reinterpret_cast<uint8_t*>(s_ids + 256);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long per = (long)tiles_x * tiles_y;
  const int img = (int)(blockIdx.x / per);
  const int tile = (int)(blockIdx.x - (long)img * per);
  const int y0 = (tile / tiles_x) * TILE_H, x0 = (tile % tiles_x) * TILE_W;
  const long hw = (long)h * w;
  const uint8_t* res = result + (long)img * hw;
  const uint8_t* ann = gt + (long)img * hw;

  s_present[tid] = 0;
  if (tid < T) s_ids[tid] = ids[tid];
  if (tid <= r) {                                        // widest dx with dx*dx + dy*dy <= r*r, in integers
    int dx = 0;
    while ((dx + 1) * (dx + 1) + tid * tid <= r * r) ++dx;
    s_wtab[tid] = dx;
  }
  __syncthreads();
  // ids over rows y0 - r .. y0 + TILE_H + r, columns x0 - r .. x0 + TILE_W + r; outside the image: 0 (never read as a mask pixel)
  for (int i = tid; i < L.ids_h * L.ids_w; i += THREADS) {
    const int ry = i / L.ids_w, rx = i - ry * L.ids_w;
    const int gy = y0 - r + ry, gx = x0 - r + rx;
    uint8_t a = 0, b = 0;
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
      a = res[(long)gy * w + gx];
      b = ann[(long)gy * w + gx];
      s_present[a] = 1;
      s_present[b] = 1;
    }
    s_r[ry * L.ids_stride + rx] = a;
    s_g[ry * L.ids_stride + rx] = b;
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int id = s_ids[t];
    if (id < 0 || id > 255 || !s_present[id]) continue;             // (uniform over the workgroup)
    // boundary words: wave `wave` takes (row, word) pairs; lane = column within the word
    const int pairs = L.bits_h * L.bits_nw;
    for (int p = wave; p < pairs; p += THREADS / 64) {
      const int ry = p / L.bits_nw, k = p - ry * L.bits_nw;
      const int rx = k * 64 + lane;
      const int gy = y0 - r + ry, gx = x0 - r + rx;
      bool br = false, bg = false;
      if (rx < TILE_W + 2 * r && gy >= 0 && gy < h && gx >= 0 && gx < w) {
        const bool east = gx + 1 < w, south = gy + 1 < h;          // a neighbour outside the image compares as the pixel itself
        const uint8_t* pr = s_r + ry * L.ids_stride + rx;
        const uint8_t* pg = s_g + ry * L.ids_stride + rx;
        const bool mr = pr[0] == id, mg = pg[0] == id;
        if (east) {
          br |= (pr[1] == id) != mr;
          bg |= (pg[1] == id) != mg;
        }
        if (south) {
          br |= (pr[L.ids_stride] == id) != mr;
          bg |= (pg[L.ids_stride] == id) != mg;
        }
        if (east && south) {
          br |= (pr[L.ids_stride + 1] == id) != mr;
          bg |= (pg[L.ids_stride + 1] == id) != mg;
        }
      }
      const unsigned long long wr = __ballot(br), wg = __ballot(bg);
      if (lane == 0) {
        s_br[p] = wr;
        s_bg[p] = wg;
      }
    }
    __syncthreads();
    int c[6] = {0, 0, 0, 0, 0, 0};
    uint8_t* mp = maps ? maps + ((long)img * T + t) * 4 * hw : nullptr;
    for (int q = tid; q < TILE_H * TILE_W; q += THREADS) {
      const int ty = q >> 6, tx = q & 63;
      const int gy = y0 + ty, gx = x0 + tx;
      if (gy >= h || gx >= w) continue;
      const bool mr = s_r[(ty + r) * L.ids_stride + tx + r] == id, mg = s_g[(ty + r) * L.ids_stride + tx + r] == id;
      c[0] += mr && mg;
      c[1] += mr || mg;
      const int word = (ty + r) * L.bits_nw + ((tx + r) >> 6), bit = (tx + r) & 63;
      const bool br = (s_br[word] >> bit) & 1, bg = (s_bg[word] >> bit) & 1;
      if (!br && !bg) continue;
      const bool hr = br && disk_hit(s_bg, L.bits_nw, s_wtab, r, ty, tx);
      const bool hg = bg && disk_hit(s_br, L.bits_nw, s_wtab, r, ty, tx);
      c[2] += br;
      c[3] += bg;
      c[4] += hr;
      c[5] += hg;
      if (mp) {
        const long o = (long)gy * w + gx;
        if (br) mp[o] = 1;
        if (bg) mp[hw + o] = 1;
        if (hr) mp[2 * hw + o] = 1;
        if (hg) mp[3 * hw + o] = 1;
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int s = wave_sum(c[k]);
      if (lane == 0 && s) atomicAdd(&counts[((long)img * T + t) * 6 + k], (unsigned long long)s);
    }
    __syncthreads();                                                 // the words are rebuilt for the next object
  }
}

}  // namespace

extern "C" int premvos_davis_counts_u8(const uint8_t* result, const uint8_t* gt, int32_t n, int32_t h, int32_t w, const int32_t* ids,
                                       int32_t T, int32_t radius, int64_t* counts, uint8_t* maps, void* stream) {
  PV_REQUIRE(n >= 0 && T >= 0, "davis_counts: negative count (n %d, T %d)", n, T);
  PV_REQUIRE(h > 0 && w > 0, "davis_counts: bad dims (h %d, w %d)", h, w);
  PV_REQUIRE(T <= 255, "davis_counts: at most 255 objects (got %d)", T);
  PV_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, "davis_counts: radius must be in 1 .. %d (got %d)", MAX_RADIUS, radius);
  if (n == 0 || T == 0) return PREMVOS_OK;
  PV_REQUIRE(result && gt && ids && counts, "davis_counts: null pointer");
  const int tiles_x = premvos::cdiv(w, TILE_W), tiles_y = premvos::cdiv(h, TILE_H);
  const long blocks = (long)tiles_x * tiles_y * n;
  PV_REQUIRE(blocks < (1L << 31), "davis_counts: too many tiles (%ld)", blocks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t hw = (size_t)h * w;
  if (hipMemsetAsync(counts, 0, sizeof(int64_t) * 6 * (size_t)n * T, s) != hipSuccess ||
      (maps && hipMemsetAsync(maps, 0, (size_t)n * T * 4 * hw, s) != hipSuccess))
    return premvos::fail(PREMVOS_ELAUNCH, "davis_counts: memset failed");
  const DavisLds L = davis_lds(radius);
  hipLaunchKernelGGL(davis_counts_kernel, dim3((unsigned)blocks), dim3(THREADS), L.bytes, s, result, gt, h, w, tiles_x, tiles_y, ids, T,
                     radius, reinterpret_cast<unsigned long long*>(counts), maps);
  return premvos::check_launch("davis_counts");
}
