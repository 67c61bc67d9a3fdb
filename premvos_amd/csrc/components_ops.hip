// Per-object largest-component clean-up of id maps: ReID_net/scripts/postproc/postproc.py:41-63 (postproc_posteriors_connected_components:
// dilate the mask with a 100 x 100 box, label the 8-connected components of the DILATED mask, count the original pixels in each, keep the
// largest, a tie to the lowest component number), run per object id k >= 1 on res = (M == k).  Integers only: every result is exact and
// does not depend on any execution order.
//
//   dilate        dil(y, x) = 1 iff some pixel of res lies in rows y - (D-1)/2 .. y + D/2 and columns x - (D-1)/2 .. x + D/2 (scipy's
//                 grey_dilation with size (D, D); its reflecting border adds nothing).  A workgroup owns 64 x 64 output pixels of one plane:
//                 a wave turns one source row into 64 row hits (ballots of the row's 64 + D - 1 columns, a masked test per lane), kept as
//                 bytes in LDS; then a thread walks 16 rows of one column with a sliding count of the row hits in its D rows.
//   label         union-find, four launches, so that kernel boundaries do the publishing:
//                   1. a 16 x 32 tile is labelled in LDS (lock-free unions with the W, NW, N, NE neighbours, then every pixel finds its
//                      root) and written as GLOBAL linear indices: a pixel points at the smallest index of its component inside the tile;
//                   2. the pixels on a tile's top row and left / right columns unite with their W, NW, N, NE neighbours in OTHER tiles.
//                      Every read and write of the label array in this launch is an agent-scope atomic (relaxed load, atomicMin);
//                   3. the tile roots that launch 2 pointed into another tile find their root, 4. every other pixel finds its own over
//                      them (agent-scope atomic loads and one atomic store: a thread may read a pixel before or after its owner
//                      flattened it, both values are parents inside the same tree).
//                 A parent's index is never above its child's, unions only lower a parent, so the root of a component is its smallest
//                 linear index: labels[p] = that index, -1 on background.  No thread waits for another's write.
//   keep_largest  count the pixels of res per root (integer adds), per plane the largest count and on a tie the smallest root (one 64-bit
//                 maximum of count << 32 | ~root), repaint.
#include "common.h"
#include "../../include/premvos_post_hip.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_MAX_PIXELS = 1 << 26;                                       // h * w: a linear index and its count stay an int32
constexpr int CC_MIN_L = 2, CC_MAX_L = 256, CC_MIN_D = 1, CC_MAX_D = 255;
constexpr int CC_DIL_T = 64, CC_DIL_ROWS = CC_DIL_T + CC_MAX_D - 1, CC_DIL_CHUNKS = (CC_DIL_T + CC_MAX_D - 1 + 63) / 64;      // 318 rows, 5 ballots
constexpr int CC_TILE_H = 16, CC_TILE_W = 32, CC_TILE = CC_TILE_H * CC_TILE_W;
constexpr int CC_BORDER = 64;                                                // a tile's border pixels (32 + 15 + 15 = 62), one wave
constexpr int CC_KEEP_THREADS = 1024;
constexpr unsigned CC_MAX_GRID_Y = 65535;

// ------------------------------------------------------------------------------------------------------------------------ dilate
// grid (column strips of 64, row bands of 64, planes up to 65535: a workgroup walks the planes it owns)
__global__ __launch_bounds__(CC_THREADS) void cc_dilate_kernel(const uint8_t* __restrict__ idmaps, const int h, const int w, const int L,
                                                               const int D, const long planes, uint8_t* __restrict__ dil) {
  __shared__ uint8_t hit[CC_DIL_ROWS * CC_DIL_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = (D - 1) / 2, hi = D / 2;                                    // a pixel sees rows y - lo .. y + hi
  const int x0 = blockIdx.x * CC_DIL_T, y0 = blockIdx.y * CC_DIL_T;
  const int sy_lo = max(0, y0 - lo), sy_hi = min(h - 1, y0 + CC_DIL_T - 1 + hi), rows = sy_hi - sy_lo + 1;      // <= CC_DIL_ROWS
  const long HW = (long)h * w;
  for (long plane = blockIdx.z; plane < planes; plane += gridDim.z) {
    const long f = plane / (L - 1);
    const int k = 1 + (int)(plane - f * (L - 1));
    const uint8_t* src = idmaps + f * HW;
    __syncthreads();                                                         // the plane before this one has been read
    for (int r = wave; r < rows; r += CC_THREADS / 64) {
      const uint8_t* row = src + (long)(sy_lo + r) * w;
      // bit (64 c + j) of the row's string = column x0 - lo + 64 c + j holds k; the lane's output column sees bits lane .. lane + D - 1
      bool any = false;
#pragma unroll
      for (int c = 0; c < CC_DIL_CHUNKS; ++c) {
        if (64 * c < CC_DIL_T + D - 1) {                                     // (the same for every lane)
          const int col = x0 - lo + 64 * c + lane;
          const bool set = col >= 0 && col < w && row[col] == k;
          const unsigned long long m = __ballot(set);
          const int a = max(lane, 64 * c) - 64 * c, b = min(lane + D, 64 * c + 64) - 64 * c;      // the window's part of this word
          if (b > a) {
            const unsigned long long upto_b = b >= 64 ? ~0ull : ((1ull << b) - 1ull), upto_a = (1ull << a) - 1ull;      // (a <= 63)
            any = any || (m & upto_b & ~upto_a) != 0ull;
          }
        }
      }
      hit[r * CC_DIL_T + lane] = any ? 1 : 0;
    }
    __syncthreads();
    const int x = x0 + lane;
    const int ya = y0 + wave * (CC_DIL_T / 4), yb = min(h, ya + CC_DIL_T / 4);      // the thread's rows of column x
    if (x < w && ya < yb) {
      uint8_t* out = dil + plane * HW + x;
      int count = 0;
      for (int sy = max(sy_lo, ya - lo); sy <= min(sy_hi, ya + hi); ++sy) count += hit[(sy - sy_lo) * CC_DIL_T + lane];
      for (int y = ya; y < yb; ++y) {
        out[(long)y * w] = count > 0 ? 1 : 0;
        if (y - lo >= sy_lo) count -= hit[(y - lo - sy_lo) * CC_DIL_T + lane];              // (y - lo <= sy_hi: it is a row of the frame)
        if (y + 1 + hi <= sy_hi) count += hit[(y + 1 + hi - sy_lo) * CC_DIL_T + lane];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------- label
// the root of i in a forest in LDS (a parent is never above its child)
__device__ __forceinline__ int find_lds(volatile int* t, int i) {
  // strictly decreasing: i (t[i] <= i always, the loop goes on only while t[i] < i)
  for (int p = t[i]; p != i; p = t[i]) i = p;
  return i;
}

__device__ __forceinline__ void unite_lds(int* t, int a, int b) {
  // strictly decreasing: max(a, b).  The larger root is pointed at the smaller with atomicMin; if it was no root any more (old != a), its
  // earlier parent old < a takes its place, the other side stays.  Labels only go down.
  for (;;) {
    a = find_lds(t, a);
    b = find_lds(t, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(&t[a], b);
    if (old == a) return;
    a = old;
  }
}

__device__ __forceinline__ int load_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i in the forest in HBM, through agent-scope atomic loads alone
__device__ __forceinline__ int find_agent(const int* lab, int i) {
  // strictly decreasing: i (lab[i] <= i always, the loop goes on only while lab[i] < i)
  for (int p = load_agent(lab + i); p != i; p = load_agent(lab + i)) i = p;
  return i;
}

__device__ __forceinline__ void unite_agent(int* lab, int a, int b) {
  // strictly decreasing: max(a, b), as in unite_lds; labels only go down (atomicMin)
  for (;;) {
    a = find_agent(lab, a);
    b = find_agent(lab, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(&lab[a], b);                                   // (agent scope)
    if (old == a) return;
    a = old;
  }
}

// launch 1: grid (tiles along x, tiles along y, planes up to 65535)
__global__ __launch_bounds__(CC_THREADS) void cc_label_tile_kernel(const uint8_t* __restrict__ masks, const int h, const int w, const long planes,
                                                                   int* __restrict__ labels) {
  __shared__ int t[CC_TILE];
  const int x0 = blockIdx.x * CC_TILE_W, y0 = blockIdx.y * CC_TILE_H;
  const long HW = (long)h * w;
  for (long plane = blockIdx.z; plane < planes; plane += gridDim.z) {
    const uint8_t* m = masks + plane * HW;
    __syncthreads();                                                         // the plane before this one has been written out
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
      const int y = y0 + i / CC_TILE_W, x = x0 + i % CC_TILE_W;
      t[i] = (y < h && x < w && m[(long)y * w + x] != 0) ? i : -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC_TILE; i += CC_THREADS) {
      if (t[i] < 0) continue;
      const int ty = i / CC_TILE_W, tx = i % CC_TILE_W;
      if (tx > 0 && t[i - 1] >= 0) unite_lds(t, i, i - 1);
      if (ty > 0) {
        if (t[i - CC_TILE_W] >= 0) unite_lds(t, i, i - CC_TILE_W);
        if (tx > 0 && t[i - CC_TILE_W - 1] >= 0) unite_lds(t, i, i - CC_TILE_W - 1);
        if (tx < CC_TILE_W - 1 && t[i - CC_TILE_W + 1] >= 0) unite_lds(t, i, i - CC_TILE_W + 1);
      }
    }
    __syncthreads();
    int* out = labels + plane * HW;
    int root[CC_TILE / CC_THREADS];
#pragma unroll
    for (int j = 0; j < CC_TILE / CC_THREADS; ++j) {
      const int i = threadIdx.x + j * CC_THREADS;
      root[j] = t[i] < 0 ? -1 : find_lds(t, i);
    }
#pragma unroll
    for (int j = 0; j < CC_TILE / CC_THREADS; ++j) {
      const int i = threadIdx.x + j * CC_THREADS;
      const int y = y0 + i / CC_TILE_W, x = x0 + i % CC_TILE_W;
      if (y < h && x < w) out[(long)y * w + x] = root[j] < 0 ? -1 : (y0 + root[j] / CC_TILE_W) * w + x0 + root[j] % CC_TILE_W;
    }
  }
}

// launch 2: a wave per tile (lane -> one of the tile's 62 border pixels), four tiles per workgroup; grid (tiles / 4, planes up to 65535)
__global__ __launch_bounds__(CC_THREADS) void cc_label_merge_kernel(const int h, const int w, const int tiles_x, const int tiles,
                                                                    const long planes, int* __restrict__ labels) {
  const int tile = blockIdx.x * (CC_THREADS / CC_BORDER) + threadIdx.x / CC_BORDER, j = threadIdx.x % CC_BORDER;
  if (tile >= tiles || j >= CC_TILE_W + 2 * (CC_TILE_H - 1)) return;
  // j < 32: the top row; then the left column's rows 1 .. 15, then the right column's
  const int ty = j < CC_TILE_W ? 0 : 1 + (j - CC_TILE_W) % (CC_TILE_H - 1);
  const int tx = j < CC_TILE_W ? j : (j - CC_TILE_W < CC_TILE_H - 1 ? 0 : CC_TILE_W - 1);
  const int y = (tile / tiles_x) * CC_TILE_H + ty, x = (tile % tiles_x) * CC_TILE_W + tx;
  if (y >= h || x >= w) return;
  const int p = y * w + x;
  const long HW = (long)h * w;
  for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    int* lab = labels + plane * HW;
    if (load_agent(lab + p) < 0) continue;
    // the W, NW, N, NE neighbours that lie in another tile
    if (tx == 0 && x > 0 && load_agent(lab + p - 1) >= 0) unite_agent(lab, p, p - 1);
    if (y > 0) {
      if (ty == 0 && load_agent(lab + p - w) >= 0) unite_agent(lab, p, p - w);
      if ((ty == 0 || tx == 0) && x > 0 && load_agent(lab + p - w - 1) >= 0) unite_agent(lab, p, p - w - 1);
      if ((ty == 0 || tx == CC_TILE_W - 1) && x < w - 1 && load_agent(lab + p - w + 1) >= 0) unite_agent(lab, p, p - w + 1);
    }
  }
}

__device__ __forceinline__ bool same_tile(const int a, const int b, const int w) {
  return (a / w) / CC_TILE_H == (b / w) / CC_TILE_H && (a % w) / CC_TILE_W == (b % w) / CC_TILE_W;
}

// launches 3 and 4: grid (blocks over a plane's pixels, planes up to 65535).  Launch 1 left every pixel pointing at a root of its own
// tile, and launch 2 changed the labels of such tile roots alone.  FAR = true: the pixels whose parent lies in another tile (tile roots
// that were united with another tile's component; a few per tile) walk to their root.  FAR = false, after it: every other pixel walks
// over parents inside its tile (tile roots united with one another) to one that is a root or was flattened by the launch before.
template <bool FAR>
__global__ __launch_bounds__(CC_THREADS) void cc_label_flatten_kernel(const int HW, const int w, const long planes, int* __restrict__ labels) {
  for (long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
    int* lab = labels + plane * HW;
    for (int p = blockIdx.x * CC_THREADS + threadIdx.x; p < HW; p += gridDim.x * CC_THREADS) {
      const int parent = load_agent(lab + p);
      if (parent < 0 || parent == p || same_tile(parent, p, w) == FAR) continue;
      const int root = find_agent(lab, parent);
      if (root != parent) __hip_atomic_store(lab + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ keep_largest
// grid (blocks over a frame's pixels, frames): counts[(frame, k), root of the pixel] += 1 for every pixel with an id 1 <= k < L.  The pixels
// of a wave mostly share one root (an object's body): per distinct (k, root) in the wave ONE integer add of their number.
__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const uint8_t* __restrict__ idmaps, const int* __restrict__ labels, const int HW,
                                                              const int L, int* __restrict__ counts) {
  const long f = blockIdx.y;
  for (int p0 = blockIdx.x * CC_THREADS; p0 < HW; p0 += gridDim.x * CC_THREADS) {      // (the whole wave stays in the loop: the ballots)
    const int p = p0 + threadIdx.x;
    int k = 0, root = -1;
    if (p < HW) {
      k = idmaps[f * HW + p];
      if (k >= 1 && k < L) root = labels[(f * (L - 1) + (k - 1)) * HW + p];
    }
    const bool counted = root >= 0 && root < HW;                             // (labels of the dilated mask: a pixel of res has a root)
    unsigned long long left = __ballot(counted);
    // strictly decreasing: the bits of `left` (each round clears at least its lowest set bit)
    while (left) {
      const int leader = __ffsll((long long)left) - 1;
      const int kk = __shfl(k, leader, 64), rr = __shfl(root, leader, 64);
      const unsigned long long same = __ballot(counted && k == kk && root == rr);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&counts[(f * (L - 1) + (kk - 1)) * HW + rr], __popcll(same));
      left &= ~same;
    }
  }
}

// grid (planes): the plane's largest count, on a tie its smallest root, and the roots that hold a pixel.  The winning root (-1: the id is
// absent) is left in counts[plane][0] for the repaint.
__global__ __launch_bounds__(CC_KEEP_THREADS) void cc_largest_kernel(int* __restrict__ counts, const int HW, int* __restrict__ ncomp) {
  __shared__ unsigned long long best;
  __shared__ int held;
  const long plane = blockIdx.x;
  int* c = counts + plane * HW;
  if (threadIdx.x == 0) {
    best = 0ull;
    held = 0;
  }
  __syncthreads();
  unsigned long long mine = 0ull;
  int n = 0;
  const auto take = [&](const int v, const int p) {
    if (v > 0) {
      const unsigned long long key = ((unsigned long long)(unsigned)v << 32) | (unsigned)(0x7fffffff - p);
      mine = key > mine ? key : mine;
      ++n;
    }
  };
  // the counts up to the first 16-byte boundary one by one, then four at a time with four reads in flight, then the rest
  const int head = min(HW, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(c) & 15u)) & 15u) / 4u)), quads = (HW - head) / 4;
  if ((int)threadIdx.x < head) take(c[threadIdx.x], threadIdx.x);
  const int4* c4 = reinterpret_cast<const int4*>(c + head);
  for (int q0 = 0; q0 < quads; q0 += 4 * CC_KEEP_THREADS) {
    int4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = q0 + j * CC_KEEP_THREADS + threadIdx.x;
      v[j] = q < quads ? c4[q] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = head + 4 * (q0 + j * CC_KEEP_THREADS + threadIdx.x);
      take(v[j].x, p);
      take(v[j].y, p + 1);
      take(v[j].z, p + 2);
      take(v[j].w, p + 3);
    }
  }
  for (int p = head + 4 * quads + threadIdx.x; p < HW; p += CC_KEEP_THREADS) take(c[p], p);
  if (mine) atomicMax(&best, mine);
  if (n) atomicAdd(&held, n);
  __syncthreads();                                                           // every count of the plane has been read
  if (threadIdx.x == 0) {
    c[0] = best ? 0x7fffffff - (int)(unsigned)(best & 0xffffffffull) : -1;
    ncomp[plane] = held;
  }
}

// grid (blocks over a frame's pixels, frames): a pixel of id k outside k's winning component becomes 0
__global__ __launch_bounds__(CC_THREADS) void cc_repaint_kernel(const uint8_t* __restrict__ idmaps, const int* __restrict__ labels,
                                                                const int* __restrict__ counts, const int HW, const int L,
                                                                uint8_t* __restrict__ out, int* __restrict__ removed) {
  const long f = blockIdx.y;
  for (int p0 = blockIdx.x * CC_THREADS; p0 < HW; p0 += gridDim.x * CC_THREADS) {      // (the whole wave stays in the loop: the ballots)
    const int p = p0 + threadIdx.x;
    int k = 0;
    bool drop = false;
    if (p < HW) {
      k = idmaps[f * HW + p];
      if (k >= 1 && k < L) {
        const long plane = f * (L - 1) + (k - 1);
        drop = labels[plane * HW + p] != counts[plane * HW];
      }
      out[f * HW + p] = drop ? 0 : (uint8_t)k;
    }
    // per id present in the wave one integer add of the wave's dropped pixels of that id
    unsigned long long left = __ballot(drop);
    // strictly decreasing: the bits of `left` (each round clears at least its lowest set bit)
    while (left) {
      const int leader = __ffsll((long long)left) - 1;
      const int kk = __shfl(k, leader, 64);
      const unsigned long long same = __ballot(drop && k == kk);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&removed[f * (L - 1) + (kk - 1)], __popcll(same));
      left &= ~same;
    }
  }
}

int check_dims(const char* who, const int h, const int w) {
  PV_REQUIRE(h >= 1 && w >= 1, "%s: h, w >= 1 (got %d, %d)", who, h, w);
  PV_REQUIRE((long)h * w <= CC_MAX_PIXELS, "%s: h * w at most 2^26 (got %d x %d)", who, h, w);
  return PREMVOS_OK;
}

int check_stack(const char* who, const int n, const int h, const int w, const int L) {
  PV_REQUIRE(n >= 1, "%s: n >= 1 (got %d)", who, n);
  if (int rc = check_dims(who, h, w)) return rc;
  PV_REQUIRE(L >= CC_MIN_L && L <= CC_MAX_L, "%s: L from %d to %d (got %d)", who, CC_MIN_L, CC_MAX_L, L);
  return PREMVOS_OK;
}

unsigned grid_planes(const long planes) { return (unsigned)(planes < (long)CC_MAX_GRID_Y ? planes : (long)CC_MAX_GRID_Y); }

unsigned stride_blocks(const long items, const long cap) {
  const long blocks = (items + CC_THREADS - 1) / CC_THREADS;
  return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

extern "C" int premvos_cc_dilate_u8(const uint8_t* idmaps, int32_t n, int32_t h, int32_t w, int32_t L, int32_t D, uint8_t* dil, void* stream) {
  PV_REQUIRE(idmaps && dil, "cc_dilate: null pointer");
  if (int rc = check_stack("cc_dilate", n, h, w, L)) return rc;
  PV_REQUIRE(D >= CC_MIN_D && D <= CC_MAX_D, "cc_dilate: D from %d to %d (got %d)", CC_MIN_D, CC_MAX_D, D);
  const long planes = (long)n * (L - 1);
  const dim3 grid((unsigned)premvos::cdiv(w, CC_DIL_T), (unsigned)premvos::cdiv(h, CC_DIL_T), grid_planes(planes));
  PV_REQUIRE(grid.y <= CC_MAX_GRID_Y, "cc_dilate: h at most %u rows (got %d)", CC_MAX_GRID_Y * CC_DIL_T, h);
  hipLaunchKernelGGL(cc_dilate_kernel, grid, dim3(CC_THREADS), 0, static_cast<hipStream_t>(stream), idmaps, h, w, L, D, planes, dil);
  return premvos::check_launch("cc_dilate");
}

extern "C" int premvos_cc_label_i32(const uint8_t* masks, int64_t planes, int32_t h, int32_t w, int32_t* labels, void* stream) {
  PV_REQUIRE(masks && labels, "cc_label: null pointer");
  PV_REQUIRE(planes >= 1, "cc_label: planes >= 1 (got %lld)", (long long)planes);
  if (int rc = check_dims("cc_label", h, w)) return rc;
  const int tiles_x = premvos::cdiv(w, CC_TILE_W), tiles_y = premvos::cdiv(h, CC_TILE_H), tiles = tiles_x * tiles_y;      // <= 2^26 / 16 + ...
  PV_REQUIRE((unsigned)tiles_y <= CC_MAX_GRID_Y, "cc_label: h at most %u rows (got %d)", CC_MAX_GRID_Y * CC_TILE_H, h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned gp = grid_planes(planes);
  hipLaunchKernelGGL(cc_label_tile_kernel, dim3((unsigned)tiles_x, (unsigned)tiles_y, gp), dim3(CC_THREADS), 0, s, masks, h, w, (long)planes, labels);
  hipLaunchKernelGGL(cc_label_merge_kernel, dim3((unsigned)premvos::cdiv(tiles, CC_THREADS / CC_BORDER), gp), dim3(CC_THREADS), 0, s, h, w, tiles_x,
                     tiles, (long)planes, labels);
  const dim3 per_pixel(stride_blocks((long)h * w, 4096), gp);
  hipLaunchKernelGGL(cc_label_flatten_kernel<true>, per_pixel, dim3(CC_THREADS), 0, s, h * w, w, (long)planes, labels);
  hipLaunchKernelGGL(cc_label_flatten_kernel<false>, per_pixel, dim3(CC_THREADS), 0, s, h * w, w, (long)planes, labels);
  return premvos::check_launch("cc_label");
}

extern "C" int premvos_cc_keep_largest_u8(const uint8_t* idmaps, const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t L,
                                          int32_t* counts_ws, uint8_t* out_idmaps, int32_t* removed, int32_t* ncomp, void* stream) {
  PV_REQUIRE(idmaps && labels && counts_ws && out_idmaps && removed && ncomp, "cc_keep_largest: null pointer");
  if (int rc = check_stack("cc_keep_largest", n, h, w, L)) return rc;
  PV_REQUIRE(n <= (int)CC_MAX_GRID_Y, "cc_keep_largest: n at most %u frames a call (got %d)", CC_MAX_GRID_Y, n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long planes = (long)n * (L - 1);
  const int HW = h * w;
  if (hipMemsetAsync(counts_ws, 0, sizeof(int32_t) * (size_t)planes * HW, s) != hipSuccess ||
      hipMemsetAsync(removed, 0, sizeof(int32_t) * (size_t)planes, s) != hipSuccess ||
      hipMemsetAsync(ncomp, 0, sizeof(int32_t) * (size_t)planes, s) != hipSuccess)
    return premvos::fail(PREMVOS_ELAUNCH, "cc_keep_largest: memset failed");
  const dim3 per_frame(stride_blocks(HW, 1024), (unsigned)n);
  hipLaunchKernelGGL(cc_count_kernel, per_frame, dim3(CC_THREADS), 0, s, idmaps, labels, HW, L, counts_ws);
  hipLaunchKernelGGL(cc_largest_kernel, dim3((unsigned)planes), dim3(CC_KEEP_THREADS), 0, s, counts_ws, HW, ncomp);
  hipLaunchKernelGGL(cc_repaint_kernel, per_frame, dim3(CC_THREADS), 0, s, idmaps, labels, counts_ws, HW, L, out_idmaps, removed);
  return premvos::check_launch("cc_keep_largest");
}
