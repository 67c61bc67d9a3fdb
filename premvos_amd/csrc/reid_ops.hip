// ReID embedding net (code/ReID_net): the operations its wide pre-activation ResNet needs next to
// the dense convs (premvos_conv2d_f32), max-pool and the FC layers (1x1 convs):
//   * per-box crops     datasets/Similarity/DAVIS_Forward_Feed.py:62-96, Similarity.py:288-297 (one frame, or the slots of
//                       several frames in one launch)
//   * BatchNorm + ReLU on a tensor that is ALSO consumed raw (the unit's identity shortcut): NetworkLayers.py:171-173
//   * for masks that are already in HBM (the streaming driver's refined masks): their rleToBbox boxes and the context boxes
//     of those, so that nothing returns to the host between the masks and the embeddings
// All are HBM-bound or latency-bound passes.
#include "common.h"

namespace {

__device__ inline void tf_lerp(int d, float scale, int in_size, int* lo, int* hi, float* t) {   // TF1 legacy coordinates
  const float s = (float)d * scale;
  const float f = floorf(s);
  *lo = (int)f;
  const int c = (int)ceilf(s);
  *hi = c < in_size - 1 ? c : in_size - 1;
  *t = s - f;
}

// One output pixel (x, y) of the S x S crop of box (bx, by, bw, bh) of `frame` [H][W][3]: the code both crop kernels share, so a
// (frame, box) pair gives the same bits whichever of them runs it.  zero_small: boxes with min(w, h) <= 10 yield an all-zero
// image BEFORE normalisation (the in-merge feed dataset), as do empty boxes.
__device__ __forceinline__ float4 reid_pixel(const uint8_t* __restrict__ frame, int H, int W, int bx, int by, int bw, int bh,
                                             int x, int y, int S, int zero_small) {
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  // tensor slicing [y:y+h, x:x+w] clips to the image
  int x1 = bx + bw, y1 = by + bh;
  bx = bx < 0 ? 0 : bx; by = by < 0 ? 0 : by;
  x1 = x1 > W ? W : x1; y1 = y1 > H ? H : y1;
  const int wc = x1 - bx, hc = y1 - by;
  float v[3] = {0.f, 0.f, 0.f};
  const bool small = zero_small && (bw < bh ? bw : bh) <= 10;
  if (!small && wc > 0 && hc > 0) {
    int ylo, yhi, xlo, xhi;
    float ty, tx;
    tf_lerp(y, (float)hc / (float)S, hc, &ylo, &yhi, &ty);
    tf_lerp(x, (float)wc / (float)S, wc, &xlo, &xhi, &tx);
    const uint8_t* f00 = frame + ((long)(by + ylo) * W + bx + xlo) * 3;
    const uint8_t* f01 = frame + ((long)(by + ylo) * W + bx + xhi) * 3;
    const uint8_t* f10 = frame + ((long)(by + yhi) * W + bx + xlo) * 3;
    const uint8_t* f11 = frame + ((long)(by + yhi) * W + bx + xhi) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      // in-merge feed: image / 255 (DAVIS_Forward_Feed.py:27); batch stage: tf.image.convert_image_dtype = cast * (1 / 255)
      // (Util/Reader.py:162) -- not the same float for 126 of the 256 byte values
      const float r255 = 1.0f / 255.0f;
      const float tl = zero_small ? (float)f00[ch] / 255.f : (float)f00[ch] * r255;
      const float tr = zero_small ? (float)f01[ch] / 255.f : (float)f01[ch] * r255;
      const float bl = zero_small ? (float)f10[ch] / 255.f : (float)f10[ch] * r255;
      const float br = zero_small ? (float)f11[ch] / 255.f : (float)f11[ch] * r255;
      const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
      v[ch] = top + (bot - top) * ty;
    }
  }
  return make_float4((v[0] - mean[0]) / stdv[0], (v[1] - mean[1]) / stdv[1], (v[2] - mean[2]) / stdv[2], 0.f);
}

// boxes: int32 [n][4] = (x, y, w, h) already context-expanded / rounded / clipped (by the host, or by context_box below).
__global__ __launch_bounds__(256) void reid_input_kernel(const uint8_t* __restrict__ frame, int H, int W,
                                                         const int* __restrict__ boxes, int n, int S, int zero_small,
                                                         float* __restrict__ out) {
  const long total = (long)n * S * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int x = idx % S, y = (idx / S) % S, p = idx / ((long)S * S);
    *reinterpret_cast<float4*>(out + idx * 4) =
        reid_pixel(frame, H, W, boxes[p * 4], boxes[p * 4 + 1], boxes[p * 4 + 2], boxes[p * 4 + 3], x, y, S, zero_small);
  }
}

// The same crops for slots that belong to SEVERAL frames of one size: slot p is cut from frames[frame_of_slot[p]] (an index
// outside [0, F) is clamped: a padded slot carries the empty box and reads nothing).
__global__ __launch_bounds__(256) void reid_input_frames_kernel(const uint8_t* __restrict__ frames, int F, int H, int W,
                                                                const int* __restrict__ frame_of_slot,
                                                                const int* __restrict__ boxes, int n, int S, int zero_small,
                                                                float* __restrict__ out) {
  const long total = (long)n * S * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int x = idx % S, y = (idx / S) % S, p = idx / ((long)S * S);
    int f = frame_of_slot[p];
    f = f < 0 ? 0 : (f >= F ? F - 1 : f);
    *reinterpret_cast<float4*>(out + idx * 4) =
        reid_pixel(frames + (long)f * H * W * 3, H, W, boxes[p * 4], boxes[p * 4 + 1], boxes[p * 4 + 2], boxes[p * 4 + 3], x, y,
                   S, zero_small);
  }
}

// reid.model.context_boxes on one box: x1.2 around the centre in float32 IN NUMPY'S ORDER (x - (0.5 * w) * 0.2, w * 1.2; each
// product and the difference rounded on its own -- a fused multiply-add moves round-half-even ties such as x = 10, w = 5),
// tf.round, clip to the image; `feed`: an excess of at least one pixel (DAVIS_Forward_Feed.py:36-60), else Similarity.py:267-287.
__device__ inline int4 context_box(int bx, int by, int bw, int bh, int height, int width, int feed) {
#pragma clang fp contract(off)
  const float f = 0.2f, c = 1.2f;                         // float32(CONTEXT - 1.0), float32(CONTEXT)
  int xs = (int)rintf(__fsub_rn((float)bx, __fmul_rn(__fmul_rn(0.5f, (float)bw), f)));
  int ys = (int)rintf(__fsub_rn((float)by, __fmul_rn(__fmul_rn(0.5f, (float)bh), f)));
  int ws = (int)rintf(__fmul_rn((float)bw, c));
  int hs = (int)rintf(__fmul_rn((float)bh, c));
  xs = xs > 0 ? xs : 0;
  ys = ys > 0 ? ys : 0;
  const int lo = feed ? 1 : 0, ex = xs + ws - width, ey = ys + hs - height;
  ws -= ex > lo ? ex : lo;
  hs -= ey > lo ? ey : lo;
  return make_int4(xs, ys, ws, hs);
}

__global__ __launch_bounds__(256) void context_boxes_kernel(const int* __restrict__ boxes, int n, int height, int width, int feed,
                                                            int* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 b = *reinterpret_cast<const int4*>(boxes + i * 4);
  *reinterpret_cast<int4*>(out + i * 4) = context_box(b.x, b.y, b.z, b.w, height, width, feed);
}

// rleToBbox of a mask, from the mask: pass 1 -- block (slab, mask) finds the extent (xmin, xmax, ymin, ymax) of the foreground in
// its slab of rows.  Rows are read as aligned 32-bit words (a mask row of a 854-wide frame starts at any byte); a word that
// holds at least one byte of the row is read whole and the bytes outside [0, w) are ignored.
constexpr int kSlabs = PREMVOS_MASK_BBOX_SLABS;

__global__ __launch_bounds__(256) void mask_bbox_partial_kernel(const uint8_t* __restrict__ masks, int h, int w, long mask_stride,
                                                                int row_stride, int* __restrict__ partial) {
  const int s = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const int rows = (h + kSlabs - 1) / kSlabs, r0 = s * rows, r1 = r0 + rows < h ? r0 + rows : h;
  const uint8_t* m = masks + (long)i * mask_stride;
  int xmin = w, xmax = -1, ymin = h, ymax = -1;
  const int nw = (w + 3) / 4 + 1;                        // aligned words that may overlap a row
  const long total = r1 > r0 ? (long)(r1 - r0) * nw : 0;
  for (long idx = tid; idx < total; idx += 256) {
    const int y = r0 + (int)(idx / nw), k = (int)(idx % nw);
    const uint8_t* row = m + (long)y * row_stride;
    const int x0 = 4 * k - (int)(reinterpret_cast<uintptr_t>(row) & 3);        // column of the word's first byte (>= -3)
    if (x0 >= w) continue;
    const uint32_t v = *reinterpret_cast<const uint32_t*>(row + x0);
    if (v == 0) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int x = x0 + b;
      if (((v >> (8 * b)) & 0xffu) && x >= 0 && x < w) {
        xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax;
        ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
      }
    }
  }
  __shared__ int4 red[256];
  red[tid] = make_int4(xmin, xmax, ymin, ymax);
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) {
      const int4 a = red[tid], b = red[tid + d];
      red[tid] = make_int4(a.x < b.x ? a.x : b.x, a.y > b.y ? a.y : b.y, a.z < b.z ? a.z : b.z, a.w > b.w ? a.w : b.w);
    }
    __syncthreads();
  }
  if (tid == 0) *reinterpret_cast<int4*>(partial + ((long)i * kSlabs + s) * 4) = red[0];
}

// pass 2 -- one block per mask joins the slabs and applies maskApi.c rleToBbox's column rule: a foreground run that crosses a
// column boundary (mask[h-1][x] and mask[0][x+1] both set: the runs are column-major) makes y = 0 and the height the full h.
// Writes the box and, when `ctx` is given, its context box (context_box above, image = the mask's h x w).
__global__ __launch_bounds__(256) void mask_bbox_finish_kernel(const uint8_t* __restrict__ masks, int h, int w, long mask_stride,
                                                               int row_stride, const int* __restrict__ partial, int feed,
                                                               int* __restrict__ bbox, int* __restrict__ ctx) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const uint8_t* top = masks + (long)i * mask_stride;
  const uint8_t* bottom = top + (long)(h - 1) * row_stride;
  int cross = 0;
  for (int x = tid; x < w - 1; x += 256) cross |= (bottom[x] != 0) & (top[x + 1] != 0);
  cross = __syncthreads_or(cross);
  if (tid != 0) return;
  int xmin = w, xmax = -1, ymin = h, ymax = -1;
  for (int s = 0; s < kSlabs; ++s) {
    const int4 p = *reinterpret_cast<const int4*>(partial + ((long)i * kSlabs + s) * 4);
    xmin = p.x < xmin ? p.x : xmin; xmax = p.y > xmax ? p.y : xmax;
    ymin = p.z < ymin ? p.z : ymin; ymax = p.w > ymax ? p.w : ymax;
  }
  int4 b = make_int4(0, 0, 0, 0);                         // an empty mask
  if (xmax >= 0) b = cross ? make_int4(xmin, 0, xmax - xmin + 1, h) : make_int4(xmin, ymin, xmax - xmin + 1, ymax - ymin + 1);
  *reinterpret_cast<int4*>(bbox + i * 4) = b;
  if (ctx) *reinterpret_cast<int4*>(ctx + i * 4) = context_box(b.x, b.y, b.z, b.w, h, w, feed);
}

// out = max(in * scale[c] + shift[c], 0) (relu != 0) over NHWC pixels; float4 over channels.
__global__ __launch_bounds__(256) void scale_shift_relu_kernel(const float* __restrict__ in, int in_ps, long npix, int c4,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift, float* __restrict__ out,
                                                               int out_ps, int relu) {
  const long total = npix * c4;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int cg = idx % c4;
    const long p = idx / c4;
    const float4 v = *reinterpret_cast<const float4*>(in + p * in_ps + cg * 4);
    const float4 s = *reinterpret_cast<const float4*>(scale + cg * 4);
    const float4 t = *reinterpret_cast<const float4*>(shift + cg * 4);
    float4 r = make_float4(v.x * s.x + t.x, v.y * s.y + t.y, v.z * s.z + t.z, v.w * s.w + t.w);
    if (relu) {
      r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f);
    }
    *reinterpret_cast<float4*>(out + p * out_ps + cg * 4) = r;
  }
}

inline int grid_for(long total) {
  long g = (total + 255) / 256;
  return (int)(g > 65535L * 16 ? 65535L * 16 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int premvos_reid_input_u8(const uint8_t* frame_rgb, int32_t h, int32_t w, const int32_t* boxes_xywh, int32_t n,
                                     int32_t size, int32_t zero_small, float* out, void* stream) {
  PV_REQUIRE(frame_rgb && boxes_xywh && out, "reid_input: null pointer");
  PV_REQUIRE(h > 0 && w > 0 && n > 0 && size > 0, "reid_input: bad dims");
  PV_REQUIRE(premvos::aligned16(out), "reid_input: out must be 16-byte aligned");
  hipLaunchKernelGGL(reid_input_kernel, dim3(grid_for((long)n * size * size)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), frame_rgb, h, w, boxes_xywh, n, size, zero_small, out);
  return premvos::check_launch("reid_input");
}

extern "C" int premvos_reid_input_frames_u8(const uint8_t* frames_rgb, int32_t nframes, int32_t h, int32_t w,
                                            const int32_t* frame_of_slot, const int32_t* boxes_xywh, int32_t n, int32_t size,
                                            int32_t zero_small, float* out, void* stream) {
  PV_REQUIRE(frames_rgb && frame_of_slot && boxes_xywh && out, "reid_input_frames: null pointer");
  PV_REQUIRE(nframes > 0 && h > 0 && w > 0 && n > 0 && size > 0, "reid_input_frames: bad dims");
  PV_REQUIRE(premvos::aligned16(out), "reid_input_frames: out must be 16-byte aligned");
  hipLaunchKernelGGL(reid_input_frames_kernel, dim3(grid_for((long)n * size * size)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), frames_rgb, nframes, h, w, frame_of_slot, boxes_xywh, n, size, zero_small,
                     out);
  return premvos::check_launch("reid_input_frames");
}

extern "C" int premvos_reid_context_boxes_i32(const int32_t* boxes_xywh, int32_t n, int32_t height, int32_t width, int32_t feed,
                                              int32_t* out, void* stream) {
  PV_REQUIRE(boxes_xywh && out, "reid_context_boxes: null pointer");
  PV_REQUIRE(n > 0 && height > 0 && width > 0, "reid_context_boxes: bad dims");
  PV_REQUIRE(premvos::aligned16(boxes_xywh) && premvos::aligned16(out), "reid_context_boxes: boxes must be 16-byte aligned");
  hipLaunchKernelGGL(context_boxes_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), boxes_xywh, n,
                     height, width, feed, out);
  return premvos::check_launch("reid_context_boxes");
}

extern "C" int premvos_mask_bbox_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, int64_t mask_stride,
                                    int32_t row_stride, int32_t feed, int32_t* bbox_xywh, int32_t* context_xywh,
                                    int32_t* workspace, void* stream) {
  PV_REQUIRE(masks && bbox_xywh && workspace, "mask_bbox: null pointer");
  PV_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && row_stride >= w && mask_stride >= (int64_t)(h - 1) * row_stride + w,
             "mask_bbox: bad dims or strides");
  PV_REQUIRE(premvos::aligned16(bbox_xywh) && premvos::aligned16(workspace) && premvos::aligned16(context_xywh),
             "mask_bbox: boxes and workspace must be 16-byte aligned");
  hipLaunchKernelGGL(mask_bbox_partial_kernel, dim3(kSlabs, n), dim3(256), 0, static_cast<hipStream_t>(stream), masks, h, w,
                     (long)mask_stride, row_stride, workspace);
  hipLaunchKernelGGL(mask_bbox_finish_kernel, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), masks, h, w,
                     (long)mask_stride, row_stride, workspace, feed, bbox_xywh, context_xywh);
  return premvos::check_launch("mask_bbox");
}

extern "C" int premvos_scale_shift_relu_f32(const float* in, int32_t in_ps, int64_t npix, int32_t c, const float* scale,
                                            const float* shift, float* out, int32_t out_ps, int32_t relu, void* stream) {
  PV_REQUIRE(in && scale && shift && out, "scale_shift_relu: null pointer");
  PV_REQUIRE(npix > 0 && c > 0 && c % 4 == 0 && in_ps % 4 == 0 && out_ps % 4 == 0 && in_ps >= c && out_ps >= c,
             "scale_shift_relu: C and strides must be multiples of 4");
  PV_REQUIRE(premvos::aligned16(in) && premvos::aligned16(out) && premvos::aligned16(scale) && premvos::aligned16(shift),
             "scale_shift_relu: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(scale_shift_relu_kernel, dim3(grid_for((long)npix * (c / 4))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, in_ps, (long)npix, c / 4, scale, shift, out, out_ps, relu);
  return premvos::check_launch("scale_shift_relu");
}
