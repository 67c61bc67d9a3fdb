/*
 * premvos_hip.h -- C-ABI of libpremvos_hip.so: the MI355X (gfx950) kernels behind the
 * PReMVOS per-frame dense hot path (PWC-Net flow, proposal_net, refinement_net forward).
 *
 * Boundary rules:
 *   - extern "C", raw DEVICE pointers + explicit sizes/strides, caller-owned buffers;
 *   - every entry point is asynchronous on the hipStream_t handed in (void* here so the
 *     header needs no HIP include), no hidden synchronisation, no global state;
 *   - returns 0 on success, <0 on argument / launch error (message: premvos_last_error()),
 *     never exit()s -- unlike the reference FFI, which "returns 1 always" and exit(-1)s on
 *     a failed launch (correlation_package/src/corr_cuda.c:80, corr_cuda_kernel.cu:49-54).
 *
 * Layout: activations are NHWC ("pixel major") fp32 with an explicit pixel stride `ps`
 * (in elements) so a tensor may be a channel slice [coff, coff+C) of a wider concat
 * buffer: pass `base + coff` and the buffer's `ps`.  Slices used as conv INPUT need
 * (pointer % 16 B == 0), ps % 4 == 0 and roundup(C,4) readable finite floats per pixel.
 *
 * The reference interface each function replaces is cited as file:line relative to
 * /root/reference/code/.
 */
#ifndef PREMVOS_HIP_H
#define PREMVOS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PREMVOS_OK 0
#define PREMVOS_EINVAL (-1)
#define PREMVOS_ELAUNCH (-2)
#define PREMVOS_EUNSUPPORTED (-3) /* valid input outside what the entry point covers (premvos_jpeg_*: the caller falls back) */
#define PREMVOS_ENOSPACE (-4) /* the caller's output buffer is too small (premvos_jpeg_entropy_encode_host); nothing was written past it */

/* activation enum for the fused conv epilogue */
#define PREMVOS_ACT_NONE 0
#define PREMVOS_ACT_RELU 1
#define PREMVOS_ACT_LEAKY 2 /* x > 0 ? x : slope * x   (nn.LeakyReLU(0.1), PWCNet.py:28) */
#define PREMVOS_ACT_SIGMOID 3 /* 1/(1+exp(-x))   (mask head, proposal_net/train.py:305) */
/* OR-ed into `act` of premvos_dwconv3x3_f32: store the result in the resident split layout "S8" of the bf16x3 mode -- every group
 * of EIGHT channels of a pixel is the 32 bytes {hi(8 x bf16), lo(8 x bf16)}, x = hi + lo (hi = bf16(x) round-to-nearest-even,
 * lo = bf16(x - hi)), in place of its eight floats (pixel stride a multiple of 8 floats' worth, channel window 32-byte aligned)
 * -- the operand form of premvos_conv_bf16x3_s8_f32.  (Round 3's {hi4, lo4} groups, 0x100, and their consumer are gone.) */
#define PREMVOS_ACT_SPLIT8_BF16 0x200

/* arithmetic of the dense-conv MFMA pipe (activations and outputs are fp32 in HBM in every mode) */
#define PREMVOS_PREC_F32 0    /* v_mfma_f32_32x32x2_f32: exact fp32 products (the parity / default bench mode)        */
#define PREMVOS_PREC_BF16 1   /* v_mfma_f32_32x32x16_bf16 on bf16(a), bf16(b), fp32 accumulate                        */
#define PREMVOS_PREC_BF16X3 3 /* split-bf16: hi*hi + hi*lo + lo*hi, fp32 accumulate (~2^-17 relative per product)    */

/* output scatter mode of the conv epilogue */
#define PREMVOS_OUT_NHWC 0
#define PREMVOS_OUT_PIXSHUF2 1 /* column j = phase*cout_ps + co -> out[2y+phase/2][2x+phase%2][co] */

const char* premvos_last_error(void);
int premvos_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Dense convolution as implicit GEMM on the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32),
 * fused bias (+ folded BatchNorm) + residual add + activation, writing into a channel
 * slice of a (concat) buffer.
 *
 * Replaces every dense conv call the reference makes through its frameworks:
 *   optical_flow_net-PWC-Net/models/PWCNet.py:24-34 (conv / predict_flow / deconv builders),
 *   proposal_net/basemodel.py:51-99 (Conv2D+BNReLU bottlenecks), proposal_net/model.py:30-51,
 *   refinement_net/network/deeplab/core/xception.py:154-178 (pointwise halves), model.py:383-433.
 *
 * Weights are pre-packed by the host (premvos_amd/ops.py: pack_conv) as a row-major matrix
 * wgt[cout_pad][k_pad], k = (kh*KW + kw)*cin_pad + c, cin_pad = roundup(cin,4),
 * k_pad = roundup(KH*KW*cin_pad, 16), cout_pad = roundup(cout, 32); zero filled padding.
 * ---------------------------------------------------------------------------------------- */
typedef struct premvos_conv_desc {
  const float* in;      /* NHWC slice base */
  const float* wgt;     /* packed weights  */
  const float* bias;    /* [cout_pad] or NULL */
  const float* res;     /* residual NHWC slice (same N,Ho,Wo,cout) or NULL; added before act */
  float* out;           /* NHWC slice base */
  int32_t n, h, w, cin; /* input dims      */
  int32_t in_ps;        /* input pixel stride (elements) */
  int32_t ho, wo, cout; /* output dims     */
  int32_t out_ps;       /* output pixel stride */
  int32_t res_ps;       /* residual pixel stride */
  int32_t kh, kw;       /* kernel          */
  int32_t sh, sw;       /* stride          */
  int32_t dh, dw;       /* dilation        */
  int32_t pt, pl;       /* pad top / left (bottom/right follow from ho,wo: asymmetric pads ok) */
  int32_t cin_pad, k_pad, cout_pad;
  int32_t act;          /* PREMVOS_ACT_*   */
  float slope;          /* leaky slope     */
  int32_t out_mode;     /* PREMVOS_OUT_*   */
  int32_t cout_ps;      /* PIXSHUF2: channels per phase (cout == 4*cout_ps); out dims are 2ho x 2wo */
  int32_t tile_hint;    /* 0 = auto; (BM<<16)|BN forces an MFMA tile config; 1 forces the direct kernel for cout <= 2;  */
                        /* 2 = Winograd F(2x2,3x3) (csrc/conv_wino_f32.hip; needs wgt_wino), 16 component slabs in the  */
                        /* workspace + an output-transform launch; 3 = the same algebra in ONE kernel without workspace */
                        /* (a workgroup walks all 16 components of its block; output transform from registers);         */
                        /* 4 = Winograd F(4x4,3x3) (needs wgt_wino4 + workspace): 4x fewer multiplies, for K-rich layers  */
                        /*     (3x3 / stride 1; atrous layers with dilation d = pad run as d x d interleaved sub-lattices)      */
                        /* 5 = short-K pointwise layers (1x1, stride 1, cin = 64 | 128 = k_pad, cout % 128 == 0, <= 512):   */
                        /* persistent workgroups, weights resident in LDS (csrc/conv_stream_f32.hip); the implicit GEMM's sums */
                        /* 6 = pointwise layers (1x1, no padding, any stride, k_pad >= 32, cout % 4 == 0, 16-byte aligned pixels): */
                        /* 128 x 128 tiles with both operands staged by LDS-DMA (csrc/conv_pwdma_f32.hip); the implicit GEMM's sums */
  int32_t split_k;      /* 0 = auto, <0 = never, >0 = force this many k-slices */
  float* workspace;     /* split-K partial slabs (may be NULL: then never split) */
  int64_t workspace_bytes;
  int32_t precision;    /* PREMVOS_PREC_*; bf16 modes: wgt = bf16 hi [cout_pad][k_pad], k_pad % 32 == 0 */
  int32_t stage_k;      /* fp32 path: k depth of an LDS stage, 16 or 32 (0 = library default); with tile_hint == 2: 64 = 64 */
                        /* instead of 128 tile rows per workgroup; with tile_hint == 3: the block (2x2-tile rows x      */
                        /* couts / waves / stage depth) of a workgroup: 0, 2..6 (table in csrc/conv_wino_f32.hip)       */
                        /* with tile_hint == 0 / 1 on a 1-2 channel head: 1 = keep the per-pixel form (csrc/conv_smalln_f32.hip) */
  const void* wgt_lo;   /* BF16X3: bf16 low parts (w - float(hi)), same shape as wgt */
  int32_t tail_m_tiles; /* fp32 path, unsplit layers: the last tail_m_tiles rows of BM-tall output tiles are computed  */
  int32_t tail_split_k; /* as tail_split_k k-slices + fixed-order reduce (fills a partly empty last wave); 0 = off    */
  const float* wgt_wino; /* optional (3x3 / stride 1 / dilation 1 / fp32 / cout % 4 == 0): the 16 Winograd F(2x2,3x3) filter  */
                         /* transforms U[c] = (G g G^T)[c/4][c%4], each packed [cout_pad][roundup(cin_pad,16)] with k = cin;   */
                         /* used when tile_hint == 2 (needs premvos_conv2d_workspace_bytes() of workspace); NULL = not packed */
  const float* wgt_wino4; /* optional, same layers: the 36 Winograd F(4x4,3x3) filter transforms U[6i+j] = (G g G^T)[i][j], packed  */
                          /* like wgt_wino; used when tile_hint == 4 (csrc/conv_wino4_f32.hip: input transform, 36 batched GEMMs,  */
                          /* output transform around workspace slabs; stage_k = GEMM block: +64 = 64 instead of 128 tile rows per  */
                          /* workgroup, +16 = 16- instead of 32-deep stages)                                                        */
} premvos_conv_desc;

int premvos_conv2d_f32(const premvos_conv_desc* d, void* stream);
/* bytes of `workspace` the descriptor needs for its (auto or forced) split-K plan; 0 = runs unsplit.  Layers with
 * too few output tiles to fill the chip (coarse PWC levels, batch-1 feature maps) are cut along K into slabs that
 * a second kernel sums in a fixed order before the fused epilogue (deterministic, unlike atomics). */
int64_t premvos_conv2d_workspace_bytes(const premvos_conv_desc* d);

/* Winograd F(4x4,3x3) with a KEPT input-transform slab, for DenseNet blocks: PWC-Net's flow estimators
 * (PWCNet.py:201-264, `x = torch.cat((self.convL_i(x), x), 1)`) feed layer i the concat of everything layers 0 ... i-1
 * produced, so premvos_conv2d_f32 with tile_hint 4 transforms the same channels again in every layer of a level.  Here the
 * caller owns ONE slab per concat buffer, V[36][tiles][v_pitch] floats (tiles = n * ceil(ho/4) * ceil(wo/4); slab channel =
 * channel of the concat buffer), and every layer adds only what is new:
 *   d        the layer's descriptor as for premvos_conv2d_f32 (wgt_wino4 packed; `in` = first channel of its input window;
 *            stage_k = GEMM block as with tile_hint 4); d->workspace holds the M slab: 36 * tiles * roundup(cout, 64 or 128) floats
 *   v_c0     slab channel of the window's first channel; the GEMM reads slab channels [v_c0, v_c0 + Kp), Kp = roundup(cin_pad, 16)
 *   t_cn     channels [0, t_cn) of the window are transformed by this call (0: everything is in the slab already); channels
 *            >= cin_pad are written as zeros, so t_cn = Kp on the first layer of a level zero-fills the K padding for all
 *            (every window of a level ends at the same channel)
 * v_pitch, v_c0, t_cn: multiples of 4, v_c0 + Kp <= v_pitch, t_cn <= Kp.  Same V values, same GEMM, same output transform as the
 * self-contained form: bit-identical results (tests/test_gpu_conv_wino.py).  PREMVOS_EINVAL if the layer is not an F(4x4) layer. */
int premvos_conv_wino4_slab_f32(const premvos_conv_desc* d, float* vslab, int64_t vslab_bytes, int32_t v_pitch, int32_t v_c0, int32_t t_cn,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * PWC-Net cost volume, the only first-party native kernel of the reference:
 *   corr_cuda_forward  correlation_package/src/corr_cuda.c:7-82
 *   blob_rearrange_kernel2 / CorrelateData  src/corr_cuda_kernel.cu:18-37, 59-127
 * for the instantiation PWC-Net uses (pad = max_displacement = md, kernel_size = 1,
 * stride1 = stride2 = 1, multiply; PWCNet.py:69):
 *   out[y][x][(dy+md)*(2md+1) + (dx+md)] = (1/C) * sum_c f1[y][x][c] * f2[y+dy][x+dx][c]
 * (zero outside), with the LeakyReLU the reference applies right after (PWCNet.py:198)
 * fused when `slope` != 1, written into channels [0, (2md+1)^2) of `out`; if `copy_f1`
 * the f1 features are also copied to channels [(2md+1)^2, +C) (the torch.cat of
 * PWCNet.py:213).  No NCHW->NHWC rearrange pass and no zeroed scratch: inputs ARE NHWC.
 * ---------------------------------------------------------------------------------------- */
int premvos_corr_fwd_f32(const float* f1, int32_t f1_ps, const float* f2, int32_t f2_ps, float* out,
                         int32_t out_ps, int32_t n, int32_t h, int32_t w, int32_t c, int32_t md,
                         float slope, int32_t copy_f1, void* stream);

/* General form of the reference op signature (pad_size, kernel_size, max_displacement, stride1,
 * stride2, corr_type_multiply) on NCHW tensors -- the exact argument list of corr_cuda_forward
 * (corr_cuda.h:1-11) minus the THCudaTensor scratch (rbot1/rbot2 are not needed).  Supports the
 * multiply type only (the reference's subtract path is never instantiated by PWCNet.py).
 * out must hold n * D*D * oh * ow floats (shape math of corr_cuda.c:23-45). */
int premvos_corr_nchw_fwd_f32(const float* in1, const float* in2, float* out, int32_t n, int32_t c,
                              int32_t h, int32_t w, int32_t pad_size, int32_t kernel_size,
                              int32_t max_displacement, int32_t stride1, int32_t stride2,
                              int32_t corr_type_multiply, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward bilinear warp of image-2 features by (flow * flow_scale) times the validity mask
 * (grid_sample(ones) >= 0.9999): PWCDCNet.warp, models/PWCNet.py:140-176, torch-0.2 grid_sample
 * (bilinear, zeros padding, align_corners=True).  flow is NHWC with 2 channels (u,v).
 * ---------------------------------------------------------------------------------------- */
int premvos_warp_fwd_f32(const float* x, int32_t x_ps, const float* flow, int32_t flow_ps, float flow_scale,
                         float* out, int32_t out_ps, int32_t n, int32_t h, int32_t w, int32_t c,
                         void* stream);

/* The two calls above fused for pyramid levels 5..2 (PWCNet.py:207-208, 220-221, ...: warp5 = self.warp(c25, up_flow5*0.625);
 * corr5 = self.corr(c15, warp5)): the image-2 features x2 are warped while the cost-volume kernel stages its f2 tile, so
 * the warped map is never written to HBM.  Bit-identical to premvos_warp_fwd_f32 followed by premvos_corr_fwd_f32.
 * md must be 4. */
int premvos_warp_corr_fwd_f32(const float* f1, int32_t f1_ps, const float* x2, int32_t x2_ps, const float* flow,
                              int32_t flow_ps, float flow_scale, float* out, int32_t out_ps, int32_t n, int32_t h,
                              int32_t w, int32_t c, int32_t md, float slope, int32_t copy_f1, void* stream);

/* layout plumbing at the stage edges (the reference nets take/return NCHW) */
int premvos_nchw_to_nhwc_f32(const float* in, float* out, int32_t out_ps, int32_t n, int32_t c, int32_t h,
                             int32_t w, void* stream);
int premvos_nhwc_to_nchw_f32(const float* in, int32_t in_ps, float* out, int32_t n, int32_t c, int32_t h,
                             int32_t w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flow-stage host pre/post processing moved on-device (script_pwc_multi.py:33-70):
 *  pre : `batch` pairs of HWC uint8 RGB frames (im1/im2: [batch][h][w][3]) -> cv2.resize(INTER_LINEAR,
 *        uint8 fixed point) to (w_,h_) -> BGR, /255 -> NHWC fp32 [2*batch][h_][w_][4] (4th channel 0;
 *        images [0,batch) = first frames, [batch,2*batch) = second frames)             (:38-56)
 *  post: flow2 NHWC [batch][h4][w4][flow_ps] (u,v in ch 0,1) -> x20 -> cv2.resize(float INTER_LINEAR) to
 *        (w,h) -> u*=w/w_, v*=h/h_ -> [batch][h][w][2] (the .flo payload layout)        (:59-68)
 * ---------------------------------------------------------------------------------------- */
int premvos_flow_preprocess_u8(const uint8_t* im1, const uint8_t* im2, int32_t batch, int32_t h, int32_t w,
                               float* out, int32_t h_, int32_t w_, void* stream);
int premvos_flow_postprocess_f32(const float* flow2, int32_t flow_ps, int32_t batch, int32_t h4, int32_t w4,
                                 float* out, int32_t h, int32_t w, int32_t h_, int32_t w_, void* stream);

/* ==========================================================================================
 * proposal_net (class-agnostic ResNet-101-C4 Faster R-CNN, `train.py --forward`); paths relative to
 * code/proposal_net/.  The dense convs (backbone, RPN head, conv5, FC heads as 1x1 convs) go through
 * premvos_conv2d_f32 with the frozen BatchNorm folded into weights+bias.
 * ========================================================================================== */

/* eval.py:76-77 CustomResize (cv2.resize INTER_LINEAR on the uint8 BGR frame) + basemodel.py:12-26
 * (x/255 - mean)/std in BGR order -> NHWC fp32 [batch][nh][nw][4] (4th channel 0).  src_is_rgb != 0: the
 * source frame is RGB (as the flow / refinement stages read it) and is channel-swapped on load. */
int premvos_proposal_preprocess_u8(const uint8_t* img_bgr, int32_t batch, int32_t h, int32_t w, float* out,
                                   int32_t nh, int32_t nw, int32_t src_is_rgb, void* stream);

/* MaxPooling('pool0', shape=3, stride=2) after tf.pad [0,1] (basemodel.py:81-82); generic k/stride/pad. */
int premvos_maxpool_f32(const float* in, int32_t in_ps, int32_t n, int32_t h, int32_t w, int32_t c, float* out,
                        int32_t out_ps, int32_t ho, int32_t wo, int32_t k, int32_t stride, int32_t pt, int32_t pl,
                        float pad_value, void* stream);

/* generate_rpn_proposals (model.py:169-217) fused with the anchor field (data.py:34-74, train.py:92-105) and
 * decode_bbox_target (model.py:113-139): per image, top-`pre_nms_topk` logits (ties -> lower index), clip to
 * the image, drop w/h <= min_size, greedy NMS (IoU > nms_thresh suppressed, TF IoU) keeping <= post_nms_topk
 * in descending-score order.  rpn is the NHWC output of the fused RPN 1x1 heads: logits at channel
 * [logit_off, +na), deltas at box_off + a*4 + {tx,ty,tw,th}.  out_idx are flat anchor indices
 * (y*fw + x)*na + a -- the 'bit-exact proposal indices' of the north star.  Unused slots: zeros / -1. */
int premvos_rpn_proposals_f32(const float* rpn, int32_t ps, int32_t n, int32_t fh, int32_t fw, int32_t na,
                              int32_t logit_off, int32_t box_off, const float* cell_anchors, float stride,
                              float img_h, float img_w, int32_t pre_nms_topk, int32_t post_nms_topk,
                              float nms_thresh, float min_size, float decode_clip, float* out_boxes,
                              float* out_scores, int32_t* out_idx, int32_t* out_count, void* stream);

/* roi_align (model.py:300-374): tf.image.crop_and_resize to (2*out_size)^2 on the remapped box, extrapolation 0,
 * fused with the 2x2 average pool.  rois: [n_img][rois_per_img][4] x1y1x2y2 in IMAGE coordinates, scaled by
 * spatial_scale (1/16); slots >= count[img] produce zeros.  out: NHWC [n_img*rois_per_img][out][out][c]. */
int premvos_roi_align_f32(const float* fmap, int32_t fmap_ps, int32_t n_img, int32_t h, int32_t w, int32_t c,
                          const float* rois, const int32_t* count, int32_t rois_per_img, float spatial_scale,
                          int32_t out_size, float* out, int32_t out_ps, void* stream);

/* The same RoIAlign (same sample coordinates, same order of the sums) with a bin stride and an epilogue.  bin_step 1 or 2: only the
 * bins with by % bin_step == 0 && bx % bin_step == 0 are computed, written densely as
 * [n_img*rois_per_img][ceil(out_size/bin_step)][ceil(out_size/bin_step)][c] (what a 1x1 stride-2 conv reads of the full output).
 * bias: NULL or c floats (16-byte aligned), added after the 2x2 average; act: PREMVOS_ACT_NONE or PREMVOS_ACT_RELU, applied last.
 * Slots >= count[img] hold act(0 + bias).  RoIAlign is linear in the feature values (bilinear samples, extrapolation value 0), so
 * a 1x1 conv without bias commutes with it: conv1x1 + bias + act on RoIs = this function on the projected feature map. */
int premvos_roi_align_epi_f32(const float* fmap, int32_t fmap_ps, int32_t n_img, int32_t h, int32_t w, int32_t c,
                              const float* rois, const int32_t* count, int32_t rois_per_img, float spatial_scale,
                              int32_t out_size, int32_t bin_step, const float* bias, int32_t act, float* out,
                              int32_t out_ps, void* stream);

/* GlobalAvgPooling (model.py:387,561): NHWC [n][hw][c] -> [n][c]. */
int premvos_global_avgpool_f32(const float* in, int32_t in_ps, int32_t n, int32_t hw, int32_t c, float* out,
                               int32_t out_ps, void* stream);

/* Inference tail (train.py:275-295, model.py:438-491) for NUM_CLASS=2: softmax, decode deltas / reg weights on
 * the proposals, clip, p > score_thresh, NMS(nms_thresh), <= max_out results by descending p.
 * head: [n_img][rois_per_img][head_ps] with class logits at [0,2) and box deltas at [2,6). */
int premvos_frcnn_tail_f32(const float* head, int32_t head_ps, const float* rois, const int32_t* count, int32_t n_img,
                           int32_t rois_per_img, float img_h, float img_w, float score_thresh, float nms_thresh,
                           int32_t max_out, float decode_clip, float rw_x, float rw_y, float rw_w, float rw_h,
                           float* out_boxes, float* out_probs, int32_t* out_idx, int32_t* out_count, void* stream);

/* ==========================================================================================
 * refinement_net (DeepLabv3+ / Xception-65 on 385x385 box crops); paths relative to code/refinement_net/.
 * Pointwise / dense convs go through premvos_conv2d_f32 (BatchNorm folded, ReLU and the module's
 * residual add fused in the epilogue).
 * ========================================================================================== */

/* Per-box network input, fusing datasets/util/BoundingBox.py:15-19 (guidance = 1 inside round(box)),
 * datasets/Resize.py:150-193 (crop = round(box) +- 50 px clipped; image: tf.image.resize_images bilinear,
 * guidance: resize_nearest_neighbor, both TF1-legacy coordinates), util/Normalization.py:9-21 and
 * DeepLabV3Plus.py:12-14 + core/feature_extractor.py:114-116.  frame: uint8 RGB [h][w][3];
 * boxes: [max_boxes][4] (y0,x0,y1,x1) floats; *count boxes are valid (rest -> zeros).
 * out: NHWC [max_boxes][size][size][4]; crop_boxes: [max_boxes][4] int32 (y0,x0,y1,x1). */
int premvos_refine_input_u8(const uint8_t* frame_rgb, int32_t h, int32_t w, const float* boxes_y0x0y1x1,
                            const int32_t* count, int32_t max_boxes, int32_t size, float* out, int32_t* crop_boxes,
                            void* stream);

/* Depthwise 3x3 (+stride, +atrous) with folded BatchNorm, optional ReLU on the INPUT (the xception module's
 * leading tf.nn.relu, core/xception.py:252-258) and on the output (exit flow / ASPP / decoder):
 * slim.separable_conv2d(num_outputs=None) of core/xception.py:154-167 and model.py:664-707.
 * wgt: [9][c_pad] (tap-major, BN scale folded), bias: [c_pad] or NULL. */
int premvos_dwconv3x3_f32(const float* in, int32_t in_ps, int32_t n, int32_t h, int32_t w, int32_t c,
                          const float* wgt, const float* bias, int32_t c_pad, float* out, int32_t out_ps, int32_t ho,
                          int32_t wo, int32_t stride, int32_t dilation, int32_t pt, int32_t pl, int32_t pre_relu,
                          int32_t act, void* stream);

/* Host only (no GPU call): WHICH kernel instance premvos_dwconv3x3_f32 launches for a shape -- the launcher takes its decision
 * from the same function, so the tests that must reach every instance (tests/dwconv_cases.py) can see which one a case reaches.
 * Validates like the launcher (what does not need the buffers); returns -1 on a bad argument, else the code
 *   bits  0-1   kernel family: PREMVOS_DW_TILE (register tile), PREMVOS_DW_ROW (row kernel), PREMVOS_DW_PIXEL (per pixel)
 *   bits  2-4   TW, output columns per thread (tile: 4 or 5, row: 4, per pixel: 1)
 *   bits  5-8   TR, output rows per thread    (tile: 4, 5 or 8, row and per pixel: 1)
 *   bit   9     AHEAD: the tile kernel keeps one input row in flight ahead of the row it consumes (dilation <= 4)
 *   bit   10    PRE_RELU
 *   bits 11-12  STRIDE template argument (tile: 1, row: 1 or 2; 0 = the per-pixel kernel, which takes any stride at run time)
 *   bits 13-14  store form: PREMVOS_DW_STORE_F32, PREMVOS_DW_STORE_S8 (two 8-byte stores per lane, c_pad/4 odd) or
 *               PREMVOS_DW_STORE_S8_PAIRED (c_pad/4 even: neighbouring lanes swap a half by DPP, one 16-byte store per lane)
 * A dilated tile (dilation > 1) maps its 4x4 tiles onto the dilation x dilation sub-lattices of the output. */
#define PREMVOS_DW_TILE 1
#define PREMVOS_DW_ROW 2
#define PREMVOS_DW_PIXEL 3
#define PREMVOS_DW_STORE_F32 0
#define PREMVOS_DW_STORE_S8 1
#define PREMVOS_DW_STORE_S8_PAIRED 2
int premvos_dwconv3x3_variant(int32_t n, int32_t h, int32_t w, int32_t c_pad, int32_t ho, int32_t wo, int32_t stride,
                              int32_t dilation, int32_t pre_relu, int32_t act);

/* Round 4: the bf16x3 mode on activations RESIDENT in the split layout "S8" -- per pixel, every group of 8 channels is the 32 bytes
 * {hi(8 x bf16), lo(8 x bf16)} (x = hi + lo; 4 bytes per element like fp32, pixel stride a multiple of 8 floats' worth of bytes,
 * channel windows 32-byte aligned).  Any conv of the three nets (1x1 / k x k, stride, dilation, asymmetric zero padding: the same
 * geometry fields of premvos_conv_desc as premvos_conv2d_f32, out_mode NHWC; replaces what the reference reaches through
 * tensorpack Conv2D basemodel.py:29-99, slim.conv2d / separable_conv2d's pointwise half xception.py:154-178, nn.Conv2d
 * PWCNet.py:24-34) as an implicit GEMM on v_mfma_f32_32x32x16_bf16: hi.hi + hi.lo + lo.hi, fp32 accumulate, operands staged by
 * LDS-DMA.  d->inp / d->wgt are IGNORED: in_s8 = the S8 input (d->in_ps its pixel stride, d->cin % 8 == 0), wgt_s8 = weights
 * packed as bf16 [cout_pad][kh*kw][ceil(cin/32)][4 groups][hi 8 | lo 8], zero padded (premvos_amd.ops.pack_conv_s8).
 * Outputs, each optional (at least one): d->out (fp32 NHWC, d->out_ps) and out_s8 (S8, pixel stride out_s8_ps floats' worth) =
 * act(sum + d->bias (+ d->res, fp32 -- or res_s8, the residual in S8 with pixel stride res_s8_ps: hi + lo, so that a bottleneck
 * chain needs no fp32 copy of its block outputs)); cout % 8 == 0.  tile: 0 = 256x256 / 8 waves / 2 buffers, 1 = 256x128 / 4 waves / 3 buffers,
 * 2 = 256x128 / 4 waves / 2 buffers, 3 = 256x128 / 8 waves / 3 buffers, 4 = 128x128 / 4 waves / 3 buffers, 5 = 128x128 / 2 buffers,
 * 6 / 7 = 256x128 and 8 = 128x256 on 16-channel stages (two workgroups per CU), 9 = 256x64, 10 = 256x256 ping-pong wave groups
 * (pointwise layers), 11 = 256x256 / 4 waves of 128x128.  Every tile adds an output's products in the same order: bit-identical
 * results -- the tile is a speed knob only (premvos_amd.ops.s8_tile_rule picks 0 or 5; the others are measured alternatives). */
int premvos_conv_bf16x3_s8_f32(const premvos_conv_desc* d, const void* in_s8, const void* wgt_s8, void* out_s8,
                               int32_t out_s8_ps, const void* res_s8, int32_t res_s8_ps, int32_t tile, void* stream);

/* fp32 NHWC [pixels][in_ps] -> S8 [pixels][out_ps floats' worth] (c channels; a partial last group is zero filled): the entry of an
 * S8 chain whose producer is an fp32 kernel. */
int premvos_split8_f32(const float* in, int32_t in_ps, void* out_s8, int32_t out_ps, int64_t pixels, int32_t c, void* stream);

/* tf.image.resize_bilinear, TF1: align_corners=1 (model.py:399-400,570-571) or 0 = legacy src = dst*in/out. */
int premvos_resize_bilinear_f32(const float* in, int32_t in_ps, int32_t n, int32_t h, int32_t w, int32_t c, float* out,
                                int32_t out_ps, int32_t ho, int32_t wo, int32_t align_corners, void* stream);

/* [n][1][1][c] -> every pixel of [n][h][w][c-slice]: the ASPP image-level feature (model.py:396-400). */
int premvos_broadcast_pixel_f32(const float* in, int32_t in_ps, int32_t n, int32_t c, float* out, int32_t out_ps,
                                int32_t h, int32_t w, void* stream);

/* SegmentationSoftmax eval branch (network/SegmentationOutputLayers.py:35-61,106-135) + the forwarder's
 * conf_score (forwarding/FewShotSegmentationForwarder.py:144-148): logits [max_boxes][lh][lw][ps>=2] ->
 * legacy-bilinear to size^2 -> softmax/argmax -> mask (nearest) and posterior (legacy bilinear) resized to the
 * crop box and zero padded to the frame.  mask: uint8 {0,1} [max_boxes][h][w]; posterior: float or NULL;
 * conf_score: [max_boxes] = mean over the frame of (2p-1 inside the mask, 1-2p outside), fixed-order reduction. */
int64_t premvos_refine_output_workspace_bytes(int32_t max_boxes, int32_t size, int32_t h, int32_t w);
int premvos_refine_output_f32(const float* logits, int32_t logits_ps, int32_t lh, int32_t lw, const int32_t* crop_boxes,
                              const int32_t* count, int32_t max_boxes, int32_t size, int32_t h, int32_t w,
                              uint8_t* mask, float* posterior, float* conf_score, void* workspace, void* stream);

/* Test-time augmentation of the refinement net: DeepLab's multi-scale / flipped inference
 * (network/deeplab/model.py:84-160 predict_labels_multi_scale, scale handling model.py:200-325).
 *
 * Member inputs of ONE scale.  net_in: the plain network input [boxes][size][size][4] (premvos_refine_input_u8's output) ->
 * out [boxes][out_size][out_size][4], its align_corners=True bilinear resize (model.py:272-277), all four channels; with flip = 1
 * immediately followed by a second [boxes][out_size][out_size][4], the same crops reversed along the width
 * (tf.reverse_v2(images, [2]), model.py:118).  out_size = scale_dimension(size, scale); out_size == size: a copy (+ a mirrored copy). */
int premvos_refine_tta_input_f32(const float* net_in, int32_t boxes, int32_t size, float* out, int32_t out_size, int32_t flip,
                                 void* stream);

/* The members' logits, passed by value: member m is [max_boxes][size[m]][size[m]][pixel_stride[m] >= 2] floats, already on the grid
 * L = scale_dimension(crop size, max(1, scale) / 4) of model.py:258-297 (a smaller native grid is brought there first:
 * premvos_resize_bilinear_f32, align_corners = 1); mirrored[m] = 1: the logits of a mirrored input, NOT yet reversed. */
#define PREMVOS_TTA_MAX_MEMBERS 12
typedef struct premvos_tta_members {
  int32_t count;                                   /* 1 .. PREMVOS_TTA_MAX_MEMBERS */
  int32_t size[PREMVOS_TTA_MAX_MEMBERS];
  int32_t pixel_stride[PREMVOS_TTA_MAX_MEMBERS];
  int32_t mirrored[PREMVOS_TTA_MAX_MEMBERS];
  const float* logits[PREMVOS_TTA_MAX_MEMBERS];
} premvos_tta_members;

/* premvos_refine_output_f32 over several members: per pixel of [max_boxes][size][size], in member order, a mirrored member's
 * logits reversed along the width (model.py:137), the output layer's own legacy-bilinear resize to size^2
 * (SegmentationOutputLayers.py:35-61 -- not predict_labels_multi_scale's align-corners one: the layer the weights were trained under),
 * two-class softmax; prob = the mean of p1 and class 1 where mean p1 > mean p0 (model.py:143-147; a tie -> 0, like tf.argmax), fp32
 * sums in member order.  Un-crop, zero padding and conf_score as premvos_refine_output_f32, whose workspace
 * (premvos_refine_output_workspace_bytes) and outputs it shares.  One unmirrored member: premvos_refine_output_f32 itself, bit for bit. */
int premvos_refine_tta_output_f32(premvos_tta_members members, const int32_t* crop_boxes, const int32_t* count, int32_t max_boxes,
                                  int32_t size, int32_t h, int32_t w, uint8_t* mask, float* posterior, float* conf_score,
                                  void* workspace, void* stream);

/* Calibration kernel: `blocks` workgroups of 4 waves each issue iters*16 independent v_mfma_f32_32x32x2_f32 per wave
 * (FLOPs = blocks*4*iters*16*4096); timing it gives the fp32 MFMA rate the GPU sustains under its own power management
 * (bench.py: roofline.mfma_ceiling_measured). */
int premvos_mfma_f32_calibrate(int64_t iters, int32_t blocks, float* sink, void* stream);

/* The same loop on CHANGING pseudo-random operands (eight A and B registers per lane, another pair for every MFMA): the fp32 matrix
 * pipe's power follows the switching activity of its operands, and on random data the socket meets its cap and the shader clock gives
 * way (the constant operands above never do).  Timed over >= 1 s: the fp32 MFMA rate a box sustains on real data
 * (bench.py: roofline.mfma_ceiling_sustained_random_data). */
int premvos_mfma_f32_calibrate_random(int64_t iters, int32_t blocks, float* sink, void* stream);

/* Calibration kernel: copies n_float4 16-byte words src -> dst (one word per thread, flat grid);
 * 2 * 16 * n_float4 bytes / time = the streaming HBM rate the GPU sustains (bench.py: roofline.hbm_ceiling_measured).  Use
 * buffers well beyond the 256 MB Infinity Cache. */
int premvos_hbm_copy_calibrate(const void* src, void* dst, int64_t n_float4, void* stream);

/* Order-independent 64-bit digest of the 4-byte words of a pixel-major window [pixels][c] with pixel stride ps (words): the plan-time
 * tuner compares the outputs of configurations that must be bit-identical (same numerics key) before it lets a stopwatch choose
 * between them (premvos_amd/ops.py::_time_cands).  *out_u64 (device) receives the digest. */
int premvos_digest_u64(const void* buf, int64_t pixels, int32_t c, int32_t ps, void* out_u64, void* stream);

/* Host-side utility (no GPU work): CRC-32C of a host buffer -- the checksum of TensorFlow tensor-bundle checkpoints,
 * which premvos_amd/weights.py reads and writes without TensorFlow (proposal_net/train.py:655, core/Saver.py:33-48). */
uint32_t premvos_crc32c_host(const void* data, int64_t n);

/* ------------------------------------------------------------------------------------------
 * Optional GPU JPEG decode.  Replaces the image readers of the stages -- cv2.imread
 * (proposal_net/train.py:500, BGR), scipy.ndimage.imread / PIL (optical_flow_net-PWC-Net/script_pwc_multi.py:34,
 * ReID_net/prepare_input.py:38, RGB) -- i.e. libjpeg(-turbo) with its defaults: JDCT_ISLOW, fancy up-sampling, YCbCr -> RGB.
 * Baseline / extended-sequential Huffman files, 8 bit, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart
 * intervals; anything else returns PREMVOS_EUNSUPPORTED and the caller keeps its default reader.  The output is the
 * library's, byte for byte.
 * ---------------------------------------------------------------------------------------- */
typedef struct premvos_jpeg_info {
  int32_t width, height, ncomp;  /* ncomp 1 (grey) or 3 (YCbCr) */
  int32_t hs, vs;                /* luma samples per chroma sample: 1x1, 2x1 or 2x2 (1x1 for grey) */
  int32_t mcux, mcuy;            /* MCU grid: ceil(width / (8 hs)) x ceil(height / (8 vs)) */
  int32_t blocks_w[3], blocks_h[3];
  int32_t reserved;
  int64_t coef_offset[3];        /* int16 elements: component c holds [blocks_h][blocks_w][64] quantised coefficients, row-major */
  int64_t coef_count;            /* total int16 elements */
  uint16_t quant[3][64];         /* quantisation table of each component, row-major (de-zig-zagged) */
} premvos_jpeg_info;

/* HOST function, no GPU work: marker parsing + Huffman decoding (ITU-T T.81 F.2).  coef == NULL: header only (fills *info).
 * Otherwise coef (host memory, any alignment; pinned for an asynchronous upload) receives info->coef_count values. */
int premvos_jpeg_entropy_decode_host(const uint8_t* data, int64_t n, premvos_jpeg_info* info, int16_t* coef,
                                     int64_t coef_capacity);
/* bytes of the device workspace (the component planes between the two kernels) */
int64_t premvos_jpeg_workspace_bytes(const premvos_jpeg_info* info);
/* coef: DEVICE copy of the coefficients (16-byte aligned); info: the host struct; out: uint8 [height][width][3],
 * RGB (bgr = 0) or BGR (bgr != 0, what cv2.imread returns).  De-quantisation + jidctint.c inverse DCT, then
 * jdsample.c fancy up-sampling fused with jdcolor.c's colour conversion. */
int premvos_jpeg_reconstruct_u8(const int16_t* coef, const premvos_jpeg_info* info, void* workspace, uint8_t* out,
                                int32_t bgr, void* stream);

/* ------------------------------------------------------------------------------------------
 * GPU baseline JPEG encode, the mirror image of the decoder above, and the overlay picture it was built for: the reference's
 * MergeTrack/merge_functions.py:527-545 (draw_mask + save_jpg) shows a result as the frame with every object's mask tinted.
 * The frame and the id map the merge loop painted are in HBM; the picture leaves the device as quantised coefficients.
 * The file is the one libjpeg(-turbo) writes with its defaults for the same pixels (what PIL's Image.save produces; cv2, which
 * save_jpg calls, is the same library behind another header), byte for byte.
 * ---------------------------------------------------------------------------------------- */
/* merge_functions.py:527-539 draw_mask with alpha 0.5 for all objects at once: out = (frame + palette[id]) >> 1 per channel where
 * idmap > 0 (im * (1 - 0.5) + colour * 0.5, then astype(uint8): the truncation is the shift), the frame's pixel elsewhere.
 * frame, out: uint8 [h][w][3]; idmap: uint8 [h][w]; palette: uint8 [256][3] (the DAVIS palette of the PNGs); all DEVICE memory. */
int premvos_overlay_blend_u8(const uint8_t* frame, const uint8_t* idmap, const uint8_t* palette, int32_t h, int32_t w,
                             uint8_t* out, void* stream);
/* Pixels -> quantised coefficients.  rgb: DEVICE uint8 [h][w][3].  idmap / palette: both NULL, or DEVICE buffers as above -- the
 * blend of premvos_overlay_blend_u8 is then applied while the pixels are loaded (the blended picture is never stored).
 * quant_luma / quant_chroma: HOST, 64 values 1 ... 255 in natural (row-major) order.  hs x vs: 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0).
 * *info (HOST) is filled with the geometry and tables; coef == NULL: that is all (the caller sizes its buffer by info->coef_count).
 * Otherwise coef (DEVICE, 16-byte aligned) receives the layout premvos_jpeg_entropy_decode_host produces, dummy blocks included.
 * Restates jccolor.c rgb_ycc_convert, jcprepct.c expand_bottom_edge, jcsample.c expand_right_edge / h2v1_downsample /
 * h2v2_downsample, jfdctint.c jpeg_fdct_islow, jcdctmgr.c quantize and jccoefct.c compress_data (dummy blocks of an edge MCU). */
int premvos_jpeg_forward_u8(const uint8_t* rgb, const uint8_t* idmap, const uint8_t* palette, int32_t h, int32_t w,
                            const uint16_t* quant_luma, const uint16_t* quant_chroma, int32_t hs, int32_t vs,
                            premvos_jpeg_info* info, int16_t* coef, int64_t coef_capacity, void* stream);
/* HOST function, no GPU work: coefficients (host memory) + the info block premvos_jpeg_forward_u8 filled -> a complete JFIF file in
 * out[0 .. *written).  jcmarker.c write_file_header / write_frame_header / write_scan_header (SOI, JFIF 1.01 APP0, two DQT, SOF0,
 * the four T.81 annex K.3 DHT, SOS) and jchuff.c encode_one_block (standard tables, 0xFF00 stuffing, 1-bit padding), EOI.
 * A file that does not fit in `capacity` bytes returns PREMVOS_ENOSPACE; nothing is ever written at or behind out + capacity. */
int premvos_jpeg_entropy_encode_host(const int16_t* coef, const premvos_jpeg_info* info, uint8_t* out, int64_t capacity,
                                     int64_t* written);

/* ------------------------------------------------------------------------------------------
 * ReID embedding net (code/ReID_net).  Its convs / FC layers go through premvos_conv2d_f32, the pool
 * through premvos_maxpool_f32.
 * ---------------------------------------------------------------------------------------- */
/* datasets/Similarity/DAVIS_Forward_Feed.py:62-96 (zero_small = 1: boxes with min(w,h) <= 10 give a zero image) and
 * Similarity.py:288-297 (zero_small = 0): frame uint8 RGB [h][w][3] / 255, crop boxes_xywh[i] (int32 x, y, w, h; already
 * context-expanded, rounded and clipped by the host), tf.image.resize_images bilinear (TF1 legacy) to size x size,
 * (x - mean) / std -> NHWC [n][size][size][4] (4th channel 0). */
int premvos_reid_input_u8(const uint8_t* frame_rgb, int32_t h, int32_t w, const int32_t* boxes_xywh, int32_t n,
                          int32_t size, int32_t zero_small, float* out, void* stream);
/* The same crops for slots of SEVERAL frames in one launch (the streaming driver's ReID stage: the refined proposals of a
 * group of frames are one batch): frames_rgb uint8 [nframes][h][w][3], slot i is cut from frame frame_of_slot[i] (device int32
 * [n]; clamped to [0, nframes)) with boxes_xywh[i] (device) -> out [n][size][size][4], bit for bit what premvos_reid_input_u8
 * writes for that (frame, box) pair (datasets/Similarity/Similarity.py:264-298; DAVIS_Forward_Feed.py:62-96). */
int premvos_reid_input_frames_u8(const uint8_t* frames_rgb, int32_t nframes, int32_t h, int32_t w,
                                 const int32_t* frame_of_slot, const int32_t* boxes_xywh, int32_t n, int32_t size,
                                 int32_t zero_small, float* out, void* stream);
/* The context region of boxes that are already in device memory (datasets/Similarity/Similarity.py:264-298 with feed = 0,
 * DAVIS_Forward_Feed.py:36-60 with feed != 0: an excess of at least one pixel): int32 boxes_xywh [n][4] -> int32 out [n][4], x1.2
 * around the centre in float32 with every product and difference rounded on its own (no fused multiply-add: the tf.round ties
 * are real, e.g. x = 10, w = 5), tf.round (half to even), clip to height x width.  Both arrays 16-byte aligned. */
int premvos_reid_context_boxes_i32(const int32_t* boxes_xywh, int32_t n, int32_t height, int32_t width, int32_t feed,
                                   int32_t* out, void* stream);
/* maskApi.c rleToBbox of n uint8 masks (nonzero = foreground) WITHOUT their run lengths: what
 * ReID_net/Forwarding/ReIDForwarding.py:68-74 computes per proposal from the RLE string ("w > 0 and h > 0" decides whether a
 * proposal gets an embedding), from the masks the refinement stage left in HBM.  Mask i = the h x w top-left window of
 * masks + i*mask_stride with row_stride bytes between rows (as premvos_rle_boundaries_pooled_u8).  bbox_xywh int32 [n][4] =
 * (x, y, w, h): the columns and rows that hold foreground -- except that, as in rleToBbox, one foreground run that crosses a
 * column boundary (mask[h-1][x] and mask[0][x+1] both set) gives y = 0 and the full height; an empty mask gives 0 0 0 0.
 * context_xywh (may be NULL): premvos_reid_context_boxes_i32 of those boxes with height = h, width = w, in the same launches.
 * workspace: int32 [n][PREMVOS_MASK_BBOX_SLABS][4].  No atomics: two launches give the same bits.  n <= 65535. */
#define PREMVOS_MASK_BBOX_SLABS 16
int premvos_mask_bbox_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, int64_t mask_stride, int32_t row_stride,
                         int32_t feed, int32_t* bbox_xywh, int32_t* context_xywh, int32_t* workspace, void* stream);

/* Inference BatchNorm (+ ReLU when relu != 0) as a per-channel scale / shift over NHWC pixels, for pre-activation units
 * whose input is also consumed raw by the identity shortcut (network/NetworkLayers.py:171-173). */
int premvos_scale_shift_relu_f32(const float* in, int32_t in_ps, int64_t npix, int32_t c, const float* scale,
                                 const float* shift, float* out, int32_t out_ps, int32_t relu, void* stream);

/* ------------------------------------------------------------------------------------------
 * MergeTrack-side mask helpers (the consumer of the hot path).  Masks are uint8 [n][h][w] row-major,
 * nonzero = foreground, resident in HBM.
 * ---------------------------------------------------------------------------------------- */
/* MergeTrack/merge_functions.py:209-217 warp_flow: out = cv2.remap(mask, grid - flow, INTER_LINEAR) (uint8 fixed-point
 * path, zero border), then (== 1) when binarize != 0.  flow: float [h][w][2] = (u, v) as in the .flo payload. */
int premvos_mask_warp_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, const float* flow, uint8_t* out,
                         int32_t binarize, void* stream);
/* The same warp (merge_functions.py:209-217, the same fixed-point arithmetic) for the masks of up to 8 videos in ONE launch: mask i
 * moves by flows[flow_of_mask[i]].  flow_of_mask int32 [n] is a DEVICE pointer; flows: float [V][h][w][2]; a mask whose entry is
 * outside [0, V) is not written.  1 <= V <= 8.  Equals V calls of premvos_mask_warp_u8 on the masks of each flow. */
int premvos_mask_warp_seats_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, const int32_t* flow_of_mask, const float* flows,
                               int32_t V, uint8_t* out, int32_t binarize, void* stream);

/* merge_functions.py:38-45 (pycocotools iou on the proposals' RLEs): pixel counts of every pair --
 * inter[ib*na + ia] = |a_ia AND b_ib|, area_a[ia], area_b[ib]; the caller forms i/u in double (u = 1 when i == 0). */
int premvos_mask_overlap_u8(const uint8_t* a, int32_t na, const uint8_t* b, int32_t nb, int64_t hw, int64_t* inter,
                            int64_t* area_a, int64_t* area_b, void* stream);

/* merge_functions.py:224-226 (pycocotools encode of the Fortran-ordered mask): ascending column-major positions
 * q = x*h + y at which the value changes (value before q = 0 is background) -> positions[i*capacity ..], nruns[i] =
 * number of changes (may exceed capacity: then only the first `capacity` are stored).  COCO counts = successive
 * differences of [0, positions..., h*w]. */
int64_t premvos_rle_workspace_bytes(int32_t n, int32_t h, int32_t w);
int premvos_rle_boundaries_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, int32_t* positions,
                              int32_t capacity, int32_t* nruns, void* workspace, void* stream);
/* The same boundaries for the n masks of a CHUNK of frames, POOLED: mask i's ascending positions go to
 * pool[offsets[i] .. offsets[i+1]) with offsets[0] = 0 -- one variable-length stream instead of n fixed-capacity rows, so that a
 * rank can hand the merge rank run lengths instead of masks (the RLE strings FewShotSegmentationForwarder.py:140-142 builds per
 * box are then pure host work on a few integers per run).  Mask i = the h x w top-left window of masks + i*mask_stride with
 * row_stride bytes between rows (masks inside a larger staging block).  offsets[n] = the total number of boundaries; it may exceed
 * pool_capacity: then only the entries below pool_capacity were stored and the caller falls back to the masks themselves.
 * workspace: premvos_rle_workspace_bytes(n, h, w). */
int premvos_rle_boundaries_pooled_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, int64_t mask_stride,
                                     int32_t row_stride, int32_t* pool, int32_t pool_capacity, int32_t* offsets,
                                     void* workspace, void* stream);

/* Masks on the wire (ONE gather of fixed-size buffers per chunk to the merge rank, masks bit-packed): n mask
 * bytes (nonzero = foreground) -> ceil(n/8) bytes, bit k of byte i = masks[8i + k] != 0; and back to {0,1} bytes.  Replaces the
 * reference's hand-over through per-frame JSON files (refinement_net/forwarding/FewShotSegmentationForwarder.py:151-155 read
 * back by MergeTrack/merge_functions.py:38-76). */
int premvos_mask_pack_bits_u8(const uint8_t* masks, int64_t n, uint8_t* bits, void* stream);
int premvos_mask_unpack_bits_u8(const uint8_t* bits, int64_t n, uint8_t* masks, void* stream);

/* Host-side utility (no GPU work): COCO rleToString of `n` run lengths into `out` (capacity `cap` bytes); returns the
 * length or -1 -- the "counts" string of every mask the refinement / merge stages write
 * (forwarding/FewShotSegmentationForwarder.py:141-142). */
int64_t premvos_rle_counts_to_string_host(const int64_t* counts, int64_t n, char* out, int64_t cap);
/* Host-side utility (no GPU work): the "counts" strings of n masks from their pooled boundaries (host copies of `pool` /
 * `offsets` above; hw = h*w), written back to back into `out`; string i = out[str_offsets[i] .. str_offsets[i+1]).  Returns the
 * total length or -1 when `cap` is too small (13 bytes per run always suffice). */
int64_t premvos_rle_strings_host(const int32_t* pool, const int32_t* offsets, int32_t n, int64_t hw, char* out, int64_t cap,
                                 int64_t* str_offsets);

/* ------------------------------------------------------------------------------------------
 * The merge loop itself (MergeTrack/merge.py:69-115 do_video; premvos_amd/csrc/track_ops.hip, premvos_amd/track.py).  One launch
 * each; the selection stays in device memory between the second and the third.
 * ---------------------------------------------------------------------------------------- */
/* The inverse of premvos_rle_boundaries_pooled_u8 (pycocotools decode, merge_functions.py:125): mask i's ascending column-major
 * boundaries pool[offsets[i] .. offsets[i+1]) -> out[i][h][w], 1 where the number of boundaries <= x*h + y is odd, else 0.
 * Offsets are clamped to [0, pool_len].  n = 0 is a no-op. */
int premvos_rle_decode_u8(const int32_t* pool, int32_t pool_len, const int32_t* offsets, int32_t n, int32_t h, int32_t w,
                          uint8_t* out, void* stream);

/* merge_functions.py:38-76 calculate_scores + merge.py:89-90 (the two np.dot) + merge_functions.py:96-121 (threshold column, non-finite
 * -> 0, argmax) for T templates and P proposals, float64 like the reference, sums in a fixed order (no atomics).
 *   inter [T][P], area_p [P], area_t [T]   as premvos_mask_overlap_u8(a = proposals, b = templates) writes them
 *   template_score [T], proposal_score [P] the 'score' entries;  emb_p [P][128], emb_t [T][128] the 'ReID' entries (+inf = none)
 *   weights5                               HOST pointer: the five normalised weights (mask, ReID, other ReID, warp, other warp)
 *   planes [5][T][P]; weighted [T][P+1] (last column = score_thresh); selected [T] (first maximum; P = the empty proposal);
 *   final_score [T] (that maximum); object_score [T] (max over the row of plane 0 + plane 1, as the reference takes it)
 * T <= 255, P <= 65535. */
int premvos_track_scores_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_t, const double* template_score,
                             const double* proposal_score, const double* emb_p, const double* emb_t, int32_t T, int32_t P,
                             const double* weights5, double score_thresh, double* planes, double* weighted, int32_t* selected,
                             double* final_score, double* object_score, void* stream);

/* merge_functions.py:123-149 remove_mask_overlap + 516-525 save_pngs in one pass: object t covers the pixels of
 * masks[selected[t]] (nonzero = foreground; selected[t] == P: nothing); a pixel goes to the covering object with the largest
 * (final_score, t).  labels [h][w] = 1 + that t (0: none), idmap [h][w] = ids[t] (what the PNG holds), refined [T][h][w] =
 * (labels == t + 1).  selected / final_score / ids are DEVICE pointers.  T <= 255. */
int premvos_track_paint_u8(const uint8_t* masks, int32_t P, int32_t h, int32_t w, const int32_t* selected,
                           const double* final_score, const int32_t* ids, int32_t T, uint8_t* labels, uint8_t* idmap,
                           uint8_t* refined, void* stream);

/* The proposal side of premvos_track_scores_f64 for P = T + F, for a caller whose fresh proposals are in device memory
 * (premvos_amd.stream --track): proposal_score [P] = cand_score [T] then fresh_score [F]; emb_p [P][128] = cand_emb [T][128] then the
 * fresh rows widened from float32.  fresh_rows [F][132] float32 = 128 embedding values + the mask's rleToBbox box (x, y, w, h) as int32
 * bits (what ReIDNet.embed_masks packs); a row whose box has w <= 0 or h <= 0 becomes +inf x 128 -- the proposal without a "ReID" key
 * of merge_functions.py:27-36 read_props (ReIDForwarding.py:68-74 wrote none).  Replaces merge.py:84 (next_props + read_props(...))
 * and the list comprehensions of merge_functions.py:46-52.  All pointers are DEVICE pointers; cand_* may be NULL when T = 0, fresh_*
 * when F = 0.  T <= 255, T + F <= 65535. */
int premvos_track_inputs_f64(const double* cand_score, const double* cand_emb, const double* fresh_score, const float* fresh_rows,
                             int32_t T, int32_t F, double* proposal_score, double* emb_p, void* stream);

/* merge_functions.py:234 for T warped candidates: cand_score [T] = 0.5 * (final_score + 1) (float64, the sum first), and the boxes
 * refinement_net_functions.py:38-64 crops by, from the warped masks' boxes bbox_xywh [T][4] int32 (x, y, w, h):
 * boxes_y0x0y1x1 [T][4] float32 = (y, x, y + h, x + w).  DEVICE pointers. */
int premvos_track_next_f32(const double* final_score, const int32_t* bbox_xywh, int32_t T, double* cand_score,
                           float* boxes_y0x0y1x1, void* stream);

/* ---- The two swaps merge.py imports next to its loop's functions (merge.py:50-52; premvos_amd/csrc/merge_modes_ops.hip): the oracle
 * merge and the probabilistic combination.  Opt-in (Tracker(combine=..., oracle=...)); float64, fixed summation order, integer atomics
 * only.  Refused (-1, before any HIP call): null pointers, non-positive dimensions, T > 255. */
/* The counts of merge_functions.py:78-94 calculate_gt_scores (pycocotools iou of every candidate with every object's annotation) in
 * ONE pass: masks uint8 [P][hw] (nonzero = foreground) against the frame's label map labels uint8 [hw] (the annotation PNG's ids):
 *   inter [T][P] = |mask_p and (labels == t + 1)|,  area_p [P] = |mask_p|,  area_l [T] = |labels == t + 1|      (int64)
 * Labels 0 and labels above T do not count.  Every mask byte and the label map are read once per candidate; a workgroup counts into
 * an LDS histogram over the labels, then adds with integer atomics.  The three outputs are zeroed by the call, on `stream`. */
int premvos_mask_label_overlap_u8(const uint8_t* masks, int32_t P, const uint8_t* labels, int32_t T, int64_t hw, int64_t* inter,
                                  int64_t* area_p, int64_t* area_l, void* stream);

/* merge_functions.py:78-94 calculate_gt_scores from those counts, then what premvos_track_scores_f64 does with its planes (merge.py:89-90,
 * merge_functions.py:96-121), with the same outputs: planes [5][T][P], all five = the IoU (0 where the intersection is empty: an object
 * the annotation lacks scores 0 everywhere); weighted [T][P+1] = the weighted sum in plane order, last column = score_thresh,
 * non-finite -> 0; selected / final_score / object_score by the same selection pass (csrc/track_select.h).  weights5: HOST pointer.
 * T <= 255, P <= 65535. */
int premvos_track_gt_scores_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_l, int32_t T, int32_t P,
                                const double* weights5, double score_thresh, double* planes, double* weighted, int32_t* selected,
                                double* final_score, double* object_score, void* stream);

/* merge_functions.py:151-195 probabilitic_combination, in place of calculate_selected_props + remove_mask_overlap; two launches.
 *   weighted [T] rows of weighted_stride doubles, the first P of each are used (P + 1 skips premvos_track_scores_f64's threshold
 *   column); a non-finite score counts as 0
 *   probs [T][P] = exp(ws / 0.1) / sum_p exp(ws / 0.1), p ascending, no maximum subtracted;  denom [T] = sum_p probs (workspace the
 *   second launch reads);  final_score [T] = the row's maximum
 *   per pixel: combined[t] = (sum over p ascending of probs[t][p] where masks[p] is nonzero) / denom[t]; background = 1 - max_t
 *   combined[t]; labels [h][w] = the first maximum of [background, combined[0 .. T)] (0 = background: it wins a tie), idmap = ids[t]
 *   of it, refined [T][h][w] = (labels == t + 1): the three outputs of premvos_track_paint_u8.
 * The reference's second softmax is monotone; the argmax is taken of its input.  masks uint8 [P][h][w]; ids: DEVICE int32 [T].
 * T <= 255, any P (beyond 1024 candidates the tile's mask bits are staged in LDS chunk by chunk). */
int premvos_track_combine_f64(const uint8_t* masks, int32_t P, int32_t h, int32_t w, const double* weighted, int64_t weighted_stride,
                              const int32_t* ids, int32_t T, double* probs, double* denom, double* final_score, uint8_t* labels,
                              uint8_t* idmap, uint8_t* refined, void* stream);

/* merge_functions.py:547-611 viz_scores: one frame's score sheet, uint8 [100 (T + 1)][100 P][3], AFTER scipy.misc.imsave's bytescale
 * (the bytes its JPEG is coded from); two launches on `stream`, nothing returns to the host in between (csrc/viz_ops.hip).
 *   frame uint8 [h][w][3];  masks uint8 [P][h][w] (nonzero = foreground);  boxes double [P][4] = x, y, w, h, truncated toward zero
 *   planes double [5][T][P];  weighted [T] rows of weighted_stride doubles, the first P of each are used;  gt double [T][P]
 *   tint3: HOST pointer to the three bytes draw_mask adds to channels 0, 1, 2 (its PALETTE_RGB[2][::-1])
 * Top row, tile j: with min(h, w) >= 2 the crop frame[y : y + h - 1, x : x + w - 1], clipped to the frame, resized to 100 x 100 by
 * cv2's fixed-point INTER_LINEAR (csrc/resize_cv.h), the mask's crop likewise; where the resized mask is > 0 the pixel is
 * (uint8)(im * 0.7 + tint * 0.3); else (and for a crop that is empty after clipping) a black tile.  Row i + 1, tile j: the five planes
 * as cells of 20 x 50 in the left half, colour ((1 - s) * 255, s * 255, 0); the weighted score top right, gt bottom right; column 0 and
 * row 0 of every tile are zero; two black 25 x 25 marks per row, in the weighted cell of the row's first maximum over the P
 * candidates and in the gt cell of gt's.  A non-finite weighted score counts as 0 (for the marks, a non-finite gt too); a non-finite
 * plane or gt value is written as 0 and does not enter the extremes.
 * bytescale: cmin / cmax = the extremes of the whole float canvas, found on the device without atomics; scale = 255 / (cmax - cmin),
 * a zero range counting as 1; out = (uint8)(clip((v - cmin) * scale, 0, 255) + 0.5).
 * workspace: device memory, 8-byte aligned, 16 (P + 1) + 8 T bytes.  1 <= T <= 255, P >= 1, 100 P <= 65535, sheet pixels <= 64 Mi. */
int premvos_viz_scores_u8(const uint8_t* frame, int32_t h, int32_t w, const uint8_t* masks, const double* boxes, int32_t P,
                          const double* planes, const double* weighted, int64_t weighted_stride, const double* gt, int32_t T,
                          const uint8_t* tint3, void* workspace, int64_t workspace_bytes, uint8_t* sheet, void* stream);

/* MergeTrack/print_max_reid_distance.py:40-48 for one video: max_distance [T] = per template the largest norm(c - t) over the video's
 * pooled proposal embeddings proposals double [N][128] (templates double [T][128]); the squares are summed over the embedding index
 * ascending; an infinite distance (a proposal without 'ReID': all inf) counts as 0; the maximum starts at 0 (N = 0, or a frame without
 * proposals) and a NaN wins it.  over [T] (may be NULL): how many distances exceed MAX_REID_DISTANCE = 25 (merge_functions.py:12).
 * One launch; integer sums and an ordered maximum only.  T <= 65535. */
int premvos_reid_max_distance_f64(const double* templates, int32_t T, const double* proposals, int64_t N, double* max_distance,
                                  int64_t* over, void* stream);

/* ---- The same loop for up to 8 videos in lockstep (premvos_amd.track.TrackerGroup): one launch serves every video's frame.
 * A SEAT is one of V places (1 <= V <= 8) that holds one video or is empty.  The seat table is a HOST pointer to
 *   int32_t seats[V][4] = { T, F, cand_slot, fresh_slot }
 * read during the call and passed to the kernel by value (no upload, no synchronisation).  T = the seat's objects (templates),
 * F = its fresh proposals, P = T + F.  The seat's proposal p < T (a carried candidate; the first T are also its templates' masks) is
 * mask cand_slot + p of ONE pool masks uint8 [S][h][w]; proposal p >= T is mask fresh_slot + p - T.  T = 0: the seat is empty -- its
 * other three entries are ignored (F counts as 0), it costs nothing and nothing is written for it.
 * Every pooled array holds the seats' slices back to back in seat order.  With sums over the seats u < v:
 *   per template  [sum T_u]            area_t, cand_score, selected, final_score, object_score, ids;  x 128: cand_emb, templ_emb
 *   per fresh row [sum F_u]            fresh_score;  x 128: fresh_emb
 *   per proposal  [sum P_u]            area_p
 *   inter  [T_v][P_v]          at      sum T_u * P_u
 *   planes [5][T_v][P_v]       at  5 * sum T_u * P_u
 *   weighted [T_v][P_v + 1]    at      sum T_u * P_u + sum T_u
 *   labels, idmap [h][w]       at      v * h * w   (the planes of empty seats stay as they were)
 * Refused (-1, before any HIP call): null pointers, V outside 1..8, T > 255, P > 65535, negative counts or slots, slots beyond S. */

/* merge_functions.py:38-45 per seat: what premvos_mask_overlap_u8(a = the seat's P proposals, b = its T templates) writes, for the pairs
 * of each seat only (on the pooled masks that entry would count every cross-video pair). */
int premvos_mask_overlap_seats_u8(const uint8_t* masks, int32_t S, int64_t hw, const int32_t* seats, int32_t V, int64_t* inter,
                                  int64_t* area_p, int64_t* area_t, void* stream);

/* merge_functions.py:38-76 + merge.py:89-90 + merge_functions.py:96-121 per seat, one workgroup each: premvos_track_scores_f64's
 * arithmetic in the same fixed order with template_score = the seat's cand_score (Tracker.step: the templates' scores are the warped
 * candidates'), emb_t = its templ_emb rows, and the proposal side = its cand_score / cand_emb rows, then its fresh_score / fresh_emb
 * rows (merge.py:84 next_props + read_props(...), read in place).  fresh_* may be NULL when no seat has fresh rows.  selected is
 * seat-local: P_v = the empty proposal.  All float64; weights5 is a HOST pointer. */
int premvos_track_scores_seats_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_t, const double* cand_score,
                                   const double* cand_emb, const double* templ_emb, const double* fresh_score, const double* fresh_emb,
                                   const int32_t* seats, int32_t V, const double* weights5, double score_thresh, double* planes,
                                   double* weighted, int32_t* selected, double* final_score, double* object_score, void* stream);

/* merge_functions.py:123-149 + 516-525 per seat: premvos_track_paint_u8 (the same order, the same tie rule) with the seat's selections
 * taken from the pool through the seat table.  labels, idmap: uint8 [V][h][w]; the (labels == t + 1) plane of the seat's template t
 * goes to plane refined_slots[v] + t of refined uint8 [R][h][w] (refined_slots: HOST int32 [V], e.g. the seat's candidate slots of a
 * second pool).  selected / final_score / ids are DEVICE pointers, pooled per template. */
int premvos_track_paint_seats_u8(const uint8_t* masks, int32_t S, int32_t h, int32_t w, const int32_t* seats, int32_t V,
                                 const int32_t* selected, const double* final_score, const int32_t* ids, uint8_t* labels, uint8_t* idmap,
                                 uint8_t* refined, int32_t R, const int32_t* refined_slots, void* stream);

/* ---- The weight search of the live loop (premvos_amd.track.SearchGroup): the V seats hold ONE video under V weight sets, what
 * MergeTrack/oldmerge.py:225-227,253-255 does one full run per np.random.random_sample(5) at a time.
 * premvos_track_scores_seats_f64 with two differences: weights is a HOST pointer to double [V][5] (row v: seat v's merge.py:119 weights,
 * normalised by the caller), passed to the kernel by value like the seat table; and every occupied seat's proposal side is its own T
 * cand_score / cand_emb rows followed by the SAME F fresh rows -- fresh_score [F], fresh_emb [F][128], no per-seat offset (merge.py:84
 * next_props + read_props(...): the file is one, the candidates are the seat's).  Every occupied seat must carry that F in the table
 * (refused otherwise); the outputs are laid out as the seat table says.  One workgroup per seat, the same device function as
 * premvos_track_scores_f64 (merge_functions.py:38-76, merge.py:89-90, merge_functions.py:96-121): the same fixed order, no atomics. */
int premvos_track_scores_sets_f64(const int64_t* inter, const int64_t* area_p, const int64_t* area_t, const double* cand_score,
                                  const double* cand_emb, const double* templ_emb, const double* fresh_score, const double* fresh_emb,
                                  const int32_t* seats, int32_t V, const double* weights, double score_thresh, double* planes,
                                  double* weighted, int32_t* selected, double* final_score, double* object_score, void* stream);

/* merge_functions.py:613-634 eval_video's pixel work as integer counts, for all seats of one frame: planes uint8 [R][h][w] is what
 * premvos_track_paint_seats_u8 wrote as `refined` (plane first_plane[v] + k = seat v's object k after overlap removal; nonzero =
 * foreground; first_plane: HOST int32 [V]); gt uint8 [h][w] is the frame's annotation id map, read once for all seats.
 * counts[v * seat_stride + 3 k + {0, 1, 2}] += |R and G|, |R or G|, |R| with G = (gt == k + 1), k < T0: the caller's slice [t] of an
 * int64 [V][N][T0][3] tensor with seat_stride = N * T0 * 3, zeroed by the caller once per video (the entry only ADDS).  Wave-reduced
 * popcounts and one integer atomic per count and workgroup: two calls on zeroed counts give the same bits.  T0 <= 255; T0 = 0 is a no-op. */
int premvos_track_eval_seats_i64(const uint8_t* planes, int32_t R, int32_t h, int32_t w, const uint8_t* gt, int32_t V, int32_t T0,
                                 const int32_t* first_plane, int64_t* counts, int64_t seat_stride, void* stream);

/* ------------------------------------------------------------------------------------------
 * The DAVIS-2017 measures' pixel work (tools/davis_eval.py:25-71 db_eval_iou, seg2bmap, _disk, db_eval_boundary;
 * premvos_amd/csrc/davis_ops.hip, premvos_amd/evaluate.py).  Integers only: the floats J and F follow from the counts on the host.
 * ---------------------------------------------------------------------------------------- */
/* counts[n][t][6] int64 = { |R&G|, |R|G|, |bR|, |bG|, |bR & dil(bG)|, |bG & dil(bR)| } for object ids[t]:
 * R = (result == id), G = (gt == id), b = seg2bmap (tools/davis_eval.py:33-47: east, south or south-east neighbour differs; the last
 * row / column compare with themselves), dil = binary dilation by the disk dx*dx + dy*dy <= radius*radius (tools/davis_eval.py:50-60)
 * with background outside the image.  maps: null, or uint8 [n][T][4][h][w] = bR, bG, bR & dil(bG), bG & dil(bR) as 0 / 1.
 * result, gt: [n][h][w] id maps, ids: [T], all DEVICE pointers; counts (and maps) are zeroed by the call, on `stream`.  An id in
 * neither map gives six zeros; ids of the maps that are not in `ids` are ignored.  T <= 255, 1 <= radius <= 48 (a 4K frame's is 36);
 * n = 0 or T = 0 is a no-op. */
int premvos_davis_counts_u8(const uint8_t* result, const uint8_t* gt, int32_t n, int32_t h, int32_t w, const int32_t* ids,
                            int32_t T, int32_t radius, int64_t* counts, uint8_t* maps, void* stream);

/* ---- the pre-warp merge of a whole video and its weight search (premvos_amd/csrc/prewarp_ops.hip) ---------------------------------
 * MergeTrack/oldmerge.py ("PREMVOS 1 uses pre-warp"): every proposal carries its mask already warped to the next frame, no network
 * runs in the loop.  All masks of a video are bit-packed in ONE pool: mask s = `stride` bytes at bits + s * stride in the layout of
 * premvos_mask_pack_bits_u8 (bit k of byte i = pixel 8 i + k), stride a multiple of 8 holding h*w bits, the pool 8-byte aligned;
 * bits beyond h*w do not count.  A block table is int32 [B][8], the same values in host memory (checked before any HIP call) and in
 * device memory (read by the kernels); row t = {a0, na, b0, nb, c0, nc, inter_off, area_off}: the na = P_t current masks of frame t
 * from slot a0; the candidates for a template's current mask in frame t, nb from slot b0 then nc from slot c0 (frame 0: the masks of
 * the objects annotated in it; t > 0: the forward masks of frame t-1's proposals, then those of the objects annotated in t-1);
 * the block's [na][nb+nc] intersections from inter[inter_off], its na + nb + nc areas from areas[area_off].  poff [N+1] = where
 * each frame's proposals begin among the video's sumP, first [N+1] = where the objects annotated in each frame begin among the T
 * templates (frame order); both also twice, host and device.  At most 64 templates, 256 proposals per frame and 8000 scores per
 * frame (T x P_t: the chain keeps them in LDS); refused with a message beyond. */
/* oldmerge.py:114-116 (pycocotools iou of every proposal with every template's current mask), for ALL frames in one launch: every
 * count the chain can ask for.  Grid: 16 x 16 pair tiles x blocks; each side is read once per tile; 64 pixels = one popcount.
 * Empty blocks are allowed; inter and areas are zeroed first. */
int premvos_bits_overlap_i32(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                             const int32_t* blocks_dev, int32_t B, int32_t* inter, int64_t n_inter, int32_t* areas, int64_t n_areas,
                             void* stream);
/* oldmerge.py:87-110 get_all_reid_scores: emb_p [sumP][128] (an all-inf row: no 'ReID'), emb_t [T][128] -> maxd [T] (per template,
 * over ALL frames, infinities counted as 0), reid / oreid: frame t's [T][P_t] block at T * poff[t] (1 - d / max, a non-finite score
 * is 0; 1 - the maximum over the OTHER templates, all ones for T == 1).  flat [T][sumP] is workspace. */
int premvos_prewarp_reid_f64(const double* emb_p, const double* emb_t, int32_t sumP, int32_t T, const int32_t* poff_host,
                             const int32_t* poff_dev, int32_t N, double* flat, double* maxd, double* reid, double* oreid, void* stream);
/* oldmerge.py:112-127 calculate_old_merge_scores + :150-197 of do_video, for W weight sets (weights [W][5], normalised) at once: one
 * workgroup per set walks the frames in order.  chosen [W][N][T]: p < P_t = proposal p of the frame, P_t + j = the j-th object
 * annotated in the frame (its score is exactly 1), -1 = the empty mask (a frame without proposals, score 0); best [W][N][T];
 * weighted (W == 1 only, or NULL): the weighted scores before the snapping, in the layout of reid. */
int premvos_prewarp_chain_f64(const int32_t* inter, int64_t n_inter, const int32_t* areas, int64_t n_areas, const int32_t* blocks_host,
                              const int32_t* blocks_dev, const int32_t* poff_host, const int32_t* poff_dev, const int32_t* first_host,
                              const int32_t* first_dev, int32_t N, int32_t T, const double* proposal_score, const double* reid,
                              const double* oreid, const double* weights, int32_t W, int32_t* chosen, double* best, double* weighted,
                              void* stream);
/* oldmerge.py:176-208 (argsort, the paint, the labels, save_with_pascal_colormap's array) and merge_functions.py:613-634 eval_video's
 * counts.  Grid: pixel words x frames x W; a lane resolves 64 pixels of the T chosen masks in paint order (ascending score; equal
 * scores: the higher index last; a NaN last).  The annotation masks are slots ann_slot0 .. + T of the pool; ids [T] (device).
 * idmap (W == 1 only, or NULL) [N][h*w]: the label of the template on top, 0 for one not annotated yet -- which still hides lower
 * scores.  counts (or NULL) int32 [W][N][T0][3] = |R and G|, |R or G|, |R| of template k < T0's painted region against
 * gt_bits [N][T0] (rows of `stride` bytes: annotation id k + 1 of each frame), by wave-reduced integer atomics. */
int premvos_prewarp_paint_bits_u8(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                                  const int32_t* blocks_dev, const int32_t* first_host, const int32_t* first_dev, const int32_t* ids,
                                  int32_t ann_slot0, const int32_t* chosen, const double* best, int32_t N, int32_t T, int32_t W,
                                  uint8_t* idmap, const uint8_t* gt_bits, int32_t T0, int32_t* counts, void* stream);
/* oldmerge.py:63-85 get_negative_ff_props (the switch use_ff_negative_props, oldmerge.py:43): frame 0's P0 proposals (pool slots
 * cur_slot0 ..) in descending `score` (float64 [P0], device; equal scores in index order, as Python's stable sort; a NaN score is
 * never taken), each taken if it shares no pixel with any of the A0 objects annotated in frame 0 (slots ann_slot0 ..) nor with a
 * proposal taken before (`iou > 0` is "the intersection has a pixel": integers only; an empty mask is taken).  K < 0: all, else the
 * walk stops after the K-th.  taken int32 [P0]: proposal indices in acceptance order, -1 beyond the count; count int32 [1];
 * conflict uint8 [P0][A0 + P0] is workspace.  A tiled grid fills `conflict`; one workgroup ranks by counting, keeps the conflict rows as bits in LDS and walks.  P0 <= 256,
 * A0 <= 64; P0 = 0, A0 = 0 and K = 0 are valid (count = 0 for the first and the last). */
int premvos_prewarp_negatives_i32(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, int32_t cur_slot0, int32_t P0,
                                  int32_t ann_slot0, int32_t A0, const double* score, int32_t K, uint8_t* conflict, int32_t* taken,
                                  int32_t* count, void* stream);
/* oldmerge.py:138,147 (`templates = ... + negative_ff_props`, `next_props = ... + negative_ff_props`): for n < n_neg the mask row of
 * proposal taken[n] (device) is copied to pool slot neg_slot0 + n and its embedding emb_p[taken[n]] to emb_neg[n] ([n_neg][128], the
 * last rows of the templates' embeddings), all inside device memory.  The negatives' slots may not overlap the proposals'. */
int premvos_prewarp_gather_neg_u8(uint8_t* bits, int32_t S, int64_t stride, int32_t cur_slot0, int32_t P0, int32_t neg_slot0,
                                  int32_t n_neg, const int32_t* taken, const double* emb_p, double* emb_neg, void* stream);
/* premvos_prewarp_chain_f64 with the last n_neg of the T templates being negatives (oldmerge.py:137-138,147): `first` runs to
 * T - n_neg; block 0's columns are the first[1] objects annotated in frame 0 and then the n_neg negatives' own masks (its c0, nc
 * range), where negative j starts; no frame forces a negative (oldmerge.py:168-174 covers annotated objects only), from frame 1 on it
 * carries the forward mask of what it chose (oldmerge.py:196-197).  n_neg = 0 is premvos_prewarp_chain_f64. */
int premvos_prewarp_chain_neg_f64(const int32_t* inter, int64_t n_inter, const int32_t* areas, int64_t n_areas, const int32_t* blocks_host,
                                  const int32_t* blocks_dev, const int32_t* poff_host, const int32_t* poff_dev, const int32_t* first_host,
                                  const int32_t* first_dev, int32_t N, int32_t T, int32_t n_neg, const double* proposal_score,
                                  const double* reid, const double* oreid, const double* weights, int32_t W, int32_t* chosen, double* best,
                                  double* weighted, void* stream);
/* premvos_prewarp_paint_bits_u8 with n_neg trailing negatives (oldmerge.py:148,173: their label stays 0 in every frame, they paint
 * and hide lower scores): `first` runs to T - n_neg, the annotation masks are slots ann_slot0 .. + T - n_neg, ids [T - n_neg],
 * T0 <= T - n_neg (oldmerge.py:210: only frame 0's objects are scored).  n_neg = 0 is premvos_prewarp_paint_bits_u8. */
int premvos_prewarp_paint_neg_bits_u8(const uint8_t* bits, int32_t S, int64_t stride, int64_t hw, const int32_t* blocks_host,
                                      const int32_t* blocks_dev, const int32_t* first_host, const int32_t* first_dev, const int32_t* ids,
                                      int32_t ann_slot0, const int32_t* chosen, const double* best, int32_t N, int32_t T, int32_t n_neg,
                                      int32_t W, uint8_t* idmap, const uint8_t* gt_bits, int32_t T0, int32_t* counts, void* stream);
/* The ingest of that pool, fused: for masks uint8 [n][h][w] grouped by frame (frame v owns [frame_first[v], frame_first[v+1]); the
 * table V+1 long, flow_of_frame V long, each twice: host memory for the checks, device memory for the kernel) row i of cur_bits is
 * what premvos_mask_pack_bits_u8 writes for mask i, and row i of fwd_bits the same packing of merge_functions.py:209-217 warp_flow
 * (cv2.remap of the mask by its frame's flow, then == 1; what premvos_mask_warp_seats_u8 with binarize writes), as MergeTrack/
 * oldmerge.py's proposals carry their mask warped to the next frame.  flows float [nflows][h][w][2]; flow_of_frame[v] = -1 (a
 * video's last frame): the frame's forward rows are zero.  Rows are row_bytes = ((h*w + 63) / 64) * 8 bytes, 8-byte aligned, zero
 * beyond h*w.  1 <= V <= 4096.  The masks may overlap neither output.  Grid: 1024-pixel blocks x V; a wave's ballot is one word. */
int premvos_mask_warp_pack_bits_u8(const uint8_t* masks, int32_t n, int32_t h, int32_t w, const int32_t* frame_first,
                                   const int32_t* frame_first_dev, const int32_t* flow_of_frame, const int32_t* flow_of_frame_dev,
                                   const float* flows, int32_t nflows, int32_t V, uint8_t* cur_bits, uint8_t* fwd_bits, int64_t row_bytes,
                                   void* stream);

/* ---- the ensemble of several merges of one video (premvos_amd/csrc/ensemble_ops.hip) ----------------------------------------------
 * MergeTrack/oldmerge.py:129-131,220-224 runs do_video(video_fn, ensemble_num) once per row of weight_set and writes each run under
 * to_ensemble/<n>/; this entry is the combination of those trees, pixel by pixel: maps = K id maps of `pixels` bytes, set k at
 * maps + k * set_stride (set_stride >= pixels; a [K][N][h][w] stack: pixels = set_stride = N*h*w).  Labels are plain bytes, 0 one of
 * them.  With c_k = the number of sets j whose label at the pixel equals set k's, voted[p] = the label of the k with the largest c_k,
 * the SMALLEST such k on a tie (the set listed first breaks ties); votes[p] (or NULL) = that c_k, 1 .. K; hist (or NULL) int64 [K + 1]:
 * hist[v] += the number of pixels whose winner has v votes -- zeroed by the caller once per video, the entry only ADDS (per-lane
 * counts, wave sums, one integer atomic per bucket and workgroup: two calls on zeroed counters give the same bits).  1 <= K <= 8;
 * pixels = 0 is a no-op.  Any alignment works; with maps, set_stride, voted and votes multiples of 16 a lane moves 16-byte vectors.
 * voted and votes may overlap neither the maps nor each other. */
int premvos_idmap_vote_u8(const uint8_t* maps, int32_t K, int64_t set_stride, int64_t pixels, uint8_t* voted, uint8_t* votes,
                          int64_t* hist, void* stream);

/* ---- boundary refinement: a fully connected CRF over frames and id maps (premvos_amd/csrc/crf_ops.hip) ----------------------------
 * ReID_net/scripts/postproc/crf/crf_davis.py:43-60 (apply_crf) runs pydensecrf on a frame: a Gaussian kernel (sxy, compat), a bilateral
 * kernel (sxy, srgb, compat), Potts compatibility, symmetric normalisation, 12 mean-field rounds, argmax.  These four entries are that
 * rule with both filters computed exactly over a square window of radius R (|dy|, |dx| <= R, the centre included, clipped at the
 * frame's borders) instead of on the permutohedral lattice:
 *   k(i,j)  = exp(-(dy^2 + dx^2) / (2 sxy^2) [- |I_i - I_j|^2 / (2 srgb^2)]),    n(i) = 1 / sqrt(sum_j k(i,j) + 1e-20)
 *   Q~_m[l,i] = n_m(i) sum_j k_m(i,j) n_m(j) Q[l,j],    Q <- softmax_l(-U + gcompat Q~_g + compat Q~_b),    Q^0 = softmax_l(-U)
 * All four take stacks of n frames (frames uint8 [n][h][w][3], maps uint8 [n][h][w], U / Q float [n][L][h][w], normalisers float
 * [n][h][w]), run on `stream`, use fp32 and no float atomics (two calls give the same bits; a frame's result does not depend on the
 * frames stacked with it) and refuse, before any HIP call: null pointers, n, h or w < 1 (or n > 65535, h * w > 2^26), L outside 2 .. 16,
 * a radius outside 0 .. 64, sigmas that are not positive, gt_prob outside (0, 1). */

/* crf_davis.py:43-60 with pydensecrf's unary_from_labels (no "unsure" label): unary[l] = -log(gt_prob) where l is the pixel's label and
 * -log((1 - gt_prob) / (L - 1)) elsewhere; q0 = softmax_l(-unary).  flag: int32 [1] in device memory, set when a map holds a label >= L:
 * then NOTHING is written to unary / q0 and the call returns PREMVOS_EINVAL -- the one entry that waits for its stream, to say so. */
int premvos_crf_unary_labels_f32(const uint8_t* idmaps, int32_t n, int32_t h, int32_t w, int32_t L, float gt_prob, float* unary, float* q0,
                                 int32_t* flag, void* stream);

/* crf_davis.py:43-60, densecrf's NORMALIZE_SYMMETRIC: norm[i] = n(i) of ONE kernel; srgb = 0: no colour term (the Gaussian kernel).
 * It depends on the frame alone: once per frame, not per round. */
int premvos_crf_norm_f32(const uint8_t* frames, int32_t n, int32_t h, int32_t w, float sxy, float srgb, int32_t R, float* norm, void* stream);

/* crf_davis.py:43-60, one mean-field round with both kernels (gsxy, gR, gcompat: the Gaussian; sxy, srgb, R, compat: the bilateral; n_g,
 * n_b: their normalisers): q_out = softmax_l(-unary + gcompat Q~_g + compat Q~_b) of q_in.  q_in = NULL: no message, q_out = Q^0 (for a
 * unary that did not come from labels).  q_out must not overlap q_in.  Grid: 64 x 16-pixel tiles x n; up to 64 KB of LDS. */
int premvos_crf_step_f32(const uint8_t* frames, const float* unary, const float* q_in, const float* n_g, const float* n_b, int32_t n, int32_t h,
                         int32_t w, int32_t L, float gsxy, int32_t gR, float gcompat, float sxy, float srgb, int32_t R, float compat,
                         float* q_out, void* stream);

/* crf_davis.py:43-60, the MAP: idmap = argmax_l q, a tie to the lowest label; changed int32 [n] = per frame the pixels whose label is
 * not `before`'s (uint8 [n][h][w], the maps the unary came from), zeroed by the call, integer adds. */
int premvos_crf_argmax_u8(const float* q, int32_t n, int32_t h, int32_t w, int32_t L, const uint8_t* before, uint8_t* idmap, int32_t* changed,
                          void* stream);

/* ---- host-side file writer (no GPU work; premvos_amd/csrc/host_files.hip) -------------------------------------------------
 * The files of ONE frame from the arrays its results consist of, without the Python interpreter (ctypes releases the interpreter
 * lock for the call, so N writer threads run at once): what the merge rank of a gathered multi-GPU job does ~430 times per second.
 * Same bytes as the Python writers of the stage drivers, i.e. as the reference's:
 *   flo_path      script_pwc_multi.py:16-31 writeFlowFile           (NULL: none -- the last frame of a video has no pair)
 *   json_path[0]  general proposals   proposal_net/eval.py:93-94 (boxes / scale, clip) + train.py:388-428 (xywh, round, json.dump)
 *   json_path[1]  specific proposals  (same)
 *   json_path[2]  combined            combine_general_and_specific.py:33 (general + specific)
 *   json_path[3]  refined             FewShotSegmentationForwarder.py:137-155: combined + "segmentation" {"size", "counts"} +
 *                                     "conf_score" (str of the float32); slot i of the frame = rle_offsets[i] .. [i + 1] in rle_pool
 *                                     (premvos_rle_boundaries_pooled_u8), conf[i]
 * Any json_path may be NULL (that file is not written).  boxes: [count][4] x0 y0 x1 y1 in RESIZED-image coordinates, probs: [count].
 * Returns 0, 1 when a directory of some path does not exist (the caller creates it and calls again; files already written are
 * simply written again) or a negative error. */
typedef struct premvos_frame_files {
  const char* flo_path;
  const float* flow;              /* [h][w][2], flow_row_stride floats between rows (>= 2 w) */
  int64_t flow_row_stride;
  int32_t h, w;
  const float* boxes[2];          /* general, specific */
  const float* probs[2];
  int32_t count[2];
  float scale;                    /* float32 of (newh / h + neww / w) / 2 (eval.py:78) */
  const char* json_path[4];
  const float* conf;              /* [count[0] + count[1]] */
  const int32_t* rle_pool;
  const int32_t* rle_offsets;     /* [count[0] + count[1] + 1] (a window of the chunk's offsets) */
} premvos_frame_files;
int premvos_write_frame_files_host(const premvos_frame_files* f);
/* Test hook of the number formatting above: n doubles -> one line each, as Python's repr(float) (json.dump) or, as_float32_str != 0,
 * as numpy's str(float32(value)).  Returns the length written or a negative error. */
int premvos_format_floats_host(const double* values, int64_t n, int32_t as_float32_str, char* out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PREMVOS_HIP_H */
