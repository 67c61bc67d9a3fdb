/* premvos_post_hip.h -- the post-processing entries of libpremvos_hip.so that came after premvos_hip.h was closed at 89 entry points.
 *
 * The same library, the same conventions (premvos_hip.h: extern "C", raw DEVICE pointers, caller-owned buffers, `stream` a hipStream_t or
 * NULL, 0 = PREMVOS_OK, a negative code with premvos_last_error() otherwise) and the same ABI version: premvos_abi_version() stays 21, no
 * entry of premvos_hip.h changed.  Every entry here checks its arguments before any HIP call.
 *
 * ---- per-object largest-component clean-up of id maps (premvos_amd/csrc/components_ops.hip) ------------------------------------------
 * ReID_net/scripts/postproc/postproc.py:41-63 (postproc_posteriors_connected_components) dilates a binary mask with a 100 x 100 box,
 * labels the connected components of the DILATED mask, counts the original pixels in each and keeps the largest, a tie going to the
 * component found first.  Here the rule runs per object id k = 1 .. L-1 of a DAVIS id map on res = (M == k), independently of the other
 * ids; what is removed becomes background.  A stack of n frames of h x w has the planes (frame, k), plane index frame * (L-1) + (k-1).
 * Integers only: every result is exact and independent of launch geometry, stacking and repetition. */
#ifndef PREMVOS_POST_HIP_H
#define PREMVOS_POST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* postproc.py:41-63, `grey_dilation(res, size=(100, 100))` for every plane: dil uint8 [n][L-1][h][w], dil(y, x) = 1 iff some pixel of
 * (idmaps[frame] == k) lies in rows y - (D-1)/2 .. y + D/2 and columns x - (D-1)/2 .. x + D/2 (scipy's box of an even size reaches one
 * further up and left; its reflecting border adds nothing), else 0.  D = 1 copies (M == k).  n, h, w >= 1, h * w <= 2^26, L from 2 to
 * 256, D from 1 to 255. */
int premvos_cc_dilate_u8(const uint8_t* idmaps, int32_t n, int32_t h, int32_t w, int32_t L, int32_t D, uint8_t* dil, void* stream);

/* postproc.py:41-63, `measure.label(dilated)` in a canonical form: masks uint8 [planes][h][w] (non-zero = set), labels int32
 * [planes][h][w] = the smallest linear index y * w + x of the pixel's 8-connected component inside its plane, -1 where the mask is 0.
 * (Numbering the components in the order of these roots gives skimage's and scipy's numbers.)  Four launches: tiles in LDS, tile
 * borders through agent-scope atomics, flatten in two steps.  planes >= 1, h, w >= 1, h * w <= 2^26. */
int premvos_cc_label_i32(const uint8_t* masks, int64_t planes, int32_t h, int32_t w, int32_t* labels, void* stream);

/* postproc.py:41-63, the count, the choice and the repaint: labels int32 [n][L-1][h][w] are premvos_cc_label_i32's of the dilated
 * planes; per plane the pixels of (idmaps[frame] == k) are counted per root, the root with the largest count wins, on a tie the
 * smallest root (the reference's strict `>` over components numbered in raster order); out_idmaps uint8 [n][h][w] = idmaps with every
 * pixel of id k outside k's winner set to 0 (an id >= L is copied).  removed int32 [n][L-1] = the pixels set to 0, ncomp int32 [n][L-1]
 * = the components that held at least one pixel (0: the id is absent); both and counts_ws (int32, n (L-1) h w: a workspace, its content
 * after the call is unspecified) are zeroed by the call.  out_idmaps does not overlap idmaps.  n from 1 to 65535, other bounds as above. */
int premvos_cc_keep_largest_u8(const uint8_t* idmaps, const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t L, int32_t* counts_ws,
                               uint8_t* out_idmaps, int32_t* removed, int32_t* ncomp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PREMVOS_POST_HIP_H */
