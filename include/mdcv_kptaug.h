/* libmdcv_kptaug.so — C ABI of the key-point batch augmentation (csrc/kptaug.hip): device work that runs OUTSIDE the training
 * step, between a loader and the model, like include/mdcv_aug.h's.
 *
 * The conventions are those of include/mdcv_aug.h and include/mdcv_hip.h: plain C symbols, plain pointers and sizes, caller-owned device
 * buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success, MDCV_EARG for an
 * argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a positive hipError_t otherwise.
 *
 * Why a header and a library beside include/mdcv_aug.h / libmdcv_aug.so and not inside them: two host tests pin that pair to
 * mosaic -- the header's prototypes are exactly `mdcv_mosaic_batch`, and the library's exported symbols are exactly the header's -- and a
 * feature change does not edit a test.  Nothing else separates the two: a change that may touch those tests can fold this file and its
 * library into that pair.
 */
#ifndef MDCV_KPTAUG_H
#define MDCV_KPTAUG_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif

/* ---- key-point augmentation: affine warp, left/right flip and per-channel colour of a finished RektNet batch (csrc/kptaug.hip, DESIGN
 *      §30); ONE launch.  imgs [B,C,S,S] fp32, hm [B,K,S,S] fp32, pts [B,K,2] fp32 ((x, y) normalised by S) -> imgs_out, hm_out, pts_out,
 *      the same layouts, out of place.  K must be 7 (the order top, mid_L_top, mid_R_top, mid_L_bot, mid_R_bot, bot_L, bot_R).
 *      One descriptor of MDCV_KPTAUG_DESC ints per image; float words are fp32 carried as their bits:
 *       [0]      flags: bit 0 apply, bit 1 swap (exchange left and right key points); every other bit must be 0
 *       [1..6]   I00 I01 I02 I10 I11 I12   the INVERSE map, output pixel index (x, y) -> source pixel index
 *       [7..12]  F00 F01 F02 F10 F11 F12   the FORWARD map, source point -> output point, both in pixel-index coordinates
 *       [13..15] gain of channel 0, 1, 2   [16..18] bias of channel 0, 1, 2   (all six are checked, whatever C is)
 *       [19..23] must be 0
 *      The kernel never inverts a matrix: the caller supplies both maps and answers for their agreement.
 *      Every fp32 operation below rounds on its own (no fma); fmaxf / fminf return the other operand for a NaN; Sf = (float)S.
 *      Decision per image.  For every k: px = pts[k].x * Sf; py = pts[k].y * Sf; X_k = (F00 * px + F01 * py) + F02;
 *       Y_k = (F10 * px + F11 * py) + F12.  The image is VALID iff all 2K values satisfy 0 <= v <= Sf (a NaN fails; the upper end is Sf,
 *       not S - 1: a label of exactly 1.0 survives an identity map).  The image is AUGMENTED iff its row passes the check, apply is set
 *       and it is valid.  Otherwise its three outputs are its inputs copied as bits.
 *      Pixels of an augmented image, output (c, y, x):
 *       sx = fminf(fmaxf((I00 * (float)x + I01 * (float)y) + I02, -1.f), Sf); sy likewise with the second row;
 *       x0 = floorf(sx); fx = sx - x0; y0 = floorf(sy); fy = sy - y0; the indices x0, x0 + 1, y0, y0 + 1 are each clamped to [0, S-1]
 *       (edge replicate); v00 = in[c, y0, x0], v01 = in[c, y0, x0+1], v10 = in[c, y0+1, x0], v11 = in[c, y0+1, x0+1];
 *       top = v00 + fx * (v01 - v00); bot = v10 + fx * (v11 - v10); v = top + fy * (bot - top);
 *       out = fminf(fmaxf(v * gain_c + bias_c, 0.f), 1.f)
 *      Points of an augmented image: j = swap ? perm[k] : k, perm = [0, 2, 1, 4, 3, 6, 5]; pts_out[k] = (X_j / Sf, Y_j / Sf), the
 *       divisions correctly rounded.
 *      Heat-maps of an augmented image are REGENERATED from the transformed points, not warped: map k is prep_label's map of a one-hot at
 *       (row min((int)Y_j, S-1), column min((int)X_j, S-1)) of an S x S crop -- resized to S x S (the identity), blurred by the 5x5
 *       Gaussian [1, 4, 6, 4, 1] / 16 with BORDER_REFLECT_101 and divided by its sum, in float64 as csrc/kpt_heatmap.h states it
 *       (value = (float)((vy[y] * vx[x]) / (sum_y * sum_x))).  The hot pixel is always inside, so such a map is never NaN.
 *      stats int32[4], ACCUMULATED (the caller zeroes it): {images augmented, images with apply set that were not valid (rejected), images
 *      passed through by their descriptor (apply == 0, or a device row that fails the check), error bits}.  desc_host is validated
 *      (MDCV_EARG, nothing is enqueued); desc is its device copy, which the kernel checks again: an image whose device row fails passes
 *      through and sets bit 0 of stats[3].  Every index the kernel forms is clamped, so no descriptor and no point makes it read or write
 *      outside the buffers.
 *      A row fails the check when a flag bit above bit 1 is set, a float word (1..18) is not finite, or a word of 19..23 is not 0.
 *      MDCV_EARG also for: a NULL pointer, B outside 1..65535, C outside 1..3, S outside 16..256, K != 7, an output buffer that overlaps
 *      an input buffer, another output buffer or stats. */
#define MDCV_KPTAUG_DESC 24
#define MDCV_KPTAUG_MIN_SIZE 16
#define MDCV_KPTAUG_MAX_SIZE 256
int mdcv_kptaug_batch(const int* desc_host, const int* desc, int B, int C, int S, int K, const float* imgs, const float* hm, const float* pts,
                      float* imgs_out, float* hm_out, float* pts_out, int* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
