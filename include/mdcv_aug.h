/* libmdcv_aug.so — C ABI of device work that runs OUTSIDE the training step: batch-level augmentation between a loader and the model.
 *
 * The conventions are those of include/mdcv_hip.h: plain C symbols, plain pointers and sizes, caller-owned device buffers, enqueue-only on
 * the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success, MDCV_EARG for an argument error (checked on
 * the host before any GPU call, so reachable on a machine without a GPU), a positive hipError_t otherwise.
 *
 * Why a library of its own: libmdcv_hip.so's enqueueing entries are the closed set the step schedule's hazard tables cover;
 * what is added here is no part of a training plan.  A later change that extends those tables can fold the two libraries together.
 */
#ifndef MDCV_AUG_H
#define MDCV_AUG_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif

/* ---- mosaic: every training image composed from the corners of four images of its own batch (csrc/mosaic.hip); ONE launch.
 *      in [B,C,H,W] fp32 -> out, the same layout, out of place; targets_in [B,T,5] fp32 rows (cls, cx, cy, w, h) normalised ->
 *      targets_out [B,T_out,5].  One descriptor of MDCV_MOSAIC_DESC ints per OUTPUT image b:
 *       [0] apply  0: image b and its label rows pass through (rows t < T_out copied in place, the rest zero; words 1..7 are ignored)
 *                  1: the mosaic below
 *       [1] xc  1..W-1     [2] yc  1..H-1     the centre
 *       [3..6] s0..s3  0..B-1   the source image of quadrant q = 2 qy + qx, which covers x in [qx ? xc : 0, qx ? W : xc), y likewise
 *       [7] must be 0
 *      Pixels, copied as bits (every source gives the corner that touches the centre):
 *       out[b, c, y, x] = in[s_q, c, y - yc + (qy ? 0 : H), x - xc + (qx ? 0 : W)]
 *      Labels.  A source row is a candidate when (((cls + cx) + cy) + w) + h > 0 in fp32 (padded rows stay padded).  For a candidate of
 *      quadrant q, every fp32 operation rounding on its own (no fma), Wf = (float)W:
 *       hw = w * 0.5f; x1 = (cx - hw) * Wf; x2 = (cx + hw) * Wf; dx = (float)(qx ? xc : xc - W); X1 = x1 + dx; X2 = x2 + dx;
 *       X1c = fminf(fmaxf(X1, lo), hi), X2c likewise, (lo, hi) = qx ? (xc, W) : (0, xc); the same in y; w' = X2c - X1c; h' = Y2c - Y1c;
 *       kept iff w' >= min_px && h' >= min_px && w' * h' >= min_visible * ((x2 - x1) * (y2 - y1))      (a NaN drops the row)
 *       kept row: (cls, ((X1c + X2c) * 0.5f) / Wf, ((Y1c + Y2c) * 0.5f) / Hf, w' / Wf, h' / Hf), divisions correctly rounded
 *      Kept rows go to the front of image b's rows in a fixed order, whatever the schedule: quadrant 0 to 3, source row order inside a
 *      quadrant; the rest is zero; a kept row beyond T_out is dropped and counted.
 *      stats int32[4], ACCUMULATED (the caller zeroes it): {rows kept, candidates dropped by the rule, kept rows lost beyond T_out, error
 *      bits}.  A pass-through image counts its candidates as kept (t < T_out) or lost (t >= T_out).  desc_host is validated (MDCV_EARG,
 *      nothing is enqueued); desc is its device copy, which the kernel checks again: an image whose device row fails passes through and
 *      sets bit 0 of stats[3].  No descriptor makes the kernel read or write outside the four buffers.
 *      MDCV_EARG also for: a NULL pointer, B outside 1..65535, H, W, T or T_out < 1, T or T_out > MDCV_MOSAIC_MAX_ROWS, C outside 1..4,
 *      H or W > 4096, min_px < 1, min_visible outside [0, 1] (NaN included), out overlapping in, targets_out overlapping targets_in. */
#define MDCV_MOSAIC_DESC 8
#define MDCV_MOSAIC_MAX_SIDE 4096
#define MDCV_MOSAIC_MAX_ROWS 65536
int mdcv_mosaic_batch(const int* desc_host, const int* desc, int B, int C, int H, int W, const float* in, float* out,
                      const float* targets_in, int T, float* targets_out, int T_out, float min_px, float min_visible, int* stats,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
