/* libmdcv_ign.so — C ABI of the opt-in prediction-IoU ignore rule of the fused YOLO head (csrc/yolo_ign.hip): Darknet's
 * `ignore_thresh`.  A cell that nobody owns, but whose PREDICTED box already overlaps a labelled box of its own image by more than `thr`,
 * leaves the no-object term, forward and gradient, on the device, behind mdcv_yolo_head_train / mdcv_yolo_head_grad of
 * include/mdcv_hip.h on the same stream.
 *
 * The conventions are those of include/mdcv_hip.h, include/mdcv_cls.h and include/mdcv_box.h: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on
 * success, MDCV_EARG for an argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a
 * positive hipError_t otherwise.  A header and a library of its own for the reason include/mdcv_cls.h gives.  Geometry, sigmoid and
 * workspace layout are shared as source (csrc/yolo_head_core.h).
 *
 * Semantics.  logits are the head's: NHWC, channel = a*(5+C) + attr (attr 0..4 = x, y, w, h, conf), channel stride ldc; targets
 * [B,T,5] (class, cx, cy, w, h); anchors_scaled [A,2] in grid units; head_workspace is the workspace mdcv_yolo_head_train of THIS step
 * left behind: owner[cell], the batch-wide ignore[Gh*Gw] plane (the reference's shape-against-anchor rule, which stays as it is),
 * acc[5] = the sum of BCE(p, 0) over the negatives and acc[7] = nN, their number.
 * A label row is REAL when the fp32 sum of its five words, added in the head's order (((c + cx) + cy) + w) + h, is > 0: the head's
 * master_mask.  Its box in grid units is gx = cx*Gw, gy = cy*Gh, gw = w*Gw, gh = h*Gh, the fp32 products the head forms.  Padding rows
 * are not labels.
 * The predicted box of cell (b, a, j, i), with (aw, ah) = anchors_scaled[a], zx zy zw zh its logits and sigmoid the head's fp32 sigmoid:
 *   px = sigmoid(zx) + i     py = sigmoid(zy) + j     pw = exp(min(zw, 20)) * aw     ph = exp(min(zh, 20)) * ah
 * Boxes are continuous (no "+1"), as in include/mdcv_box.h; every operation is one fp32 operation rounding on its own:
 *   iw = min(px + pw/2, gx + gw/2) - max(px - pw/2, gx - gw/2), ih the same in y; inter = iw * ih when iw > 0 and ih > 0, else 0
 *   union = pw*ph + gw*gh - inter + 1e-7
 * A cell is IGNORED when (1) owner[cell] < 0, (2) ignore[j*Gw + i] == 0 and (3) inter > thr * union for at least one real row of ITS
 * image b.  No division is made, and union >= 1e-7, so everything is finite for any finite logits and any labels, zero-size ones
 * included.  With S the sum of BCE(p, 0) = -max(log(1 - sigmoid(zconf)), -100) over the ignored cells and n their number:
 *   nN' = nN - n        loss_noobj = no_object_loss * (acc5 - S) / nN'        (NaN when nN' == 0: a mean over an empty selection)
 * and in the gradient the conf word of an ignored cell is 0 * gscale, every remaining negative is scaled by 1 / nN' instead of 1 / nN,
 * and no other channel and no owned cell changes.
 *
 * THE ONE WRITE INTO THE HEAD WORKSPACE.  When n > 0, mdcv_yolo_ign_loss replaces acc[5] by acc5 - S (exactly 0 when nN' == 0) and
 * acc[7] by nN' in head_workspace; nothing else of it is written.  The mdcv_yolo_head_grad that follows therefore scales the remaining
 * negatives by 1 / nN' unchanged.  A gradient that mdcv_yolo_head_train wrote itself (dlogits != NULL) used the old nN: with this rule
 * on, pass dlogits = NULL there and call mdcv_yolo_head_grad behind mdcv_yolo_ign_loss.  When n == 0 every byte of out7 and of
 * head_workspace keeps its bits.
 *
 * ign_workspace: mdcv_yolo_ign_workspace_bytes() bytes, 8-byte aligned: two fp64 sums (S, n), ZERO before the first call and left zero
 * again by every mdcv_yolo_ign_loss, then the bit mask of the ignored cells, rewritten whole by every call: 64-bit words, 4 *
 * ceil(A*Gh*Gw / 256) of them per image, image after image; bit k of word w of image b is the cell q = 64*w + k of that image in the
 * kernel's order, pixel-major and anchor-minor: a = q % A, j = (q / A) / Gw, i = (q / A) % Gw (bits with q >= A*Gh*Gw are 0). */
#ifndef MDCV_IGN_H
#define MDCV_IGN_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif

long long mdcv_yolo_ign_workspace_bytes(int B, int A, int Gh, int Gw);

/* label rows compacted into LDS per pass of the mask kernel; any T is served, in ceil(T / this) passes */
int mdcv_yolo_ign_rows_per_pass(void);

/* Writes the mask; out7[0] and out7[6] += fp32(no_object_loss * ((acc5 - S) / nN' - acc5 / nN)), the difference formed in fp64 and
 * rounded once; ign_out[0] = n, ign_out[1] = nN'; the write into head_workspace stated above.  Two launches.
 * MDCV_EARG: a NULL pointer, dtype not MDCV_F32 / MDCV_BF16, any of B T A C Gh Gw < 1, Gh or Gw > 4095, A > 127 (the head's limits),
 * ldc < A*(5+C), B*T above 2^31 - 2^16, B * ceil(A*Gh*Gw / 256) above 2^31 - 1, thr outside (0, 1) (NaN included), ign_workspace
 * not 8-byte aligned. */
int mdcv_yolo_ign_loss(int dtype, const void* logits, int ldc, const float* targets, const float* anchors_scaled, int B, int T, int A, int C,
                       int Gh, int Gw, float thr, float no_object_loss, void* head_workspace, void* ign_workspace, float* out7,
                       float* ign_out, void* stream);

/* Writes 0 * *gscale (gscale NULL: 1) into the conf word, channel a*(5+C) + 4, of every ignored cell in dlogits (channel stride ldd),
 * the plane mdcv_yolo_head_grad has just written.  Sparse: a wave whose mask word is zero does nothing; no other byte is written.  One
 * launch.  MDCV_EARG as above (no T, ldc or thr here), and for A*(5+C) > Cpad or ldd < Cpad. */
int mdcv_yolo_ign_grad(int dtype, void* dlogits, int ldd, int Cpad, int B, int A, int C, int Gh, int Gw, const void* ign_workspace,
                       const float* gscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
