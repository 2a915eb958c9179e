/* libmdcv_box.so — C ABI of the opt-in box loss of the fused YOLO head (csrc/yolo_box.hip): GIoU, DIoU or CIoU between the
 * predicted and the labelled box of every owned cell, forward and gradient, on the device, behind mdcv_yolo_head_train /
 * mdcv_yolo_head_grad of include/mdcv_hip.h on the same stream.
 *
 * The conventions are those of include/mdcv_hip.h and include/mdcv_cls.h: plain C symbols, plain pointers and sizes, caller-owned device
 * buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success, MDCV_EARG for an
 * argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a positive hipError_t otherwise.
 * A header and a library of its own for the reason include/mdcv_cls.h gives: include/mdcv_hip.h's stream-taking entries are pinned by
 * host tests to the schedule-hazard tables.  Geometry, row assignment, sigmoid and workspace layout are shared as source
 * (csrc/yolo_head_core.h).
 *
 * Semantics.  logits are the head's: NHWC, channel = a*(5+C) + attr (attr 0..3 = x, y, w, h), channel stride ldc; targets [B,T,5]
 * (class, cx, cy, w, h); anchors_scaled [A,2] in grid units.  head_workspace is the workspace mdcv_yolo_head_train of THIS step left
 * behind (read only): owner[cell] says which label row owns a cell, acc[6] is nM, the number of owned cells.
 * For an owned cell (b, a, gj, gi) with owner row t: gx, gy, gw, gh are the fp32 products the head's row assignment forms from the
 * row's source row (cx*Gw, cy*Gh, w*Gw, h*Gh; a padding row reads row 0), (aw, ah) = anchors_scaled[a], zx zy zw zh the four logits,
 * sigmoid the head's fp32 sigmoid; everything after these inputs is fp64 on the device, in grid units:
 *   px = sigmoid(zx) + gi     py = sigmoid(zy) + gj
 *   pw = exp(min(zw, 20)) * aw  ph = exp(min(zh, 20)) * ah
 *   iw = max(min(px+pw/2, gx+gw/2) - max(px-pw/2, gx-gw/2), 0), ih the same in y, inter = iw * ih
 *   union = pw*ph + gw*gh - inter + eps,  iou = inter / union,  eps = 1e-7
 *   cw = max(px+pw/2, gx+gw/2) - min(px-pw/2, gx-gw/2), ch the same in y: the smallest box enclosing both
 *   MDCV_BOX_GIOU  q = iou - (cw*ch + eps - union) / (cw*ch + eps)
 *   MDCV_BOX_DIOU  q = iou - rho2 / c2,  rho2 = (px-gx)^2 + (py-gy)^2,  c2 = cw^2 + ch^2 + eps
 *   MDCV_BOX_CIOU  q = iou - (rho2 / c2 + alpha * v),  v = 4/pi^2 * (atan(gw/(gh+eps)) - atan(pw/(ph+eps)))^2,
 *                  alpha = v / (v - iou + 1 + eps), a CONSTANT in the gradient (Zheng et al. 2020)
 *   loss_box = box_loss / nM * sum over owned cells of (1 - q)      (a mean over the mask like the head's four MSE parts: no 1/B)
 *   mean_iou = 1 / nM * sum over owned cells of iou                 (plain IoU: a training metric, no gradient)
 *   dz = d loss_box / dz through dpx/dzx = s (1 - s), s the fp32 sigmoid, and dpw/dzw = pw for zw <= 20, 0 above (the clamp).
 * Boundaries.  nM == 0 gives NaN for both sums, like the six parts of the head.  Every value is finite for any finite logits and any
 * label row: union, cw*ch + eps, c2, gh + eps, ph + eps and the denominator of alpha (iou < 1 always) are all >= eps > 0, so a label
 * of zero width or height, a predicted width that underflows to 0 and exp(20) * anchor are all served.  A row whose centre is outside
 * the grid is dropped, as the head drops it (and flags it in ITS err word).  Subgradients at an exact tie: of min(u, v) / max(u, v)
 * with u the predicted and v the labelled edge, the LABEL takes the tie (the predicted edge gets no gradient: the comparisons are
 * strict); max(., 0) of the overlap passes no gradient at 0; zw == 20 exactly still passes its gradient.
 *
 * box_workspace: mdcv_yolo_box_workspace_bytes() bytes, 8-byte aligned, ZERO before the first call; every mdcv_yolo_box_loss leaves it
 * zero again, so a buffer is zeroed once, when it is allocated. */
#ifndef MDCV_BOX_H
#define MDCV_BOX_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif

#define MDCV_BOX_GIOU 0
#define MDCV_BOX_DIOU 1
#define MDCV_BOX_CIOU 2

long long mdcv_yolo_box_workspace_bytes(void);

/* out7[0] += loss_box, box_out[0] += loss_box, box_out[1] = mean_iou (out7[1..6] are not touched).  Two launches.
 * MDCV_EARG: a NULL pointer, dtype not MDCV_F32 / MDCV_BF16, an unknown mode, any of B T A C Gh Gw < 1, Gh or Gw > 4095, A > 127 (the
 * head's limits), ldc < A*(5+C), B*T above 2^31 - 2^16, box_workspace not 8-byte aligned. */
int mdcv_yolo_box_loss(int dtype, const void* logits, int ldc, const float* targets, const float* anchors_scaled, int B, int T, int A, int C,
                       int Gh, int Gw, float thresh, int mode, float box_loss, const void* head_workspace, void* box_workspace, float* out7,
                       float* box_out, void* stream);

/* ADDS dz * *gscale (gscale NULL: 1) to the four channels a*(5+C) + 0..3 of every owned cell in dlogits (channel stride ldd), the plane
 * mdcv_yolo_head_grad has just written: the word is read, the sum formed in fp32 and rounded once to the logits' dtype, so the head's
 * MSE gradients stay beside it.  No other byte is written and no pad channel is read.  One launch.  MDCV_EARG as above, and for
 * A*(5+C) > Cpad or ldd < Cpad. */
int mdcv_yolo_box_grad(int dtype, const void* logits, int ldc, void* dlogits, int ldd, int Cpad, const float* targets,
                       const float* anchors_scaled, int B, int T, int A, int C, int Gh, int Gw, float thresh, int mode, float box_loss,
                       const void* head_workspace, const float* gscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
