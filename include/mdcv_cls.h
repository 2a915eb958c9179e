/* libmdcv_cls.so — C ABI of the opt-in class loss of the fused YOLO head (csrc/yolo_cls.hip): forward and gradient, on the
 * device, behind mdcv_yolo_head_train / mdcv_yolo_head_grad of include/mdcv_hip.h on the same stream.
 *
 * The conventions are those of include/mdcv_hip.h: plain C symbols, plain pointers and sizes, caller-owned device buffers, enqueue-only
 * on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success, MDCV_EARG for an argument error (checked
 * on the host before any GPU call, so reachable on a machine without a GPU), a positive hipError_t otherwise.
 *
 * Why a header and a library of its own and not inside include/mdcv_hip.h: host tests pin that header's stream-taking
 * entries to the schedule-hazard tables, and a feature change does not edit a test; include/mdcv_aug.h and include/mdcv_kptaug.h went
 * the same way.  The geometry, the row assignment, the sigmoid and the workspace layout are shared as source (csrc/yolo_head_core.h).
 *
 * Semantics.  logits are the head's: NHWC, channel = a*(5+C) + attr, channel stride ldc; targets [B,T,5] (class, cx, cy, w, h);
 * anchors_scaled [A,2] in grid units.  head_workspace is the workspace mdcv_yolo_head_train of THIS step left behind (read only):
 * owner[cell] says which label row owns a cell, acc[6] is nM, the number of owned cells.  k = cls_loss / B, p = sigmoid(z) (the head's).
 * The class target of an owned cell is the set of the class ids (int)targets[b,t,0] of EVERY row t of image b that lands in the cell
 * with the cell's anchor as its best anchor, padding rows (re-read as row 0, with their own class word) included: utils.py:271 sets
 * tcls for every row, not only for the owner.
 *   MDCV_CLS_CE   loss = k / nM * sum_cells ( log sum_c exp(p_c - m) - (p_c* - m) ), m = max_c p_c: cross entropy over the C SIGMOIDS
 *                 (models.py:205), c* = the LOWEST class id of the cell's set (argmax of a multi-hot row = first occurrence);
 *                 dz_c = k / nM * (softmax(p)_c - [c == c*]) * p_c (1 - p_c)
 *   MDCV_CLS_BCE  loss = k / (nM C) * sum_cells sum_c -( y_c max(log p_c, -100) + (1 - y_c) max(log(1 - p_c), -100) ), y the multi-hot
 *                 set; dz_c = k / (nM C) * (p_c - y_c) * pq / max(pq, 1e-12), pq = p_c (1 - p_c)
 * Sums are fp64 on the device.  nM == 0 gives NaN, like the six parts of the head.  A row whose centre is outside the grid is dropped,
 * as the head drops it (and flags it in ITS err word).  A class id outside [0, C) after (int) truncation contributes nothing and sets
 * the class err word; the reference raises IndexError for ids >= C and wraps negative ones.
 *
 * cls_workspace: mdcv_yolo_cls_workspace_bytes() bytes, 8-byte aligned, ZERO before the first call; every mdcv_yolo_cls_loss leaves the
 * accumulator zero again, so a buffer is zeroed once, when it is allocated.  Its int32 word MDCV_CLS_ERR_WORD is the err word of the
 * LAST call (1: a class id was out of range). */
#ifndef MDCV_CLS_H
#define MDCV_CLS_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif

#define MDCV_CLS_CE 0
#define MDCV_CLS_BCE 1
#define MDCV_CLS_MAX_CLASSES 4096   /* a lane keeps one membership bit per 64 classes in one 64-bit word */
#define MDCV_CLS_ERR_WORD 3

long long mdcv_yolo_cls_workspace_bytes(void);

/* out7[0] += loss_cls, cls_out[0] += loss_cls (one float each; out7[1..6] are not touched).  Two launches.
 * MDCV_EARG: a NULL pointer, dtype not MDCV_F32 / MDCV_BF16, an unknown mode, any of B T A C Gh Gw < 1, C > MDCV_CLS_MAX_CLASSES,
 * Gh or Gw > 4095, A > 127 (the head's limits), ldc < A*(5+C), B*T above 2^31 - 2^16. */
int mdcv_yolo_cls_loss(int dtype, const void* logits, int ldc, const float* targets, const float* anchors_scaled, int B, int T, int A, int C,
                       int Gh, int Gw, float thresh, int mode, float cls_loss, const void* head_workspace, void* cls_workspace, float* out7,
                       float* cls_out, void* stream);

/* OVERWRITES the C class channels of every owned cell in dlogits (channel stride ldd) with dz * *gscale (gscale NULL: 1), rounded once
 * to the logits' dtype; mdcv_yolo_head_grad has written the plane before, with zeros there.  No other byte is written and no pad
 * channel is read.  One launch.  MDCV_EARG as above, and for A*(5+C) > Cpad or ldd < Cpad. */
int mdcv_yolo_cls_grad(int dtype, const void* logits, int ldc, void* dlogits, int ldd, int Cpad, const float* targets,
                       const float* anchors_scaled, int B, int T, int A, int C, int Gh, int Gw, float thresh, int mode, float cls_loss,
                       const void* head_workspace, const float* gscale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
