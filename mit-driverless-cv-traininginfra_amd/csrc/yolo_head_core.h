// The pieces of the fused YOLO head that more than one unit runs: csrc/yolo_head.hip (assignment, six-part loss, gradient, decode) and
// csrc/yolo_cls.hip (the opt-in class loss, libmdcv_cls.so).  One definition each, so that the two cannot drift apart: the geometry of a
// head, the assignment of one label row, the head's sigmoid and the layout of its workspace.  Every unit that includes this is built
// with -ffp-contract=off: the integer assignment (gi, gj, best anchor) is BIT-EXACT with the reference only if every fp32 operation
// below rounds on its own, in the reference's order.
#pragma once
#include "common.h"

namespace {

struct HeadGeom {
  int B, T, A, C, Gh, Gw, ldc;
  float thresh;
};

// row (b,t) -> source row (padding rows take row 0, utils.py:223-228), grid coords, best anchor, "any IoU > thresh"
__device__ __forceinline__ void assign_row(const float* __restrict__ tg, const float* __restrict__ anchors, const HeadGeom& g, int b, int t,
                                           int& src, int& gi, int& gj, int& best, bool& over, float& gx, float& gy, float& gw, float& gh) {
  const float* r = tg + ((size_t)b * g.T + t) * 5;
  float s = r[0]; s = s + r[1]; s = s + r[2]; s = s + r[3]; s = s + r[4];       // utils.py:210
  src = s > 0.f ? t : 0;
  const float* q = tg + ((size_t)b * g.T + src) * 5;
  gx = q[1] * (float)g.Gw; gy = q[2] * (float)g.Gh; gw = q[3] * (float)g.Gw; gh = q[4] * (float)g.Gh;   // :213-216
  gi = (int)gx; gj = (int)gy;                                                    // :219-220 truncation
  best = 0; over = false;
  float best_iou = -1.f;
  for (int a = 0; a < g.A; ++a) {                                               // :236-240 via bbox_iou :178-191
    const float aw = anchors[2 * a], ah = anchors[2 * a + 1];
    const float ix = fminf(gw, aw) - 0.f + 1.f, iy = fminf(gh, ah) - 0.f + 1.f;
    const float inter = fmaxf(ix, 0.f) * fmaxf(iy, 0.f);
    const float a1 = (gw - 0.f + 1.f) * (gh - 0.f + 1.f);
    const float a2 = (aw - 0.f + 1.f) * (ah - 0.f + 1.f);
    const float iou = inter / (a1 + a2 - inter + 1e-12f);
    if (iou > g.thresh) over = true;
    if (iou > best_iou) { best_iou = iou; best = a; }                            // :257 first max wins
  }
}

// 1 / (1 + expf(-x)) wherever expf(-x) is finite.  From x = -88.8 down expf(-x) is inf and the quotient 0, while the true value
// e^x / (1 + e^x) = e^x (1 + e^x rounds to 1) is still a (denormal) fp32 number: with 0, BCE(p, 1) clamps at 100 instead of -x and its
// gradient vanishes.  Every logit above -88.8 keeps the bits it always had, so a training run without such logits is unchanged.
// Used by the loss, gradient and decode kernels only: the assignment path has no sigmoid.
__device__ __forceinline__ float sigmoidf_(float x) {
  const float e = expf(-x);
  return e == INFINITY ? expf(x) : 1.f / (1.f + e);
}

// workspace of one head (mdcv_yolo_head_workspace_bytes): ints owner[B*A*Gh*Gw] | ignore[Gh*Gw] | err[1] (+pad to an even count) ; then
// acc[8] doubles (8-byte aligned by construction): sums (x,y,w,h,obj,noobj), acc[6] = nM (cells with an owner), acc[7] = nN
struct HeadWs {
  int* owner; int* ignore; int* err; double* acc;
  long long cells, ints;
};
static inline HeadWs head_ws(void* workspace, int B, int A, int Gh, int Gw) {
  HeadWs w;
  w.cells = (long long)B * A * Gh * Gw;
  w.ints = (w.cells + (long long)Gh * Gw + 2 + 1) & ~1LL;
  w.owner = (int*)workspace; w.ignore = w.owner + w.cells; w.err = w.ignore + (long long)Gh * Gw;
  w.acc = (double*)((int*)workspace + w.ints);
  return w;
}

}  // namespace
