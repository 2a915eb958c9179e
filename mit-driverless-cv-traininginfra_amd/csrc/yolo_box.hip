// Opt-in box loss of the fused YOLO head for gfx950 (libmdcv_box.so, include/mdcv_box.h): GIoU / DIoU / CIoU between the
// predicted and the labelled box of every owned cell, forward and gradient.  The definition is in the header.
//
// The reference regresses boxes with four unrelated MSE terms (CVC-YOLOv3/models.py:199-202); this is the IoU-family loss every YOLO
// since v4 trains with, beside or instead of them.
//
// The work is SPARSE and SCALAR: at most B*T cells carry a box term, and a cell is one row assignment, one owner lookup, four logits
// and about a hundred flops.  So, unlike the class loss (a wave per row, lanes over the classes):
//   one LANE per label row (b,t), 64 rows per wave, 256 per block, grid-stride over B*T rows
//   the lane recomputes assign_row for its row (csrc/yolo_head_core.h, bit-exact with the head) and reads owner[cell] of the head's
//     workspace: only the owner row of a cell goes on, so every owned cell is visited by exactly one lane of one launch and the
//     read-modify-write of the gradient needs no atomic
//   the four logits of the cell (and, in the gradient pass, the four dlogits words) move as ONE 16-byte (fp32) or 8-byte (bf16) vector
//     where the address allows, as four scalars otherwise (A*(5+C) odd, a channel stride that is no multiple of four)
//   box_term() below is the whole arithmetic, in fp64 (B*T rows: the rate of the fp64 pipe does not matter), shared by both kernels:
//     it returns 1 - q, the IoU and the four partials; the loss kernel drops the partials at compile time
//   px, py come from the head's fp32 sigmoidf_, so the box loss sees the probabilities the head's own terms see
//   loss: lane-local fp64 partials of both sums over all rows of the lane, ONE wave reduction each at the end, four waves through LDS,
//     one atomic pair per block; a one-thread finalize divides by nM, adds into out7[0] / box_out and zeroes the accumulators
// Compiled with -ffp-contract=off like yolo_head.hip: assign_row must round as the head's does, or a cell would miss its owner.
#include "yolo_head_core.h"
#include "../../include/mdcv_box.h"

namespace {

struct BoxArgs {
  const void* logits; void* dlogits; const float* tg; const float* anchors; const int* owner; const double* head_acc;
  double* acc; const float* gscale;
  HeadGeom g; int ldd, mode;
  float k;                                                    // box_loss
};

// one axis of the pair (predicted [u1, u2], labelled [v1, v2]): overlap length i, enclosing length c, and their partials with respect to
// the predicted centre (ic, cc) and the predicted size (is, cs).  Strict comparisons: at a tie the labelled edge is the argument taken.
struct Axis { double i, c, ic, is, cc, cs; };
__device__ __forceinline__ Axis box_axis(double u1, double u2, double v1, double v2) {
  const bool lo = u1 > v1, hi = u2 < v2;                      // the predicted edge is the inner one
  const bool olo = u1 < v1, ohi = u2 > v2;                    // ... the outer one
  const double raw = (hi ? u2 : v2) - (lo ? u1 : v1);
  const bool live = raw > 0.0;
  Axis a;
  a.i = live ? raw : 0.0;
  a.ic = live ? (double)hi - (double)lo : 0.0;
  a.is = live ? 0.5 * ((double)hi + (double)lo) : 0.0;
  a.c = (ohi ? u2 : v2) - (olo ? u1 : v1);
  a.cc = (double)ohi - (double)olo;
  a.cs = 0.5 * ((double)ohi + (double)olo);
  return a;
}

// l = 1 - q, the plain IoU, and d[k] = d(1 - q) / d(px, py, pw, ph)
struct BoxTerm { double l, iou, d[4]; };
__device__ __forceinline__ BoxTerm box_term(int mode, double px, double py, double pw, double ph, double gx, double gy, double gw, double gh) {
  constexpr double eps = 1e-7;
  const Axis X = box_axis(px - 0.5 * pw, px + 0.5 * pw, gx - 0.5 * gw, gx + 0.5 * gw);
  const Axis Y = box_axis(py - 0.5 * ph, py + 0.5 * ph, gy - 0.5 * gh, gy + 0.5 * gh);
  const double inter = X.i * Y.i;
  const double di[4] = {X.ic * Y.i, X.i * Y.ic, X.is * Y.i, X.i * Y.is};
  const double uni = pw * ph + gw * gh - inter + eps;
  const double du[4] = {-di[0], -di[1], ph - di[2], pw - di[3]};
  const double iou = inter / uni;
  double q = iou, dq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dq[k] = (di[k] - iou * du[k]) / uni;
  if (mode == MDCV_BOX_GIOU) {
    const double ca = X.c * Y.c + eps, fill = uni / ca;       // q = iou - (ca - union) / ca = iou - 1 + union / ca
    const double dca[4] = {X.cc * Y.c, X.c * Y.cc, X.cs * Y.c, X.c * Y.cs};
    q += fill - 1.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] += (du[k] - fill * dca[k]) / ca;
  } else {
    const double ex = px - gx, ey = py - gy;
    const double c2 = X.c * X.c + Y.c * Y.c + eps, pen = (ex * ex + ey * ey) / c2;
    const double drho[4] = {2.0 * ex, 2.0 * ey, 0.0, 0.0};
    const double dc2[4] = {2.0 * X.c * X.cc, 2.0 * Y.c * Y.cc, 2.0 * X.c * X.cs, 2.0 * Y.c * Y.cs};
    q -= pen;
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] -= (drho[k] - pen * dc2[k]) / c2;
    if (mode == MDCV_BOX_CIOU) {
      const double kv = 0.40528473456935108578;               // 4 / pi^2
      const double hp = ph + eps, r = pw / hp;
      const double dif = atan(gw / (gh + eps)) - atan(r);
      const double v = kv * dif * dif;
      const double alpha = v / (v - iou + 1.0 + eps);         // a constant in the gradient
      const double dv = -2.0 * kv * dif / (1.0 + r * r) / hp; // dv / dpw ; dv / dph = -r * dv / dpw
      q -= alpha * v;
      dq[2] -= alpha * dv;
      dq[3] += alpha * dv * r;
    }
  }
  BoxTerm t;
  t.l = 1.0 - q; t.iou = iou;
#pragma unroll
  for (int k = 0; k < 4; ++k) t.d[k] = -dq[k];
  return t;
}

// four consecutive elements as one vector where the address allows
template <typename T> struct V4;
template <> struct V4<float> {
  __device__ static __forceinline__ void ld(const float* p, float* z) {
    if (((uintptr_t)p & 15) == 0) { const float4 v = *reinterpret_cast<const float4*>(p); z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w; }
    else { z[0] = p[0]; z[1] = p[1]; z[2] = p[2]; z[3] = p[3]; }
  }
  __device__ static __forceinline__ void st(float* p, const float* z) {
    if (((uintptr_t)p & 15) == 0) *reinterpret_cast<float4*>(p) = make_float4(z[0], z[1], z[2], z[3]);
    else { p[0] = z[0]; p[1] = z[1]; p[2] = z[2]; p[3] = z[3]; }
  }
};
template <> struct V4<bf16_t> {
  __device__ static __forceinline__ void ld(const bf16_t* p, float* z) {
    if (((uintptr_t)p & 7) == 0) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      z[0] = __uint_as_float(v.x << 16); z[1] = __uint_as_float(v.x & 0xffff0000u);
      z[2] = __uint_as_float(v.y << 16); z[3] = __uint_as_float(v.y & 0xffff0000u);
    } else { z[0] = bf2f(p[0]); z[1] = bf2f(p[1]); z[2] = bf2f(p[2]); z[3] = bf2f(p[3]); }
  }
  __device__ static __forceinline__ void st(bf16_t* p, const float* z) {
    if (((uintptr_t)p & 7) == 0) *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(z[0], z[1]), pack_bf16x2(z[2], z[3]));
    else { p[0] = f2bf(z[0]); p[1] = f2bf(z[1]); p[2] = f2bf(z[2]); p[3] = f2bf(z[3]); }
  }
};

// Is row (b,t) the owner of its cell?  If so: the cell's term, the factors dp/dz of its four logits and the element offset of its cell.
struct Cell { BoxTerm t; double dz[4]; size_t pix; int ch; };
template <typename T>
__device__ __forceinline__ bool box_cell(const BoxArgs& a, int row, Cell& c) {
  const HeadGeom& g = a.g;
  const int b = row / g.T, t = row - b * g.T;
  int src, gi, gj, best; bool over; float gx, gy, gw, gh;
  assign_row(a.tg, a.anchors, g, b, t, src, gi, gj, best, over, gx, gy, gw, gh);
  if (gi < 0 || gi >= g.Gw || gj < 0 || gj >= g.Gh) return false;               // dropped by the head (its err word says so)
  if (a.owner[(((size_t)b * g.A + best) * g.Gh + gj) * g.Gw + gi] != t) return false;
  c.pix = ((size_t)b * g.Gh + gj) * g.Gw + gi;
  c.ch = best * (5 + g.C);
  float z[4];
  V4<T>::ld(reinterpret_cast<const T*>(a.logits) + c.pix * g.ldc + c.ch, z);
  const float sx = sigmoidf_(z[0]), sy = sigmoidf_(z[1]);
  const double pw = exp((double)fminf(z[2], 20.f)) * (double)a.anchors[2 * best];
  const double ph = exp((double)fminf(z[3], 20.f)) * (double)a.anchors[2 * best + 1];
  c.t = box_term(a.mode, (double)sx + (double)gi, (double)sy + (double)gj, pw, ph, (double)gx, (double)gy, (double)gw, (double)gh);
  c.dz[0] = (double)sx * (1.0 - (double)sx); c.dz[1] = (double)sy * (1.0 - (double)sy);
  c.dz[2] = z[2] <= 20.f ? pw : 0.0; c.dz[3] = z[3] <= 20.f ? ph : 0.0;          // no gradient through the clamp
  return true;
}

template <typename T>
__global__ __launch_bounds__(256) void yolo_box_loss_kernel(BoxArgs a) {
  const int rows = a.g.B * a.g.T;
  double vl = 0.0, vi = 0.0;
  for (long long row = blockIdx.x * 256ll + threadIdx.x; row < rows; row += gridDim.x * 256ll) {
    Cell c;
    if (!box_cell<T>(a, (int)row, c)) continue;
    vl += c.t.l; vi += c.t.iou;
  }
  __shared__ double red[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double sl = wave_sum_d(vl), si = wave_sum_d(vi);
  if (lane == 0) { red[wave][0] = sl; red[wave][1] = si; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(a.acc + 0, red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    atomicAdd(a.acc + 1, red[0][1] + red[1][1] + red[2][1] + red[3][1]);
  }
}

// out7[0] += loss_box ; box_out[0] += loss_box ; box_out[1] = mean_iou ; the accumulators are cleared for the next call
__global__ void yolo_box_finalize_kernel(const double* __restrict__ head_acc, double* __restrict__ acc, float k, float* __restrict__ out7,
                                         float* __restrict__ box_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nM = head_acc[6];
  const float l = (float)((double)k * acc[0] / nM);           // mean over an empty selection = NaN
  out7[0] += l;
  box_out[0] += l;
  box_out[1] = (float)(acc[1] / nM);
  acc[0] = 0.0; acc[1] = 0.0;
}

template <typename T>
__global__ __launch_bounds__(256) void yolo_box_grad_kernel(BoxArgs a) {
  const int rows = a.g.B * a.g.T;
  const double w = (double)a.k / a.head_acc[6] * (double)(a.gscale ? a.gscale[0] : 1.f);
  for (long long row = blockIdx.x * 256ll + threadIdx.x; row < rows; row += gridDim.x * 256ll) {
    Cell c;
    if (!box_cell<T>(a, (int)row, c)) continue;
    T* pd = reinterpret_cast<T*>(a.dlogits) + c.pix * a.ldd + c.ch;
    float d[4];
    V4<T>::ld(pd, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = d[k] + (float)(w * c.t.d[k] * c.dz[k]);
    V4<T>::st(pd, d);
  }
}

// 32 blocks of 256 lanes hold 8192 rows in one pass (a batch of 64 images with 128 label rows each); beyond that the lanes stride
constexpr int kMaxBlocks = 32;
static unsigned box_grid(long long rows) { const long long b = (rows + 255) / 256; return (unsigned)(b > kMaxBlocks ? kMaxBlocks : b); }

static bool bad_geometry(int dtype, int ldc, int B, int T, int A, int C, int Gh, int Gw, int mode) {
  if (dtype != MDCV_F32 && dtype != MDCV_BF16) return true;
  if (mode != MDCV_BOX_GIOU && mode != MDCV_BOX_DIOU && mode != MDCV_BOX_CIOU) return true;
  if (B < 1 || T < 1 || A < 1 || C < 1 || Gh < 1 || Gw < 1) return true;
  if (Gh > 4095 || Gw > 4095 || A > 127) return true;
  if ((long long)A * (5 + C) > ldc) return true;
  return (long long)B * T > (1LL << 31) - (1LL << 16);
}

}  // namespace

extern "C" {

long long mdcv_yolo_box_workspace_bytes(void) { return 16; }  // two fp64 accumulators: sum of (1 - q), sum of iou

int mdcv_yolo_box_loss(int dtype, const void* logits, int ldc, const float* targets, const float* anchors_scaled, int B, int T, int A, int C,
                       int Gh, int Gw, float thresh, int mode, float box_loss, const void* head_workspace, void* box_workspace, float* out7,
                       float* box_out, void* stream) {
  if (!logits || !targets || !anchors_scaled || !head_workspace || !box_workspace || !out7 || !box_out) return MDCV_EARG;
  if (bad_geometry(dtype, ldc, B, T, A, C, Gh, Gw, mode) || ((uintptr_t)box_workspace & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const HeadWs hw = head_ws(const_cast<void*>(head_workspace), B, A, Gh, Gw);
  BoxArgs a{logits, nullptr, targets, anchors_scaled, hw.owner, hw.acc, (double*)box_workspace, nullptr,
            HeadGeom{B, T, A, C, Gh, Gw, ldc, thresh}, 0, mode, box_loss};
  const unsigned grid = box_grid((long long)B * T);
  if (dtype == MDCV_BF16) hipLaunchKernelGGL(yolo_box_loss_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(yolo_box_loss_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  MDCV_CHECK_LAUNCH();
  hipLaunchKernelGGL(yolo_box_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)hw.acc, a.acc, box_loss, out7, box_out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_yolo_box_grad(int dtype, const void* logits, int ldc, void* dlogits, int ldd, int Cpad, const float* targets,
                       const float* anchors_scaled, int B, int T, int A, int C, int Gh, int Gw, float thresh, int mode, float box_loss,
                       const void* head_workspace, const float* gscale, void* stream) {
  if (!logits || !dlogits || !targets || !anchors_scaled || !head_workspace) return MDCV_EARG;
  if (bad_geometry(dtype, ldc, B, T, A, C, Gh, Gw, mode) || (long long)A * (5 + C) > Cpad || ldd < Cpad) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const HeadWs hw = head_ws(const_cast<void*>(head_workspace), B, A, Gh, Gw);
  BoxArgs a{logits, dlogits, targets, anchors_scaled, hw.owner, hw.acc, nullptr, gscale,
            HeadGeom{B, T, A, C, Gh, Gw, ldc, thresh}, ldd, mode, box_loss};
  const unsigned grid = box_grid((long long)B * T);
  if (dtype == MDCV_BF16) hipLaunchKernelGGL(yolo_box_grad_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(yolo_box_grad_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
