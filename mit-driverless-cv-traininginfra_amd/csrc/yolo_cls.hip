// Opt-in class loss of the fused YOLO head for gfx950 (libmdcv_cls.so, include/mdcv_cls.h): forward and gradient.
//
// The reference computes loss_cls = c * (1/B) * CrossEntropy(sigmoid(cls)[mask], argmax(tcls[mask])) and multiplies it by a hard-coded 0
// (CVC-YOLOv3/models.py:203-205); here c is an argument, and MDCV_CLS_BCE is YOLOv3's independent logistic classifiers.
//
// The work is SPARSE: at most B*T cells of B*A*Gh*Gw carry a class term, so nothing here walks the cells or the dlogits plane.
//   one wave64 per label row (b,t), four rows per 256-thread block, grid-stride over rows
//   the wave recomputes assign_row for its row (csrc/yolo_head_core.h, bit-exact with the head) and reads owner[cell] of the head's
//     workspace: only the owner row of a cell goes on, so every owned cell is visited by exactly one wave
//   its lanes scan the T rows of image b, 64 at a time, assign_row each; the rows of the same (anchor, cell) are listed by a ballot and
//     their class ids broadcast one by one: c* = their minimum, and lane l keeps bit r of `mine` for class l + 64 r (the multi-hot set)
//   lane l holds sigmoid of classes l and l + 64 in registers (80 classes: both rounds); classes from 128 up are re-read per pass
//   max, sum of exponentials and c*'s sigmoid come from __shfl_xor / __shfl reductions; no LDS per row
//   loss: lane-local fp64 partials over all rows of the wave, ONE wave reduction at the end, four waves through LDS, one atomic per block;
//     a one-thread finalize adds k * sum / nM to out7[0] and to the class scalar and zeroes the accumulator for the next step
//   gradient: the same walk; the wave overwrites the C class channels of its cell in dlogits and touches no other byte
// Compiled with -ffp-contract=off like yolo_head.hip: assign_row must round as the head's does, or a cell would miss its owner.
#include <limits.h>

#include "yolo_head_core.h"
#include "../../include/mdcv_cls.h"

namespace {

struct ClsArgs {
  const void* logits; void* dlogits; const float* tg; const float* anchors; const int* owner; const double* head_acc;
  double* acc; int* errw; const float* gscale;
  HeadGeom g; int ldd, mode;
  float k;                                                    // cls_loss / B
};

struct CellSet {
  int best, gi, gj;
  int cstar;                                                  // lowest class id of the cell's set; INT_MAX: every id was out of range
  unsigned long long mine;                                    // bit r: class lane + 64 r is in the set
};

// Is row (b,t) the owner of its cell?  If so, collect the class set of the cell from ALL rows of image b (wave-uniform result but `mine`).
__device__ __forceinline__ bool cell_set(const ClsArgs& a, int b, int t, int lane, CellSet& cs) {
  const HeadGeom& g = a.g;
  int src, gi, gj, best; bool over; float gx, gy, gw, gh;
  assign_row(a.tg, a.anchors, g, b, t, src, gi, gj, best, over, gx, gy, gw, gh);
  if (gi < 0 || gi >= g.Gw || gj < 0 || gj >= g.Gh) return false;               // dropped by the head (its err word says so)
  if (a.owner[(((size_t)b * g.A + best) * g.Gh + gj) * g.Gw + gi] != t) return false;
  cs.best = best; cs.gi = gi; cs.gj = gj; cs.cstar = INT_MAX; cs.mine = 0ull;
  for (int t0 = 0; t0 < g.T; t0 += 64) {
    const int t2 = t0 + lane;
    int label = -1;                                           // -1: this lane's row is not in the cell
    if (t2 < g.T) {
      int s2, i2, j2, b2; bool o2; float x2, y2, w2, h2;
      assign_row(a.tg, a.anchors, g, b, t2, s2, i2, j2, b2, o2, x2, y2, w2, h2);
      if (i2 == gi && j2 == gj && b2 == best) {
        const float lf = a.tg[((size_t)b * g.T + t2) * 5];    // class word of the ROW itself, padding rows included (utils.py:271)
        if (lf > -1.f && lf < (float)g.C) label = (int)lf;    // (int) truncates towards zero: (-1, 0) -> 0, like .long(); NaN fails
        else if (a.errw) atomicExch(a.errw, 1);               // (the gradient pass has no err word: the loss pass flagged the id)
      }
    }
    unsigned long long m = __ballot(label >= 0);
    while (m) {                                               // one or two rows per cell in practice
      const int from = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int lbl = __shfl(label, from, 64);
      cs.cstar = lbl < cs.cstar ? lbl : cs.cstar;
      if ((lbl & 63) == lane) cs.mine |= 1ull << (lbl >> 6);
    }
  }
  return true;
}

// sigmoids of one cell's class logits: lane l holds classes l and l + 64, later rounds are re-read
template <typename T>
struct ClsRow {
  const T* px; int C, lane; float p0, p1;
  __device__ __forceinline__ ClsRow(const T* px_, int C_, int lane_) : px(px_), C(C_), lane(lane_) {
    p0 = lane < C ? sigmoidf_(ET<T>::ld(px + lane)) : 0.f;
    p1 = lane + 64 < C ? sigmoidf_(ET<T>::ld(px + lane + 64)) : 0.f;
  }
  __device__ __forceinline__ float p(int r) const { return r == 0 ? p0 : (r == 1 ? p1 : sigmoidf_(ET<T>::ld(px + lane + 64 * r))); }
  // m = max_c p_c, s = sum_c exp(p_c - m): torch's log_softmax subtracts the maximum too, and C = 1 comes out as exactly (p, 1)
  __device__ __forceinline__ void max_sum(float& m, float& s) const {
    m = -INFINITY;
    for (int r = 0; lane + 64 * r < C; ++r) m = fmaxf(m, p(r));
    m = wave_max(m);
    s = 0.f;
    for (int r = 0; lane + 64 * r < C; ++r) s += expf(p(r) - m);
    s = wave_sum(s);
  }
};

template <typename T>
__device__ __forceinline__ const T* cell_logits(const ClsArgs& a, int b, const CellSet& cs) {
  const HeadGeom& g = a.g;
  return reinterpret_cast<const T*>(a.logits) + (((size_t)b * g.Gh + cs.gj) * g.Gw + cs.gi) * g.ldc + cs.best * (5 + g.C) + 5;
}

template <typename T>
__global__ __launch_bounds__(256) void yolo_cls_loss_kernel(ClsArgs a) {
  const HeadGeom& g = a.g;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rows = g.B * g.T;
  double v = 0.0;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int b = row / g.T, t = row - b * g.T;
    CellSet cs;
    if (!cell_set(a, b, t, lane, cs)) continue;
    const ClsRow<T> R(cell_logits<T>(a, b, cs), g.C, lane);
    if (a.mode == MDCV_CLS_CE) {
      if (cs.cstar == INT_MAX) continue;
      float m, s;
      R.max_sum(m, s);
      const int rs = cs.cstar >> 6;
      const float ps = __shfl(R.p(lane + 64 * rs < g.C ? rs : 0), cs.cstar & 63, 64);
      if (lane == 0) v += (double)(logf(s) - (ps - m));
    } else {
      for (int r = 0; lane + 64 * r < g.C; ++r) {
        const float pc = R.p(r);
        const bool y = (cs.mine >> r) & 1ull;
        v += (double)(-fmaxf(logf(y ? pc : 1.f - pc), -100.f));                 // BCE, log clamped like torch and like the head's conf terms
      }
    }
  }
  __shared__ double red[4];
  const double s = wave_sum_d(v);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = red[0] + red[1] + red[2] + red[3];
    if (tot != 0.0) atomicAdd(a.acc, tot);
  }
}

// out7[0] += loss_cls ; cls_out[0] += loss_cls ; the accumulator and the pending err word are handed over and cleared for the next call
__global__ void yolo_cls_finalize_kernel(const double* __restrict__ head_acc, double* __restrict__ acc, int* __restrict__ errw, float k, int mode,
                                         int C, float* __restrict__ out7, float* __restrict__ cls_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nM = head_acc[6];
  const float l = k * (float)(acc[0] / (mode == MDCV_CLS_BCE ? nM * (double)C : nM));     // mean over an empty selection = NaN
  out7[0] += l;
  cls_out[0] += l;
  acc[0] = 0.0;
  errw[1] = errw[0];
  errw[0] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void yolo_cls_grad_kernel(ClsArgs a) {
  const HeadGeom& g = a.g;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rows = g.B * g.T;
  const float nM = (float)a.head_acc[6];
  const float up = a.gscale ? a.gscale[0] : 1.f;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int b = row / g.T, t = row - b * g.T;
    CellSet cs;
    if (!cell_set(a, b, t, lane, cs)) continue;
    const ClsRow<T> R(cell_logits<T>(a, b, cs), g.C, lane);
    T* pd = reinterpret_cast<T*>(a.dlogits) + (((size_t)b * g.Gh + cs.gj) * g.Gw + cs.gi) * a.ldd + cs.best * (5 + g.C) + 5;
    if (a.mode == MDCV_CLS_CE) {
      if (cs.cstar == INT_MAX) continue;                      // no valid id: the head's zeros stay
      float m, s;
      R.max_sum(m, s);
      for (int r = 0; lane + 64 * r < g.C; ++r) {
        const int c = lane + 64 * r;
        const float pc = R.p(r);
        const float gr = a.k * (expf(pc - m) / s - (c == cs.cstar ? 1.f : 0.f)) / nM * pc * (1.f - pc);
        ET<T>::st(pd + c, gr * up);
      }
    } else {
      const float nE = nM * (float)g.C;
      for (int r = 0; lane + 64 * r < g.C; ++r) {
        const float pc = R.p(r), pq = pc * (1.f - pc);
        const float y = (cs.mine >> r) & 1ull ? 1.f : 0.f;
        const float gr = a.k * (pc - y) * pq / fmaxf(pq, 1e-12f) / nE;          // the form of the head's conf gradient (yolo_grad_elem)
        ET<T>::st(pd + lane + 64 * r, gr * up);
      }
    }
  }
}

constexpr int kMaxBlocks = 1024;
static unsigned cls_grid(long long rows) { const long long b = (rows + 3) / 4; return (unsigned)(b > kMaxBlocks ? kMaxBlocks : b); }

static bool bad_geometry(int dtype, int ldc, int B, int T, int A, int C, int Gh, int Gw, int mode) {
  if (dtype != MDCV_F32 && dtype != MDCV_BF16) return true;
  if (mode != MDCV_CLS_CE && mode != MDCV_CLS_BCE) return true;
  if (B < 1 || T < 1 || A < 1 || C < 1 || Gh < 1 || Gw < 1) return true;
  if (Gh > 4095 || Gw > 4095 || A > 127 || C > MDCV_CLS_MAX_CLASSES) return true;
  if ((long long)A * (5 + C) > ldc) return true;
  return (long long)B * T > (1LL << 31) - (1LL << 16);
}

// the words behind the fp64 accumulator: [2] err of the call in flight, [3] = MDCV_CLS_ERR_WORD err of the last finished call
struct ClsWs { double* acc; int* errw; };
static ClsWs cls_ws(void* p) { return ClsWs{(double*)p, (int*)p + 2}; }

}  // namespace

extern "C" {

long long mdcv_yolo_cls_workspace_bytes(void) { return 16; }

int mdcv_yolo_cls_loss(int dtype, const void* logits, int ldc, const float* targets, const float* anchors_scaled, int B, int T, int A, int C,
                       int Gh, int Gw, float thresh, int mode, float cls_loss, const void* head_workspace, void* cls_workspace, float* out7,
                       float* cls_out, void* stream) {
  if (!logits || !targets || !anchors_scaled || !head_workspace || !cls_workspace || !out7 || !cls_out) return MDCV_EARG;
  if (bad_geometry(dtype, ldc, B, T, A, C, Gh, Gw, mode) || ((uintptr_t)cls_workspace & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const HeadWs hw = head_ws(const_cast<void*>(head_workspace), B, A, Gh, Gw);
  const ClsWs cw = cls_ws(cls_workspace);
  ClsArgs a{logits, nullptr, targets, anchors_scaled, hw.owner, hw.acc, cw.acc, cw.errw, nullptr,
            HeadGeom{B, T, A, C, Gh, Gw, ldc, thresh}, 0, mode, (float)((double)cls_loss / B)};
  const unsigned grid = cls_grid((long long)B * T);
  if (dtype == MDCV_BF16) hipLaunchKernelGGL(yolo_cls_loss_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(yolo_cls_loss_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  MDCV_CHECK_LAUNCH();
  hipLaunchKernelGGL(yolo_cls_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)hw.acc, cw.acc, cw.errw, a.k, mode, C, out7, cls_out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_yolo_cls_grad(int dtype, const void* logits, int ldc, void* dlogits, int ldd, int Cpad, const float* targets,
                       const float* anchors_scaled, int B, int T, int A, int C, int Gh, int Gw, float thresh, int mode, float cls_loss,
                       const void* head_workspace, const float* gscale, void* stream) {
  if (!logits || !dlogits || !targets || !anchors_scaled || !head_workspace) return MDCV_EARG;
  if (bad_geometry(dtype, ldc, B, T, A, C, Gh, Gw, mode) || (long long)A * (5 + C) > Cpad || ldd < Cpad) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const HeadWs hw = head_ws(const_cast<void*>(head_workspace), B, A, Gh, Gw);
  ClsArgs a{logits, dlogits, targets, anchors_scaled, hw.owner, hw.acc, nullptr, nullptr, gscale,
            HeadGeom{B, T, A, C, Gh, Gw, ldc, thresh}, ldd, mode, (float)((double)cls_loss / B)};
  const unsigned grid = cls_grid((long long)B * T);
  if (dtype == MDCV_BF16) hipLaunchKernelGGL(yolo_cls_grad_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(yolo_cls_grad_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
