// RektNet validation for a whole batch in one launch: per-sample CrossRatioLoss and per-key-point pixel distances (gfx950, wave64).
//
//   eval_model              <- RektNet/train_eval.py:115-138  (a loader of batch_size 1: the loss of every image ALONE)
//   print_kpt_L2_distance   <- RektNet/train_eval.py:140-186, utils.calculate_distance (utils.py:239-244)
//
// mdcv_cross_ratio_loss (rektnet_head.hip) is the BATCH loss: its geometric term is the mean of a [B,B] all-pairs matrix, which at B = 1 is a
// per-image quantity and at B > 1 is not the mean of the per-image ones.  Here sample i's unit vectors meet only sample i's.
// Row i of the output, 12 floats: loc, geo, total, d0..d6, 0, 0.
//
// Arithmetic as in rektnet_head.hip: fp32 differences and products, fp64 accumulation, one rounding to fp32 per output.
// Reproducibility: which thread adds which element, and in which order, is a function of the element's index INSIDE its sample (so of H and W
// only) -- not of the sample's position in the batch, nor of the 16-byte phase of its first float.  No atomics.  A row is therefore the same
// bits whether its sample is evaluated alone, at the end of a batch of 257, or twice.
#include <limits.h>

#include "../../include/mdcv_hip.h"
#include "common.h"

namespace {

// the 16-byte phase of a float pointer, in floats
__device__ __forceinline__ int phase4(const float* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// The two aligned 16-byte vectors that floats 4g .. 4g+3 of the sample at p (phase s) lie in, and the four floats out of them.  Callers keep
// 1 <= g <= G - 2 (G whole groups in the sample), so neither vector leaves the sample at any phase.  No branch: s is uniform in the workgroup.
struct Vec2 { uint4 lo, hi; };
__device__ __forceinline__ Vec2 ld_straddle(const float* p, int s, int g) {
  const float* q = p + 4 * (size_t)g - s;
  return Vec2{mdcv_ld_stream(q), mdcv_ld_stream(q + 4)};
}
__device__ __forceinline__ void pick_group(const Vec2& v, int s, float* f) {
  float e[8];
  ET<float>::unpack(v.lo, e);
  ET<float>::unpack(v.hi, e + 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = s == 0 ? e[k] : (s == 1 ? e[k + 1] : (s == 2 ? e[k + 2] : e[k + 3]));
  // e[7] is never picked; kept alive to here, or the compiler takes the load's last register for address arithmetic between two loads
  // and has to wait for the load first
  asm volatile("" : : "v"(e[7]));
}

// Sum of (a - b)^2 over the vector part of a sample, groups 1 .. G-2: thread tid adds groups 1 + tid, 1 + tid + 256, ... in that order, U groups
// requested before the first is used.  Past the last group a lane re-reads group G-2 (in bounds) and adds nothing, so the loads of a pass never
// sit behind a branch.  ALIGNED: both samples start on a 16-byte boundary, one vector per group; otherwise two per group (ld_straddle).
// The additions and their order are the same in both forms.
template <bool ALIGNED, int U>
__device__ __forceinline__ double hm_vector_part(const float* __restrict__ a, const float* __restrict__ b, int sa, int sb, int G, int tid) {
  double acc = 0.0;
  for (int g0 = 1 + tid; g0 < G - 1; g0 += 256 * U) {
    float fa[U][4], fb[U][4];
    if (ALIGNED) {
      uint4 va[U], vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = min(g0 + 256 * u, G - 2);
        va[u] = mdcv_ld_stream(a + 4 * (size_t)g);
        vb[u] = mdcv_ld_stream(b + 4 * (size_t)g);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) { ET<float>::unpack(va[u], fa[u]); ET<float>::unpack(vb[u], fb[u]); }
    } else {
      Vec2 va[U], vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = min(g0 + 256 * u, G - 2);
        va[u] = ld_straddle(a, sa, g);
        vb[u] = ld_straddle(b, sb, g);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) { pick_group(va[u], sa, fa[u]); pick_group(vb[u], sb, fb[u]); }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (g0 + 256 * u < G - 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = fa[u][e] - fb[u][e]; acc += (double)(d * d); }
      }
    }
  }
  return acc;
}

// everything of a row that comes from the 14 + 14 point coordinates ; loc_hm: the heat-map sum of loss_type 1 (ignored otherwise)
__device__ __forceinline__ void eval_points_row(const float* __restrict__ P, const float* __restrict__ Tg, int loss_type, int include_geo,
                                                float gamma_h, float gamma_v, float dist_sx, float dist_sy, double loc_hm,
                                                float* __restrict__ row) {
  // difference vectors d_q = P[a] - P[b] and the six terms u.v, as DQ_A / DQ_B / TERM_U / TERM_V in rektnet_head.hip (cross_ratio_loss.py:36-55)
  constexpr int DQ_A[9] = {5, 3, 1, 6, 4, 2, 2, 4, 6};
  constexpr int DQ_B[9] = {3, 1, 0, 4, 2, 0, 1, 3, 5};
  constexpr int TERM_U[6] = {1, 2, 3, 4, 7, 8};       // vA vB vC vD hA hB
  constexpr int TERM_V[6] = {0, 1, 4, 5, 6, 7};
  float p[14], t[14];
#pragma unroll
  for (int c = 0; c < 14; ++c) { p[c] = P[c]; t[c] = Tg[c]; }
  double loc = loc_hm;
  if (loss_type != 1) {
    loc = 0.0;
#pragma unroll
    for (int c = 0; c < 14; ++c) { const float d = p[c] - t[c]; loc += (double)(loss_type == 0 ? d * d : fabsf(d)); }
  }
  double geo = 0.0;
  if (include_geo) {
    float ux[9], uy[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const float dx = p[2 * DQ_A[q]] - p[2 * DQ_B[q]], dy = p[2 * DQ_A[q] + 1] - p[2 * DQ_B[q] + 1];
      const float nrm = fmaxf(sqrtf(dx * dx + dy * dy), 1e-12f);         // F.normalize eps: coincident points give the zero vector
      ux[q] = dx / nrm; uy[q] = dy / nrm;
    }
    const double wv = (double)gamma_v / 4.0, wh = (double)gamma_h / 2.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int u = TERM_U[k], v = TERM_V[k];
      const double dot = (double)ux[u] * (double)ux[v] + (double)uy[u] * (double)uy[v];
      geo += (k < 4 ? wv : wh) * (1.0 - dot);
    }
  }
  float o[MDCV_KPT_EVAL_ROW];
  o[0] = (float)loc; o[1] = (float)geo; o[2] = (float)(loc + geo);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const float ex = dist_sx * (p[2 * k] - t[2 * k]), ey = dist_sy * (p[2 * k + 1] - t[2 * k + 1]);
    o[3 + k] = (float)sqrt((double)ex * (double)ex + (double)ey * (double)ey);
  }
  o[10] = 0.f; o[11] = 0.f;
  float4* dst = reinterpret_cast<float4*>(row);        // 48-byte rows of a 16-byte aligned buffer
  dst[0] = float4{o[0], o[1], o[2], o[3]};
  dst[1] = float4{o[4], o[5], o[6], o[7]};
  dst[2] = float4{o[8], o[9], o[10], o[11]};
}

// loss types 0 and 2: the heat-maps are never touched.  One thread per sample.
__global__ __launch_bounds__(256) void kpt_eval_pts_kernel(const float* __restrict__ pts, const float* __restrict__ tpts, int B, int loss_type,
                                                           int include_geo, float gamma_h, float gamma_v, float dist_sx, float dist_sy,
                                                           float* __restrict__ rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  eval_points_row(pts + (size_t)i * 14, tpts + (size_t)i * 14, loss_type, include_geo, gamma_h, gamma_v, dist_sx, dist_sy, 0.0,
                  rows + (size_t)i * MDCV_KPT_EVAL_ROW);
}

// loss type 1: one workgroup per sample streams its n = 7 H W floats of hm and thm once (HBM-bound: 8 n bytes per sample).
// The sample is cut into groups of four floats by INDEX, g = j / 4, G = n / 4 whole groups.  Groups 1 .. G-2 are the vector part
// (hm_vector_part).  Group 0, group G-1 and the n % 4 floats behind it are the scalar head and tail, added by thread 0 behind its vector groups:
// they are what a 16-byte load at a phase != 0 would reach out of the sample for.  The phase of a sample's first float only decides HOW a
// group's floats are loaded, never which thread adds them or when.
__global__ __launch_bounds__(256) void kpt_eval_hm_kernel(const float* __restrict__ hm, const float* __restrict__ pts, const float* __restrict__ thm,
                                                          const float* __restrict__ tpts, int n, int include_geo, float gamma_h, float gamma_v,
                                                          float dist_sx, float dist_sy, float* __restrict__ rows) {
  __shared__ double red[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* a = hm + (size_t)i * n;
  const float* b = thm + (size_t)i * n;
  const int sa = phase4(a), sb = phase4(b);
  const int G = n >> 2;
  double acc = (sa | sb) == 0 ? hm_vector_part<true, 8>(a, b, 0, 0, G, tid) : hm_vector_part<false, 4>(a, b, sa, sb, G, tid);
  if (tid == 0) {
    const int head = n < 4 ? n : 4, tail = 4 * (G - 1) > 4 ? 4 * (G - 1) : 4;
    for (int j = 0; j < head; ++j) { const float d = a[j] - b[j]; acc += (double)(d * d); }
    for (int j = tail; j < n; ++j) { const float d = a[j] - b[j]; acc += (double)(d * d); }
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)
    eval_points_row(pts + (size_t)i * 14, tpts + (size_t)i * 14, 1, include_geo, gamma_h, gamma_v, dist_sx, dist_sy,
                    red[0] + red[1] + red[2] + red[3], rows + (size_t)i * MDCV_KPT_EVAL_ROW);
}

}  // namespace

extern "C" {

// Per-sample validation rows of a batch; the contract is in include/mdcv_hip.h.  Every refusal comes before any HIP call.
int mdcv_kpt_eval_rows(const float* hm, const float* pts, const float* thm, const float* tpts, int B, int H, int W, int loss_type,
                       int include_geo, float gamma_horz, float gamma_vert, float dist_sx, float dist_sy, float* rows, void* stream) {
  if (!pts || !tpts || !rows || B < 1 || B > 65535 || loss_type < 0 || loss_type > 2) return MDCV_EARG;
  if (reinterpret_cast<uintptr_t>(rows) & 15) return MDCV_EARG;                       // the rows are written with 16-byte stores
  hipStream_t st = (hipStream_t)stream;
  if (loss_type == 1) {
    if (!hm || !thm || H < 1 || W < 1 || 7LL * H * W > INT_MAX) return MDCV_EARG;
    MDCV_LAUNCH(kpt_eval_hm_kernel, dim3((unsigned)B), dim3(256), 0, st, hm, pts, thm, tpts, 7 * H * W, include_geo, gamma_horz, gamma_vert,
                dist_sx, dist_sy, rows);
  } else {
    MDCV_LAUNCH(kpt_eval_pts_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, pts, tpts, B, loss_type, include_geo, gamma_horz,
                gamma_vert, dist_sx, dist_sy, rows);
  }
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
