// The device restatement of RektNet/utils.py:83-97 `prep_label`, shared by the synthetic crop generator (synth.hip) and the real-crop
// loader (kptload.hip): a one-hot at (int(y), int(x)) of the ORIGINAL crop -> cv2.resize (INTER_LINEAR, float64) -> 5x5 cv2.GaussianBlur
// (sigma 0: [1, 4, 6, 4, 1] / 16, BORDER_REFLECT_101) -> divided by its sum.  The resized, blurred one-hot is separable, so a heat-map is
// the outer product of two S-vectors; both are float64 like cv2's, the sums run sequentially in index order, the total is sum_y * sum_x
// and a value is (float)(vy[y] * vx[x] / tot).  oracle/synth_oracle.py (_resize_onehot_axis, _blur_reflect101, cone_crops) is the numpy
// side and agrees bit for bit; units that include this header are built with -ffp-contract=off for that reason.
// A down-scaled one-hot that no tap reads gives tot == 0 and an all-NaN map (0 / 0), as the reference does.
#pragma once
#include "common.h"

namespace kpthm {

__device__ __forceinline__ double resize_onehot(int d, int hot, int src, int dst) {   // cv2 INTER_LINEAR sample d of a one-hot at `hot`
  const double sc = (double)src / (double)dst;
  float fx = (float)(((double)d + 0.5) * sc - 0.5);
  int sx = (int)floorf(fx);
  fx = fx - (float)sx;
  if (sx < 0) { sx = 0; fx = 0.f; }
  if (sx >= src - 1) { sx = src - 1; fx = 0.f; }
  const int s1 = sx + 1 < src ? sx + 1 : src - 1;
  const double f = (double)fx;
  return (1.0 - f) * (sx == hot ? 1.0 : 0.0) + f * (s1 == hot ? 1.0 : 0.0);
}

// The two vectors and their sums for nk key points of one crop, by all nt threads of a workgroup (ends with a barrier).
//   hot[k * 2 + a]: the hot pixel of key point k on axis a (0: x, 1: y); ow, oh: the original crop's width and height
//   rz, bl: LDS, 2 * nk * S doubles each, indexed [(a * nk + k) * S + d]; bl holds the blurred vectors afterwards
//   sums:   LDS, 2 * nk doubles, [a * nk + k]; the total of map k is sums[nk + k] * sums[k]  (sum_y * sum_x)
__device__ __forceinline__ void axes(double* rz, double* bl, double* sums, const int* hot, int nk, int ow, int oh, int S, int tid, int nt) {
  for (int i = tid; i < 2 * nk * S; i += nt) {
    const int a = i / (nk * S), r = i - a * nk * S, k = r / S, d = r - k * S;
    rz[i] = resize_onehot(d, hot[k * 2 + a], a == 0 ? ow : oh, S);
  }
  __syncthreads();
  for (int i = tid; i < 2 * nk * S; i += nt) {
    const int d = i % S;
    const double* v = rz + (i - d);
    const double g[5] = {1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0};
    double acc = 0.0;
#pragma unroll
    for (int t = -2; t <= 2; ++t) {
      int j = d + t;
      if (j < 0) j = -j;
      if (j >= S) j = 2 * (S - 1) - j;                                          // BORDER_REFLECT_101
      acc += g[t + 2] * v[j];
    }
    bl[i] = acc;
  }
  __syncthreads();
  if (tid < 2 * nk) {
    const double* v = bl + tid * S;
    double s = 0.0;
    for (int d = 0; d < S; ++d) s += v[d];
    sums[tid] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ float value(double vy, double vx, double tot) { return (float)((vy * vx) / tot); }

// nk maps [nk][S][S] fp32 from axes()' tables.  vec: S % 4 == 0 and hm 16-byte aligned -> one 16-byte store per four x.
__device__ __forceinline__ void store(float* __restrict__ hm, const double* bl, const double* sums, int nk, int S, int tid, int nt, bool vec) {
  if (vec) {
    const int S4 = S >> 2;
    for (int i = tid; i < nk * S * S4; i += nt) {
      const int k = i / (S * S4), r = i - k * S * S4, y = r / S4, x = (r - y * S4) * 4;
      const double tot = sums[nk + k] * sums[k], vy = bl[(nk + k) * S + y];
      const double* vx = bl + k * S + x;
      const f32x4_t o = {value(vy, vx[0], tot), value(vy, vx[1], tot), value(vy, vx[2], tot), value(vy, vx[3], tot)};
      *reinterpret_cast<f32x4_t*>(hm + (size_t)i * 4) = o;
    }
  } else {
    for (int i = tid; i < nk * S * S; i += nt) {
      const int k = i / (S * S), r = i - k * S * S, y = r / S, x = r - y * S;
      hm[i] = value(bl[(nk + k) * S + y], bl[k * S + x], sums[nk + k] * sums[k]);
    }
  }
}

}  // namespace kpthm
