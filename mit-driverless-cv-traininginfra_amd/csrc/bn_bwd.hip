// BatchNorm(+activation) backward for gfx950: pass 1 reduces the per-channel sums to partial rows, pass 2 applies dy = cA*g + cB*y + cC.
// Strip kernels: see strip.h.  The rows are summed and finalized by col_reduce.hip.
#include "strip.h"

namespace {

// backward, pass 1: g = dout * act'(pre);  accum += [sum g, sum g*xhat1, (sum g*xhat2)]   (fp64 atomics, one per channel per block)
struct BnBwdArgs {
  const void* dout; const void* y1; const void* y2; void* dy1; void* dy2;
  const float* s1; const float* b1; const float* m1; const float* is1;
  const float* s2; const float* b2; const float* m2; const float* is2;
  const float* cA1; const float* cB1; const float* cC1; const float* cA2; const float* cB2; const float* cC2;
  double* accum; float* partial;            // (accum: read by no kernel, left null; it stays for the kernels' argument layout)
  int ldd, ld1, ld2, ldy1, ldy2, M, C, act, PB, CV, PPI;
  float slope;
};
// VEC consecutive fp32 sums as 16-byte stores
template <int VEC>
__device__ __forceinline__ void store_row(float* dst, const float (&v)[VEC]) {
  *reinterpret_cast<uint4*>(dst) = ET<float>::pack(v);
  if constexpr (VEC == 8) *reinterpret_cast<uint4*>(dst + 4) = ET<float>::pack(v + 4);
}
template <typename T, bool DUAL>     // DUAL: see bn_act_bwd_apply_kernel
__global__ __launch_bounds__(256) void bn_act_bwd_reduce_kernel(BnBwdArgs a) {
  constexpr int VEC = ET<T>::VEC;
  constexpr int ND = DUAL ? VEC : 1;
  __shared__ float red[256 * VEC];
  const int tid = threadIdx.x;
  const bool active = tid < a.PPI * a.CV;
  const int cv = active ? tid % a.CV : 0, pi = active ? tid / a.CV : 0;
  constexpr int nsum = DUAL ? 3 : 2;
  float s1[VEC], b1[VEC], m1[VEC], i1[VEC], s2[ND], b2[ND], m2[ND], i2[ND];
  ldcoef<VEC>(a.s1, cv * VEC, s1, 1.f); ldcoef<VEC>(a.b1, cv * VEC, b1, 0.f); ldcoef<VEC>(a.m1, cv * VEC, m1, 0.f); ldcoef<VEC>(a.is1, cv * VEC, i1, 0.f);
  if constexpr (DUAL) {
    ldcoef<VEC>(a.s2, cv * VEC, s2, 0.f); ldcoef<VEC>(a.b2, cv * VEC, b2, 0.f);
    ldcoef<VEC>(a.m2, cv * VEC, m2, 0.f); ldcoef<VEC>(a.is2, cv * VEC, i2, 0.f);
  }
  float sg[VEC], sx1[VEC], sx2[ND];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { sg[e] = 0.f; sx1[e] = 0.f; }
#pragma unroll
  for (int e = 0; e < ND; ++e) sx2[e] = 0.f;
  const long long p0 = (long long)blockIdx.x * a.PB;
  const long long p1 = min((long long)a.M, p0 + a.PB);
  const T* dout = reinterpret_cast<const T*>(a.dout);
  const T* y1 = reinterpret_cast<const T*>(a.y1);
  const T* y2 = reinterpret_cast<const T*>(a.y2);
  if (active)
    for (long long pb = p0 + pi; pb < p1; pb += 4 * a.PPI) {
      uint4 qd[4], qv[4], qw[DUAL ? 4 : 1];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                     // issue all loads of 4 pixels before touching any
        const long long p = pb + (long long)u * a.PPI;
        if (p < p1) {
          qd[u] = *reinterpret_cast<const uint4*>(dout + p * a.ldd + cv * VEC);
          qv[u] = *reinterpret_cast<const uint4*>(y1 + p * a.ld1 + cv * VEC);
          if constexpr (DUAL) qw[u] = *reinterpret_cast<const uint4*>(y2 + p * a.ld2 + cv * VEC);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
      if (pb + (long long)u * a.PPI >= p1) break;
      float d[VEC], v[VEC], w[ND];
      ET<T>::unpack(qd[u], d);
      ET<T>::unpack(qv[u], v);
      if constexpr (DUAL) ET<T>::unpack(qw[u], w);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float pre = v[e] * s1[e] + b1[e];
        if constexpr (DUAL) pre += w[e] * s2[e] + b2[e];
        const float g = d[e] * act_grad(pre, a.act, a.slope);
        sg[e] += g;
        sx1[e] += g * (v[e] - m1[e]) * i1[e];
        if constexpr (DUAL) sx2[e] += g * (w[e] - m2[e]) * i2[e];
      }
      }
    }
  // fold the PPI pixel-lanes that share a channel vector; one partial row [nsum][C] per block (summed by partial_reduce)
  float* prow = a.partial + (size_t)blockIdx.x * nsum * a.C;
  block_fold<VEC>(sg, a.CV, red, tid);
  if (tid < a.CV) store_row<VEC>(prow + tid * VEC, sg);
  block_fold<VEC>(sx1, a.CV, red, tid);
  if (tid < a.CV) store_row<VEC>(prow + a.C + tid * VEC, sx1);
  if constexpr (DUAL) {
    block_fold<VEC>(sx2, a.CV, red, tid);
    if (tid < a.CV) store_row<ND>(prow + 2 * a.C + tid * VEC, sx2);
  }
}

// backward, pass 2: dy_i = cA_i*g + cB_i*y_i + cC_i
// DUAL: two BatchNorms feed one activation (RektNet's residual blocks).  A template parameter, not a runtime test of y2: the single form
// then carries 40 coefficient registers instead of 80 (214 -> ~120 VGPRs), so four blocks fit on a CU instead of two -- the kernel shares
// the chip with the side stream's weight gradients, whose blocks leave no registers on the CUs they occupy.
template <typename T, bool DUAL>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(BnBwdArgs a) {
  constexpr int VEC = ET<T>::VEC;
  constexpr int ND = DUAL ? VEC : 1;
  const int tid = threadIdx.x;
  if (tid >= a.PPI * a.CV) return;
  const int cv = tid % a.CV, pi = tid / a.CV;
  float s1[VEC], b1[VEC], A1[VEC], B1[VEC], C1[VEC], s2[ND], b2[ND], A2[ND], B2[ND], C2[ND];
  ldcoef<VEC>(a.s1, cv * VEC, s1, 1.f); ldcoef<VEC>(a.b1, cv * VEC, b1, 0.f);
  ldcoef<VEC>(a.cA1, cv * VEC, A1, 0.f); ldcoef<VEC>(a.cB1, cv * VEC, B1, 0.f); ldcoef<VEC>(a.cC1, cv * VEC, C1, 0.f);
  if constexpr (DUAL) {
    ldcoef<VEC>(a.s2, cv * VEC, s2, 0.f); ldcoef<VEC>(a.b2, cv * VEC, b2, 0.f);
    ldcoef<VEC>(a.cA2, cv * VEC, A2, 0.f); ldcoef<VEC>(a.cB2, cv * VEC, B2, 0.f); ldcoef<VEC>(a.cC2, cv * VEC, C2, 0.f);
  }
  const long long p0 = (long long)blockIdx.x * a.PB;
  const long long p1 = min((long long)a.M, p0 + a.PB);
  const T* dout = reinterpret_cast<const T*>(a.dout);
  const T* y1 = reinterpret_cast<const T*>(a.y1);
  const T* y2 = reinterpret_cast<const T*>(a.y2);
  T* dy1 = reinterpret_cast<T*>(a.dy1);
  T* dy2 = reinterpret_cast<T*>(a.dy2);
  for (long long pb = p0 + pi; pb < p1; pb += 4 * a.PPI) {
    uint4 qd[4], qv[4], qw[DUAL ? 4 : 1];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long p = pb + (long long)u * a.PPI;
      if (p < p1) {
        qd[u] = ld_stream(dout + p * a.ldd + cv * VEC);
        qv[u] = ld_stream(y1 + p * a.ld1 + cv * VEC);
        if constexpr (DUAL) qw[u] = ld_stream(y2 + p * a.ld2 + cv * VEC);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long p = pb + (long long)u * a.PPI;
      if (p >= p1) break;
      float d[VEC], v[VEC], w[ND], o1[VEC], o2[ND];
      ET<T>::unpack(qd[u], d);
      ET<T>::unpack(qv[u], v);
      if constexpr (DUAL) ET<T>::unpack(qw[u], w);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if constexpr (!DUAL) {
          o1[e] = mdcv_bn_bwd_dy(d[e], v[e], s1[e], b1[e], A1[e], B1[e], C1[e], a.act, a.slope);     // (shared with the operand-load forms: bit-identical)
        } else {
          float pre = v[e] * s1[e] + b1[e];
          pre += w[e] * s2[e] + b2[e];
          const float g = d[e] * act_grad(pre, a.act, a.slope);
          o1[e] = A1[e] * g + B1[e] * v[e] + C1[e];
          o2[e] = A2[e] * g + B2[e] * w[e] + C2[e];
        }
      }
      *reinterpret_cast<uint4*>(dy1 + p * a.ldy1 + cv * VEC) = ET<T>::pack(o1);
      if constexpr (DUAL) *reinterpret_cast<uint4*>(dy2 + p * a.ldy2 + cv * VEC) = ET<T>::pack(o2);
    }
  }
}

}  // namespace

// Pass 1 of the BN(+act) backward, shared by the two entry points below: block i stores the partial row partial_ws[i][nsums][C] with
// [0] = sum g, [1] = sum g*xhat1 and, with a second BatchNorm (y2), [2] = sum g*xhat2.  *rows: the number of rows written.
static int launch_bwd_reduce(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1, const float* mean1,
                             const float* invstd1, const void* y2, int ld2, const float* s2, const float* b2, const float* mean2,
                             const float* invstd2, float* partial_ws, int M, int C, int act, float slope, hipStream_t st, int* rows) {
  BnBwdArgs a = {};
  a.dout = dout; a.y1 = y1; a.y2 = y2; a.s1 = s1; a.b1 = b1; a.m1 = mean1; a.is1 = invstd1; a.s2 = s2; a.b2 = b2; a.m2 = mean2; a.is2 = invstd2;
  a.partial = partial_ws; a.ldd = ldd; a.ld1 = ld1; a.ld2 = ld2;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const Strip s = make_strip<T>(M, C, kReduceBlocks, 8);
    if (s.CV > 256 || (256 % s.CV)) return MDCV_EARG;
    fill_strip(a, s, M, C, act, slope);
    *rows = cdiv(M, s.PB);
    if (a.y2) MDCV_LAUNCH((bn_act_bwd_reduce_kernel<T, true>), dim3((unsigned)*rows), dim3(256), 0, st, a);
    else MDCV_LAUNCH((bn_act_bwd_reduce_kernel<T, false>), dim3((unsigned)*rows), dim3(256), 0, st, a);
    return MDCV_OK;
  });
}

extern "C" {

// floats of scratch mdcv_bn_act_bwd_reduce needs (one [nsums][C] partial row per block)
int mdcv_bn_act_bwd_reduce_ws_floats(int dtype, int M, int C, int nsums) {
  const Strip s = dtype == MDCV_BF16 ? make_strip<bf16_t>(M, C, kReduceBlocks, 8) : make_strip<float>(M, C, kReduceBlocks, 8);
  return cdiv(M, s.PB) * nsums * C;
}

// pass 1 of the BN(+act) backward: accum[0] += sum g ; accum[1] += sum g*xhat1 ; accum[2] += sum g*xhat2 (if y2)
int mdcv_bn_act_bwd_reduce(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1,
                           const float* mean1, const float* invstd1, const void* y2, int ld2, const float* s2, const float* b2,
                           const float* mean2, const float* invstd2, double* accum, float* partial_ws, int M, int C, int act, float slope,
                           void* stream) {
  if (!dout || !y1 || !accum || !partial_ws || (C & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  int rows = 0;
  const int rc = launch_bwd_reduce(dtype, dout, ldd, y1, ld1, s1, b1, mean1, invstd1, y2, ld2, s2, b2, mean2, invstd2, partial_ws, M, C, act, slope,
                                   st, &rows);
  if (rc != MDCV_OK) return rc;
  return launch_partial_reduce(partial_ws, rows, (y2 ? 3 : 2) * C, accum, st);
}

// pass 1 of the BN(+act) backward including the finalize: partial rows -> (dgamma, dbeta, cA, cB, cC) of one or two BatchNorms
// in the same launch sequence (main reduce kernel + one column-owner kernel; no atomics).
int mdcv_bn_act_bwd_reduce_finalize(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1,
                                    const float* mean1, const float* invstd1, const void* y2, int ld2, const float* s2, const float* b2,
                                    const float* mean2, const float* invstd2, float* partial_ws, int M, int C, int act, float slope,
                                    double count, const float* gamma1, float* dgamma1, float* dbeta1, float* cA1, float* cB1, float* cC1,
                                    const float* gamma2, float* dgamma2, float* dbeta2, float* cA2, float* cB2, float* cC2, void* stream) {
  if (!dout || !y1 || !partial_ws || (C & 7) || !gamma1 || !dgamma1 || !dbeta1 || !cA1 || !cB1 || !cC1 || !mean1 || !invstd1) return MDCV_EARG;
  if (y2 && (!gamma2 || !dgamma2 || !dbeta2 || !cA2 || !cB2 || !cC2 || !mean2 || !invstd2)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  int rows = 0;
  const int rc = launch_bwd_reduce(dtype, dout, ldd, y1, ld1, s1, b1, mean1, invstd1, y2, ld2, s2, b2, mean2, invstd2, partial_ws, M, C, act, slope,
                                   st, &rows);
  if (rc != MDCV_OK) return rc;
  return launch_bn_colfinal_bwd(partial_ws, rows, y2 ? 3 : 2, C, count, {gamma1, mean1, invstd1, dgamma1, dbeta1, cA1, cB1, cC1},
                                {gamma2, mean2, invstd2, dgamma2, dbeta2, cA2, cB2, cC2}, st);
}

int mdcv_bn_act_bwd_apply(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1,
                          const float* cA1, const float* cB1, const float* cC1, void* dy1, int ldy1,
                          const void* y2, int ld2, const float* s2, const float* b2, const float* cA2, const float* cB2,
                          const float* cC2, void* dy2, int ldy2, int M, int C, int act, float slope, void* stream) {
  if (!dout || !y1 || !dy1 || (C & 7)) return MDCV_EARG;
  BnBwdArgs a = {};
  a.dout = dout; a.y1 = y1; a.y2 = y2; a.dy1 = dy1; a.dy2 = dy2; a.s1 = s1; a.b1 = b1; a.s2 = s2; a.b2 = b2;
  a.cA1 = cA1; a.cB1 = cB1; a.cC1 = cC1; a.cA2 = cA2; a.cB2 = cB2; a.cC2 = cC2;
  a.ldd = ldd; a.ld1 = ld1; a.ld2 = ld2; a.ldy1 = ldy1; a.ldy2 = ldy2;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const Strip s = make_strip<T>(M, C, 2048, 4);
    if (s.CV > 256) return MDCV_EARG;
    fill_strip(a, s, M, C, act, slope);
    const dim3 grid((unsigned)cdiv(M, s.PB));
    if (a.y2) MDCV_LAUNCH((bn_act_bwd_apply_kernel<T, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else MDCV_LAUNCH((bn_act_bwd_apply_kernel<T, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    return MDCV_OK;
  });
}

}  // extern "C"
