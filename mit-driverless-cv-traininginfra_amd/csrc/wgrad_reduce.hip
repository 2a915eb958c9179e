// Weight-gradient slab reduce: every weight-gradient kernel of the conv family (wgrad_gemm.hip, wgrad_shift.hip, wgrad_stream.hip, wgrad_stream_s2.hip)
// writes fp32 slabs ws[split][Cout_pad][KK*Cin_pad]; the kernels here sum them over the splits into the OIHW fp32 gradient of the real channels.
#include "common.h"
#include "wgrad_gemm.h"

namespace {

// slabs -> OIHW fp32 gradient (real Cin, i.e. without channel padding).
// One block per (co, chunk of 64 input channels): slab rows [tap][ci] are read coalesced along ci and summed over the
// splits, transposed through LDS, and written as the contiguous OIHW run [ci0..ci0+63][tap].
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int splits, int Cout_pad,
                                                           int Cin_real, int Cin_pad, int KK, int Ktot, int accumulate) {
  extern __shared__ float tile[];                       // [KK][65]
  const int co = blockIdx.x, ci0 = blockIdx.y * 64;
  const int nci = min(64, Cin_real - ci0);
  const size_t slab = (size_t)Cout_pad * Ktot;
  const float* row = ws + (size_t)co * Ktot;
  for (int i = threadIdx.x; i < KK * 64; i += 256) {
    const int t = i >> 6, c = i & 63;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;       // 4 independent chains: the loads of 4 splits are in flight together
    if (c < nci) {
      const float* p = row + t * Cin_pad + ci0 + c;
      int sp = 0;
      for (; sp + 4 <= splits; sp += 4) {
        s0 += p[(size_t)sp * slab]; s1 += p[(size_t)(sp + 1) * slab]; s2 += p[(size_t)(sp + 2) * slab]; s3 += p[(size_t)(sp + 3) * slab];
      }
      for (; sp < splits; ++sp) s0 += p[(size_t)sp * slab];
    }
    tile[t * 65 + c] = (s0 + s1) + (s2 + s3);
  }
  __syncthreads();
  float* out = dw + ((size_t)co * Cin_real + ci0) * KK;
  for (int i = threadIdx.x; i < nci * KK; i += 256) {
    const int c = i / KK, t = i - c * KK;
    const float v = tile[t * 65 + c];
    out[i] = accumulate ? out[i] + v : v;
  }
}

// Same reduction with the loads spread out: thread (c = tid & 63, q = tid >> 6) sums the splits s = q, q+4, ... of all KK taps of
// input channel c (KK independent loads per split, several splits unrolled), so a block has ~4*KK*unroll loads in flight per
// thread group instead of four dependent chains; the four partial sums meet in LDS.  (The chained version was latency-bound:
// 25 us per layer, 1.9 ms per YOLOv3 step.)
template <int KK>
__global__ __launch_bounds__(256) void wgrad_reduce_kk_kernel(const float* __restrict__ ws, float* __restrict__ dw, int splits, int Cout_pad,
                                                              int Cin_real, int Cin_pad, int Ktot, int accumulate) {
  __shared__ float tile[4][KK][65];
  const int co = blockIdx.x, ci0 = blockIdx.y * 64;
  const int nci = min(64, Cin_real - ci0);
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const size_t slab = (size_t)Cout_pad * Ktot;
  float acc[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) acc[t] = 0.f;
  if (c < nci) {
    const float* p = ws + (size_t)co * Ktot + ci0 + c;
#pragma unroll 4
    for (int sp = q; sp < splits; sp += 4) {
      const float* ps = p + (size_t)sp * slab;
#pragma unroll
      for (int t = 0; t < KK; ++t) acc[t] += __builtin_nontemporal_load(ps + t * Cin_pad);   // the slabs' only reader (strip.h: ld_stream; 13.11 / 13.09 -> 13.05 / 13.07 ms)
    }
  }
#pragma unroll
  for (int t = 0; t < KK; ++t) tile[q][t][c] = acc[t];
  __syncthreads();
  float* out = dw + ((size_t)co * Cin_real + ci0) * KK;
  for (int i = threadIdx.x; i < nci * KK; i += 256) {
    const int cc = i / KK, t = i - cc * KK;
    const float v = (tile[0][t][cc] + tile[1][t][cc]) + (tile[2][t][cc] + tile[3][t][cc]);
    out[i] = accumulate ? out[i] + v : v;
  }
}

// Slab reduce for SMALL layers (Cout * ceil(Cin/64) < 128 blocks in the kernel above: RektNet's 16..64-channel layers took 13-25 us
// there, most of it idle lanes and serial split loops).  One thread per slab element k (coalesced), 16 split groups per block
// with 8 loads in flight each, fixed-order tree in LDS -> deterministic.  Grid (ceil(Ktot/64), Cout_real).
__global__ __launch_bounds__(1024) void wgrad_reduce_flat_kernel(const float* __restrict__ ws, float* __restrict__ dw, int splits, int Cout_pad,
                                                                 int Cin_real, int Cin_pad, int KK, int Ktot, int accumulate) {
  __shared__ float part[16][64];
  const int co = blockIdx.y, c = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + c;
  const size_t slab = (size_t)Cout_pad * Ktot;
  float acc = 0.f;
  if (k < Ktot) {
    const float* p = ws + (size_t)co * Ktot + k;
    int sp = sg;
    for (; sp + 112 < splits; sp += 128) {                 // 8 independent loads in flight
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(p + (size_t)(sp + 16 * u) * slab);
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; sp < splits; sp += 16) acc += __builtin_nontemporal_load(p + (size_t)sp * slab);
  }
  part[sg][c] = acc;
  __syncthreads();
  if (sg == 0 && k < Ktot) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = part[u][c];
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
      for (int u = 0; u < w; ++u) v[u] += v[u + w];
    const int t = k / Cin_pad, ci = k - t * Cin_pad;
    if (ci < Cin_real) {
      float* out = dw + ((size_t)co * Cin_real + ci) * KK + t;
      *out = accumulate ? *out + v[0] : v[0];
    }
  }
}
}  // namespace

// sums the fp32 slabs ws[splits][Cout_pad][KK*Cin_pad] into the OIHW gradient
int launch_wgrad_reduce(const float* ws, float* dw_oihw, int splits, int Cout_pad, int Cout_real, int Cin_pad, int Cin_real, int KK,
                        int accumulate, hipStream_t st) {
  const int Ktot = KK * Cin_pad;
  if (Cout_real * cdiv(Cin_real, 64) < 128) {
    MDCV_LAUNCH(wgrad_reduce_flat_kernel, dim3((unsigned)cdiv(Ktot, 64), (unsigned)Cout_real), dim3(1024), 0, st, ws, dw_oihw, splits,
                       Cout_pad, Cin_real, Cin_pad, KK, Ktot, accumulate);
  } else {
    const dim3 rgrid((unsigned)Cout_real, (unsigned)cdiv(Cin_real, 64));
    if (KK == 9) MDCV_LAUNCH(wgrad_reduce_kk_kernel<9>, rgrid, dim3(256), 0, st, ws, dw_oihw, splits, Cout_pad, Cin_real, Cin_pad, Ktot, accumulate);
    else if (KK == 1) MDCV_LAUNCH(wgrad_reduce_kk_kernel<1>, rgrid, dim3(256), 0, st, ws, dw_oihw, splits, Cout_pad, Cin_real, Cin_pad, Ktot, accumulate);
    else MDCV_LAUNCH(wgrad_reduce_kernel, rgrid, dim3(256), KK * 65 * 4, st, ws, dw_oihw, splits, Cout_pad, Cin_real, Cin_pad, KK, Ktot, accumulate);
  }
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

extern "C" int mdcv_wgrad_reduce(const float* ws, int splits, float* dw_oihw, int accumulate, int Cout_pad, int Cout, int Cin_pad, int Cin, int KK,
                                 void* stream) {
  if (!ws || !dw_oihw || splits < 1 || Cout < 1 || Cin < 1 || Cout > Cout_pad || Cin > Cin_pad || KK < 1) return MDCV_EARG;
  return launch_wgrad_reduce(ws, dw_oihw, splits, Cout_pad, Cout, Cin_pad, Cin, KK, accumulate, (hipStream_t)stream);
}
