// Shared host / device helpers of the HBM-bound NHWC elementwise and per-channel-reduction units for gfx950: layout.hip, bn_fwd.hip,
// bn_bwd.hip, col_reduce.hip and pool_upsample.hip.  Internal: not part of the C ABI.
//
// These units replace nn.BatchNorm2d (train + eval), nn.LeakyReLU / nn.ReLU, the shortcut add, nn.MaxPool2d, nn.Upsample(nearest) and
// their autograd backward on the reference hot path (CVC-YOLOv3/models.py:66-71,74-88,325-327; RektNet/resnet.py:22-27, keypoint_net.py:59).
//
// The BatchNorm and column-sum kernels are "strip" kernels: a block owns a contiguous strip of pixels, a thread owns one 16-byte channel
// vector (8 bf16 / 4 fp32) and walks down the strip, so every access is a coalesced 16-byte load/store and per-channel reductions stay in
// registers until one LDS fold and one partial row per block.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- launches that cross units (the kernels live in col_reduce.hip)
// partial[rows][cols] (fp32) added to accum[cols] (fp64)
int launch_partial_reduce(const float* partial, int rows, int cols, double* accum, hipStream_t st);
// one BatchNorm of the backward: what the column-owner finalize reads (gamma, mean, invstd) and writes (dgamma, dbeta, cA, cB, cC)
struct BnBwdCoefs {
  const float* gamma; const float* mean; const float* invstd;
  float* dgamma; float* dbeta; float* cA; float* cB; float* cC;
};
// partial[rows][nsums][C] of bn_act_bwd_reduce_kernel -> the coefficients of one (nsums == 2) or two (nsums == 3) BatchNorms
int launch_bn_colfinal_bwd(const float* partial, int rows, int nsums, int C, double count, const BnBwdCoefs& bn1, const BnBwdCoefs& bn2,
                           hipStream_t st);

// ---------------------------------------------------------------- host helpers
// The one launch path per element type: f(T{}), T = bf16_t or float, checks what depends on T, launches and returns MDCV_OK, or returns an
// error with nothing launched; the launch error, if any, is picked up here.  Any other dtype is an argument error.
template <typename F> static int launch_by_dtype(int dtype, F&& f) {
  const int rc = dtype == MDCV_BF16 ? f(bf16_t{}) : dtype == MDCV_F32 ? f(float{}) : MDCV_EARG;
  if (rc != MDCV_OK) return rc;
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

static unsigned ew_grid(long long total) {
  long long g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (unsigned)g;
}

struct Strip {
  int CV, PPI, PB;   // vectors per pixel, pixels per block-iteration, pixels per block
};
template <typename T> static Strip make_strip(int M, int C, int target_blocks, int min_iters = 1) {
  Strip s;
  s.CV = C / ET<T>::VEC;
  s.PPI = 256 / s.CV; if (s.PPI < 1) s.PPI = 1;
  long long pb = ((long long)M + target_blocks - 1) / target_blocks;
  pb = ((pb + s.PPI - 1) / s.PPI) * s.PPI;
  if (pb < (long long)s.PPI * min_iters) pb = (long long)s.PPI * min_iters;   // amortise the per-block prologue / fold
  s.PB = (int)pb;
  return s;
}

// reduction kernels store one partial row per block (no atomics): the cap is on the rows the follow-up tree reduce has to read
constexpr int kReduceBlocks = 1024;

// the fields BnActArgs and BnBwdArgs share: problem size, activation (ReLU, act 2, is a leaky ReLU of slope 0) and the strip
template <typename A> static void fill_strip(A& a, const Strip& s, int M, int C, int act, float slope) {
  a.M = M; a.C = C; a.act = act; a.slope = act == 2 ? 0.f : slope;
  a.PB = s.PB; a.CV = s.CV; a.PPI = s.PPI;
}

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ uint4 ld_stream(const void* p) { return mdcv_ld_stream(p); }     // (common.h: non-temporal 16-byte load of a last-use operand)

// flat index of a grid-stride kernel over [B][Hd][Wd][CV] -> channel vector cv, pixel pix = (b * Hd + h) * Wd + w and its coordinates
__device__ __forceinline__ void decode_pixel(long long i, int CV, int Wd, int Hd, int& cv, long long& pix, int& w, int& h, int& b) {
  cv = (int)(i % CV);
  pix = i / CV;
  w = (int)(pix % Wd);
  const long long t = pix / Wd;
  h = (int)(t % Hd); b = (int)(t / Hd);
}

// fold the per-thread channel-vector sums of a block: lanes that own the same channel vector are CV apart.
// Requires 256 % CV == 0.  red: 256*VEC floats.  Result: threads tid < CV hold the block total for vector tid in v[].
template <int VEC>
__device__ __forceinline__ void block_fold(float (&v)[VEC], int CV, float* red, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  if (CV < 64) {
    for (int off = 32; off >= CV; off >>= 1) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[e] += __shfl_xor(v[e], off, 64);
    }
  }
  const int span = CV < 64 ? CV : 64;
  __syncthreads();
  if (lane < span) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[(wave * 64 + lane) * VEC + e] = v[e];
  }
  __syncthreads();
  if (tid < CV) {
    float s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.f;
    for (int w = 0; w < 4; ++w) {
      if (CV > 64 && ((w * 64) % CV) != (tid & ~63)) continue;
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] += red[(w * 64 + (tid & 63)) * VEC + e];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = s[e];
  }
}

// VEC consecutive per-channel coefficients as 16-byte loads (arrays are 16-byte aligned, c0 is a multiple of VEC)
template <int VEC>
__device__ __forceinline__ void ldcoef(const float* __restrict__ p, int c0, float (&o)[VEC], float dflt) {
  if (!p) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) o[e] = dflt;
    return;
  }
#pragma unroll
  for (int q = 0; q < VEC / 4; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(p + c0 + 4 * q);
    o[4 * q] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
  }
}

__device__ __forceinline__ float act_fwd(float v, int act, float slope) { return act == 0 ? v : (v > 0.f ? v : v * slope); }
__device__ __forceinline__ float act_grad(float pre, int act, float slope) { return act == 0 ? 1.f : (pre > 0.f ? 1.f : slope); }
