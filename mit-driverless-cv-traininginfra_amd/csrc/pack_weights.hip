// Weight packing for the conv family: OIHW fp32 master weights -> the GEMM operand layouts the forward and data-gradient kernels read
// (conv_gemm.h, conv_shift.hip, pw_block.hip), one layer per launch or every layer of a network in one launch.
#include "common.h"

namespace {

// OIHW fp32 master weights -> GEMM operand layouts (T):
//   wf[n][tap][ci_pad]  (forward "B" operand, n < Cout_pad)      wd[ci][tap][co_pad]  (dgrad "B" operand, ci < Cin_pad)
template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wd, int Cout, int Cin,
                                    int KK, int Cout_pad, int Cin_pad) {
  const int nf = Cout_pad * KK * Cin_pad;
  const int nd = wd ? Cin_pad * KK * Cout_pad : 0;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nf + nd; e += gridDim.x * blockDim.x) {
    if (e < nf) {
      const int n = e / (KK * Cin_pad), rem = e - n * (KK * Cin_pad);
      const int t = rem / Cin_pad, ci = rem - t * Cin_pad;
      const float v = (n < Cout && ci < Cin) ? w[((size_t)n * Cin + ci) * KK + t] : 0.f;
      ET<T>::st(wf + e, v);
    } else {
      const int f = e - nf;
      const int ci = f / (KK * Cout_pad), rem = f - ci * (KK * Cout_pad);
      const int t = rem / Cout_pad, co = rem - t * Cout_pad;
      const float v = (co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * KK + t] : 0.f;
      ET<T>::st(wd + f, v);
    }
  }
}

// all layers in one launch: blockIdx.y selects the layer descriptor, blockIdx.x grid-strides inside it
// blocks per layer of the batched pack (grid.x; blocks past a layer's tile count exit at once).  With 64, the eight 4.7 M-parameter layers
// (60 % of YOLOv3's parameters) ran on 64 blocks x 8 tiles each while every other block had long finished: 327 us for 0.5 GB.
constexpr unsigned kPackBlocks = 256;
struct PackDesc { const float* w; void* wf; void* wd; int Cout, Cin, KK, Cout_pad, Cin_pad; int pad_[3]; const float* bias; float* bias_pad; };   // 72 bytes
// Tile = 16 output channels x up to 64 input channels x all taps, read from OIHW as contiguous runs (one run per output
// channel), transposed through LDS and written as  wf[co][tap][ci .. ci+63]  (128-byte runs) and  wd[ci][tap][co .. co+15].
// (A plain gather kernel read 17x the parameter bytes: rocprofv3 FETCH_SIZE 4.2 GB for 248 MB of weights.)
// Full tiles of the layers that hold nearly all parameters (bf16, Cin and Cout multiples of 64 / 16, 3x3 or 1x1, 16-byte aligned OIHW rows):
// the tap count is a compile-time constant, so no index of the tile needs a runtime division (the generic loops below spend ~100 of them per
// thread and tile), the OIHW runs are read as float4 with a whole tile's loads in flight, and both packed forms leave as 16-byte stores.
template <int KK>
__device__ __forceinline__ void pack_tile_fast(const PackDesc& d, float* tile, int co0, int ci0) {
  constexpr int PER = 64 * KK, CS = PER + 1, Q = PER / 4, NLD = (16 * Q + 255) / 256;
  const float* __restrict__ w = d.w;
  bf16_t* __restrict__ wf = reinterpret_cast<bf16_t*>(d.wf);
  bf16_t* __restrict__ wd = reinterpret_cast<bf16_t*>(d.wd);
  float4 v4[NLD];
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < 16 * Q) {
      const int co = i / Q, q = i - co * Q;
      v4[k] = *reinterpret_cast<const float4*>(w + ((size_t)(co0 + co) * d.Cin + ci0) * KK + 4 * q);
    }
  }
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i < 16 * Q) {
      const int co = i / Q, q = i - co * Q;
      float* t = tile + co * CS + 4 * q;
      t[0] = v4[k].x; t[1] = v4[k].y; t[2] = v4[k].z; t[3] = v4[k].w;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 16 * KK * 8; i += 256) {        // wf[co][tap][ci .. ci + 7]
    const int cv = i & 7, r = i >> 3;
    const int co = r / KK, t = r - co * KK;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[co * CS + (cv * 8 + e) * KK + t];
    *reinterpret_cast<uint4*>(wf + ((size_t)(co0 + co) * KK + t) * d.Cin_pad + ci0 + cv * 8) = ET<bf16_t>::pack(v);
  }
  if (wd) {
    for (int i = threadIdx.x; i < 2 * PER; i += 256) {          // wd[ci][tap][co .. co + 7]
      const int cov = i & 1, r = i >> 1;
      const int c = r / KK, t = r - c * KK;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = tile[(cov * 8 + e) * CS + r];
      *reinterpret_cast<uint4*>(wd + ((size_t)(ci0 + c) * KK + t) * d.Cout_pad + co0 + cov * 8) = ET<bf16_t>::pack(v);
    }
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const PackDesc* __restrict__ table) {
  extern __shared__ float tile[];
  const PackDesc d = table[blockIdx.y];
  if (blockIdx.x == 0 && d.bias)                          // the layer's fp32 bias parameter -> its padded operand buffer
    for (int i = threadIdx.x; i < d.Cout; i += 256) d.bias_pad[i] = d.bias[i];
  if constexpr (sizeof(T) == 2) {
    if ((d.KK == 9 || d.KK == 1) && d.Cin % 64 == 0 && d.Cin_pad == d.Cin && d.Cout % 16 == 0 && d.Cout_pad == d.Cout &&
        (reinterpret_cast<uintptr_t>(d.w) & 15) == 0) {   // (uniform per layer)
      const int tiles_ci = d.Cin / 64, ntiles = tiles_ci * (d.Cout / 16);
      for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int co0 = (tl / tiles_ci) * 16, ci0 = (tl % tiles_ci) * 64;
        if (d.KK == 9) pack_tile_fast<9>(d, tile, co0, ci0); else pack_tile_fast<1>(d, tile, co0, ci0);
      }
      return;
    }
  }
  const float* __restrict__ w = d.w;
  T* __restrict__ wf = reinterpret_cast<T*>(d.wf);
  T* __restrict__ wd = reinterpret_cast<T*>(d.wd);
  const int KK = d.KK;
  const int CIT = d.Cin_pad < 64 ? d.Cin_pad : 64;
  const int tiles_ci = (d.Cin_pad + CIT - 1) / CIT, tiles_co = (d.Cout_pad + 15) / 16;
  const int cstride = CIT * KK + 1;                       // +1: conflict-free column reads in the wd pass
  const int per = CIT * KK;
  for (int tl = blockIdx.x; tl < tiles_ci * tiles_co; tl += gridDim.x) {
    const int co0 = (tl / tiles_ci) * 16, ci0 = (tl % tiles_ci) * CIT;
    for (int i = threadIdx.x; i < 16 * per; i += 256) {
      const int co = i / per, rem = i - co * per;
      const int c = rem / KK, t = rem - c * KK;
      const int gco = co0 + co, gci = ci0 + c;
      tile[co * cstride + rem] = (gco < d.Cout && gci < d.Cin) ? w[((size_t)gco * d.Cin + gci) * KK + t] : 0.f;
    }
    __syncthreads();
    constexpr int VEC = ET<T>::VEC;
    if (CIT % VEC == 0) {                                   // 16-byte stores: VEC consecutive ci (wf) / co (wd) per thread
      const int cvn = CIT / VEC;
      for (int i = threadIdx.x; i < 16 * KK * cvn; i += 256) {
        const int cv = i % cvn, r = i / cvn;
        const int t = r % KK, co = r / KK;
        const int gco = co0 + co, gci = ci0 + cv * VEC;
        if (gco < d.Cout_pad && gci < d.Cin_pad) {
          float v[VEC];
#pragma unroll
          for (int e = 0; e < VEC; ++e) v[e] = tile[co * cstride + (cv * VEC + e) * KK + t];
          *reinterpret_cast<uint4*>(wf + ((size_t)gco * KK + t) * d.Cin_pad + gci) = ET<T>::pack(v);
        }
      }
      if (wd) {
        constexpr int COV = 16 / VEC;
        for (int i = threadIdx.x; i < COV * per; i += 256) {
          const int cov = i % COV, r = i / COV;
          const int t = r % KK, c = r / KK;
          const int gco = co0 + cov * VEC, gci = ci0 + c;
          if (gco < d.Cout_pad && gci < d.Cin_pad) {
            float v[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = tile[(cov * VEC + e) * cstride + c * KK + t];
            *reinterpret_cast<uint4*>(wd + ((size_t)gci * KK + t) * d.Cout_pad + gco) = ET<T>::pack(v);
          }
        }
      }
    } else {
    for (int i = threadIdx.x; i < 16 * per; i += 256) {   // wf: c fastest
      const int c = i % CIT, r = i / CIT;
      const int t = r % KK, co = r / KK;
      const int gco = co0 + co, gci = ci0 + c;
      if (gco < d.Cout_pad && gci < d.Cin_pad) ET<T>::st(wf + ((size_t)gco * KK + t) * d.Cin_pad + gci, tile[co * cstride + c * KK + t]);
    }
    if (wd) {
      for (int i = threadIdx.x; i < 16 * per; i += 256) { // wd: co fastest
        const int co = i & 15, r = i >> 4;
        const int t = r % KK, c = r / KK;
        const int gco = co0 + co, gci = ci0 + c;
        if (gco < d.Cout_pad && gci < d.Cin_pad) ET<T>::st(wd + ((size_t)gci * KK + t) * d.Cout_pad + gco, tile[co * cstride + c * KK + t]);
      }
    }
    }
    __syncthreads();
  }
}
}  // namespace

extern "C" {

int mdcv_pack_weights(int dtype, const float* w_oihw, void* w_fwd, void* w_dgrad, int Cout, int Cin, int KH, int KW,
                      int Cout_pad, int Cin_pad, void* stream) {
  if (!w_oihw || !w_fwd) return MDCV_EARG;
  const int KK = KH * KW;
  const long long n = (long long)Cout_pad * KK * Cin_pad * (w_dgrad ? 2 : 1);
  const unsigned grid = (unsigned)min(cdiv(n, 256), 8192);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MDCV_BF16)
    MDCV_LAUNCH(pack_weights_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, w_oihw, (bf16_t*)w_fwd, (bf16_t*)w_dgrad, Cout, Cin, KK, Cout_pad, Cin_pad);
  else if (dtype == MDCV_F32)
    MDCV_LAUNCH(pack_weights_kernel<float>, dim3(grid), dim3(256), 0, st, w_oihw, (float*)w_fwd, (float*)w_dgrad, Cout, Cin, KK, Cout_pad, Cin_pad);
  else return MDCV_EARG;
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

// one launch for every conv of a network: `table` = nlayers device-resident 64-byte records
//   { const float* w_oihw; void* w_fwd; void* w_dgrad (or NULL); int Cout, Cin, KH*KW, Cout_pad, Cin_pad; int reserved[3]; }
int mdcv_pack_weights_batched(int dtype, const void* table, int nlayers, int max_taps, void* stream) {
  if (!table || nlayers < 1 || max_taps < 1) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const int lds = 16 * (64 * max_taps + 1) * 4;          // 16 x (64 ci x taps + 1) floats
  if (lds > 160 * 1024) return MDCV_EARG;
  static DynLds dyn_lds16, dyn_lds32;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds16, reinterpret_cast<const void*>(pack_weights_batched_kernel<bf16_t>), lds); e != hipSuccess) return (int)e;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds32, reinterpret_cast<const void*>(pack_weights_batched_kernel<float>), lds); e != hipSuccess) return (int)e;
  if (dtype == MDCV_BF16) MDCV_LAUNCH(pack_weights_batched_kernel<bf16_t>, dim3(kPackBlocks, (unsigned)nlayers), dim3(256), lds, st, (const PackDesc*)table);
  else if (dtype == MDCV_F32) MDCV_LAUNCH(pack_weights_batched_kernel<float>, dim3(kPackBlocks, (unsigned)nlayers), dim3(256), lds, st, (const PackDesc*)table);
  else return MDCV_EARG;
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
