// NCHW fp32 <-> padded NHWC (bf16 / fp32) layout conversion for gfx950.
#include "strip.h"

namespace {

template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int B, int C, int H, int W, int ldc, int Cpad) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = Cpad / VEC;
  const long long total = (long long)B * H * W * CV;
  const int HW = H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cv = (int)(i % CV);
    const long long pix = i / CV;
    const int b = (int)(pix / HW), hw = (int)(pix - (long long)b * HW);
    float v[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int c = cv * VEC + e;
      v[e] = c < C ? src[((size_t)b * C + c) * HW + hw] : 0.f;
    }
    *reinterpret_cast<uint4*>(dst + (size_t)pix * ldc + cv * VEC) = ET<T>::pack(v);
  }
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ src, float* __restrict__ dst, int B, int C, int H, int W, int ldc) {
  const long long total = (long long)B * C * H * W;
  const int HW = H * W;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int hw = (int)(i % HW);
    const long long bc = i / HW;
    const int c = (int)(bc % C), b = (int)(bc / C);
    dst[i] = ET<T>::ld(src + ((size_t)b * HW + hw) * ldc + c);
  }
}

}  // namespace

extern "C" {

int mdcv_nchw_to_nhwc(int dtype, const float* src, void* dst, int B, int C, int H, int W, int ldc, int Cpad, void* stream) {
  if (!src || !dst || (Cpad & 7) || (ldc & 7) || Cpad < C) return MDCV_EARG;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(nchw_to_nhwc_kernel<T>, dim3(ew_grid((long long)B * H * W * Cpad / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, src, (T*)dst,
                B, C, H, W, ldc, Cpad);
    return MDCV_OK;
  });
}

int mdcv_nhwc_to_nchw(int dtype, const void* src, int ldc, float* dst, int B, int C, int H, int W, void* stream) {
  if (!src || !dst) return MDCV_EARG;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(nhwc_to_nchw_kernel<T>, dim3(ew_grid((long long)B * C * H * W)), dim3(256), 0, (hipStream_t)stream, (const T*)src, dst,
                B, C, H, W, ldc);
    return MDCV_OK;
  });
}

}  // extern "C"
