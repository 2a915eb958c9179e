// 2x2 and generic max-pool, x2 and generic nearest upsample, forward and backward, NHWC for gfx950.  One thread per 16-byte channel vector.
#include "strip.h"

namespace {

// ---------------------------------------------------------------- nearest x2 upsample
template <typename T>
__global__ void upsample2x_fwd_kernel(const T* __restrict__ in, int ldi, T* __restrict__ out, int ldo, int B, int H, int W, int C) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const long long total = (long long)B * H * W * 4 * CV;       // one thread per OUTPUT vector
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, ow, oh, b; long long op;
    decode_pixel(i, CV, 2 * W, 2 * H, cv, op, ow, oh, b);
    const long long ip = ((long long)b * H + (oh >> 1)) * W + (ow >> 1);
    *reinterpret_cast<uint4*>(out + op * ldo + cv * VEC) = *reinterpret_cast<const uint4*>(in + ip * ldi + cv * VEC);
  }
}
template <typename T>
__global__ void upsample2x_bwd_kernel(const T* __restrict__ dout, int ldo, T* __restrict__ din, int ldi, int B, int H, int W, int C) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const long long total = (long long)B * H * W * CV;           // one thread per INPUT vector: sum of its 2x2 outputs
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, w, h, b; long long ip;
    decode_pixel(i, CV, W, H, cv, ip, w, h, b);
    float s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const long long op = ((long long)b * 2 * H + 2 * h + dy) * 2 * W + 2 * w + dx;
        float v[VEC];
        ET<T>::unpack(*reinterpret_cast<const uint4*>(dout + op * ldo + cv * VEC), v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] += v[e];
      }
    *reinterpret_cast<uint4*>(din + ip * ldi + cv * VEC) = ET<T>::pack(s);
  }
}

// ---------------------------------------------------------------- 2x2 max-pool (yolo_baseline_tiny.cfg): stride 2, or stride 1 on a
// bottom/right zero-padded input (nn.ZeroPad2d((0,1,0,1)) + nn.MaxPool2d(2,1), reference models.py:74-84).  idx = winning window
// position (kh*2+kw; first maximum wins like torch; 4 = the zero padding won) so that backward is a pure gather.  The update is torch's
// `v > best || isnan(v)`: a NaN in a window reaches the output, and idx points at the LAST NaN in scan order (a real value never replaces a
// NaN, a later NaN does).  The zero padding is never NaN.  A window of only -inf keeps idx = 0, whatever sits there.
template <typename T>
__global__ void maxpool2x2_fwd_kernel(const T* __restrict__ in, int ldi, T* __restrict__ out, int ldo, unsigned char* __restrict__ idx,
                                      int B, int H, int W, int C, int stride) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const int Ho = stride == 2 ? H / 2 : H, Wo = stride == 2 ? W / 2 : W;
  const long long total = (long long)B * Ho * Wo * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, ow, oh, b; long long op;
    decode_pixel(i, CV, Wo, Ho, cv, op, ow, oh, b);
    float best[VEC]; unsigned char bi[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { best[e] = -INFINITY; bi[e] = 0; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int h = oh * stride + (k >> 1), w = ow * stride + (k & 1);
      float v[VEC];
      const bool inside = h < H && w < W;
      if (inside) ET<T>::unpack(*reinterpret_cast<const uint4*>(in + (((long long)b * H + h) * W + w) * ldi + cv * VEC), v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float x = inside ? v[e] : 0.f;                    // zero padding takes part in the max
        if (x > best[e] || x != x) { best[e] = x; bi[e] = inside ? (unsigned char)k : (unsigned char)4; }
      }
    }
    *reinterpret_cast<uint4*>(out + op * ldo + cv * VEC) = ET<T>::pack(best);
#pragma unroll
    for (int e = 0; e < VEC; ++e) idx[op * C + cv * VEC + e] = bi[e];
  }
}
template <typename T>
__global__ void maxpool2x2_bwd_kernel(const T* __restrict__ dout, int ldo, const unsigned char* __restrict__ idx, T* __restrict__ din, int ldi,
                                      int B, int H, int W, int C, int stride) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const int Ho = stride == 2 ? H / 2 : H, Wo = stride == 2 ? W / 2 : W;
  const long long total = (long long)B * H * W * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, w, h, b; long long ip;
    decode_pixel(i, CV, W, H, cv, ip, w, h, b);
    float g[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) g[e] = 0.f;
    const int nwin = stride == 2 ? 1 : 4;
    for (int q = 0; q < nwin; ++q) {
      int oh, ow, pos;
      if (stride == 2) { oh = h >> 1; ow = w >> 1; pos = (h & 1) * 2 + (w & 1); }
      else { oh = h - (q >> 1); ow = w - (q & 1); pos = (q >> 1) * 2 + (q & 1); }
      if (oh < 0 || ow < 0 || oh >= Ho || ow >= Wo) continue;
      const long long op = ((long long)b * Ho + oh) * Wo + ow;
      float d[VEC];
      ET<T>::unpack(*reinterpret_cast<const uint4*>(dout + op * ldo + cv * VEC), d);
#pragma unroll
      for (int e = 0; e < VEC; ++e) if (idx[op * C + cv * VEC + e] == pos) g[e] += d[e];
    }
    *reinterpret_cast<uint4*>(din + ip * ldi + cv * VEC) = ET<T>::pack(g);
  }
}

// ---------------------------------------------------------------- generic max-pool and nearest upsample (reference models.py:74-88 builds
// nn.MaxPool2d(size, stride, (size - 1) // 2) and nn.Upsample(scale_factor = stride) for ANY size / stride; the bundled cfgs only use the
// 2x2 pools and the x2 upsample above).  Padding never wins (-inf); the first maximum in (kh, kw) scan order wins like torch, and a NaN
// beats everything but a later NaN (same update rule as above); idx = kh*k + kw (k <= 15), so backward is a gather over the windows that
// contain the input pixel: no atomics, deterministic.  A window of only -inf keeps idx = 0, which may be a padding position: its gradient
// goes nowhere.
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ in, int ldi, T* __restrict__ out, int ldo, unsigned char* __restrict__ idx,
                                   int B, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const long long total = (long long)B * Ho * Wo * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, ow, oh, b; long long op;
    decode_pixel(i, CV, Wo, Ho, cv, op, ow, oh, b);
    float best[VEC]; unsigned char bi[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    for (int kh = 0; kh < k; ++kh) {
      const int h = oh * stride - pad + kh;
      if (h < 0 || h >= H) continue;
      for (int kw = 0; kw < k; ++kw) {
        const int w = ow * stride - pad + kw;
        if (w < 0 || w >= W) continue;
        float v[VEC];
        ET<T>::unpack(*reinterpret_cast<const uint4*>(in + (((long long)b * H + h) * W + w) * ldi + cv * VEC), v);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = (unsigned char)(kh * k + kw); }
      }
    }
    *reinterpret_cast<uint4*>(out + op * ldo + cv * VEC) = ET<T>::pack(best);
#pragma unroll
    for (int e = 0; e < VEC; ++e) idx[op * C + cv * VEC + e] = bi[e];
  }
}
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ dout, int ldo, const unsigned char* __restrict__ idx, T* __restrict__ din, int ldi,
                                   int B, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const long long total = (long long)B * H * W * CV;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, w, h, b; long long ip;
    decode_pixel(i, CV, W, H, cv, ip, w, h, b);
    float g[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) g[e] = 0.f;
    // windows that contain (h, w): oh*stride - pad <= h <= oh*stride - pad + k - 1
    int oh0 = h + pad - k + 1; oh0 = oh0 > 0 ? (oh0 + stride - 1) / stride : 0;
    int ow0 = w + pad - k + 1; ow0 = ow0 > 0 ? (ow0 + stride - 1) / stride : 0;
    const int oh1 = min(Ho - 1, (h + pad) / stride), ow1 = min(Wo - 1, (w + pad) / stride);
    for (int oh = oh0; oh <= oh1; ++oh)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int pos = (h + pad - oh * stride) * k + (w + pad - ow * stride);
        const long long op = ((long long)b * Ho + oh) * Wo + ow;
        float d[VEC];
        ET<T>::unpack(*reinterpret_cast<const uint4*>(dout + op * ldo + cv * VEC), d);
#pragma unroll
        for (int e = 0; e < VEC; ++e) if (idx[op * C + cv * VEC + e] == pos) g[e] += d[e];
      }
    *reinterpret_cast<uint4*>(din + ip * ldi + cv * VEC) = ET<T>::pack(g);
  }
}
template <typename T>
__global__ void upsample_fwd_kernel(const T* __restrict__ in, int ldi, T* __restrict__ out, int ldo, int B, int H, int W, int C, int sc) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const int Ws = W * sc, Hs = H * sc;
  const long long total = (long long)B * Hs * Ws * CV;         // one thread per OUTPUT vector
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, ow, oh, b; long long op;
    decode_pixel(i, CV, Ws, Hs, cv, op, ow, oh, b);
    const long long ip = ((long long)b * H + oh / sc) * W + ow / sc;
    *reinterpret_cast<uint4*>(out + op * ldo + cv * VEC) = *reinterpret_cast<const uint4*>(in + ip * ldi + cv * VEC);
  }
}
template <typename T>
__global__ void upsample_bwd_kernel(const T* __restrict__ dout, int ldo, T* __restrict__ din, int ldi, int B, int H, int W, int C, int sc) {
  constexpr int VEC = ET<T>::VEC;
  const int CV = C / VEC;
  const long long total = (long long)B * H * W * CV;           // one thread per INPUT vector: sum of its sc x sc outputs (fixed order)
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    int cv, w, h, b; long long ip;
    decode_pixel(i, CV, W, H, cv, ip, w, h, b);
    float s[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[e] = 0.f;
    for (int dy = 0; dy < sc; ++dy)
      for (int dx = 0; dx < sc; ++dx) {
        const long long op = ((long long)b * sc * H + sc * h + dy) * sc * W + sc * w + dx;
        float v[VEC];
        ET<T>::unpack(*reinterpret_cast<const uint4*>(dout + op * ldo + cv * VEC), v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] += v[e];
      }
    *reinterpret_cast<uint4*>(din + ip * ldi + cv * VEC) = ET<T>::pack(s);
  }
}

}  // namespace

extern "C" {

int mdcv_upsample2x_fwd(int dtype, const void* in, int ldi, void* out, int ldo, int B, int H, int W, int C, void* stream) {
  if (!in || !out || (C & 7)) return MDCV_EARG;
  const long long n = (long long)B * H * W * 4 * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(upsample2x_fwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)in, ldi, (T*)out, ldo, B, H, W, C);
    return MDCV_OK;
  });
}

int mdcv_upsample2x_bwd(int dtype, const void* dout, int ldo, void* din, int ldi, int B, int H, int W, int C, void* stream) {
  if (!dout || !din || (C & 7)) return MDCV_EARG;
  const long long n = (long long)B * H * W * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(upsample2x_bwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)dout, ldo, (T*)din, ldi, B, H, W, C);
    return MDCV_OK;
  });
}

int mdcv_maxpool2x2_fwd(int dtype, const void* in, int ldi, void* out, int ldo, unsigned char* idx, int B, int H, int W, int C, int stride,
                        void* stream) {
  if (!in || !out || !idx || (C & 7) || (stride != 1 && stride != 2)) return MDCV_EARG;
  const long long n = (long long)B * (stride == 2 ? H / 2 : H) * (stride == 2 ? W / 2 : W) * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(maxpool2x2_fwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)in, ldi, (T*)out, ldo, idx,
                B, H, W, C, stride);
    return MDCV_OK;
  });
}

int mdcv_maxpool2x2_bwd(int dtype, const void* dout, int ldo, const unsigned char* idx, void* din, int ldi, int B, int H, int W, int C, int stride,
                        void* stream) {
  if (!dout || !din || !idx || (C & 7) || (stride != 1 && stride != 2)) return MDCV_EARG;
  const long long n = (long long)B * H * W * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(maxpool2x2_bwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)dout, ldo, idx, (T*)din, ldi,
                B, H, W, C, stride);
    return MDCV_OK;
  });
}

// generic forms (any window <= 15 / stride / scale); Ho = (H + 2*pad - k) / stride + 1
int mdcv_maxpool_fwd(int dtype, const void* in, int ldi, void* out, int ldo, unsigned char* idx, int B, int H, int W, int C, int k, int stride,
                     int pad, void* stream) {
  if (!in || !out || !idx || (C & 7) || k < 1 || k > 15 || stride < 1 || pad < 0 || 2 * pad >= k + (k == 1) || H + 2 * pad < k || W + 2 * pad < k) return MDCV_EARG;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long long n = (long long)B * Ho * Wo * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(maxpool_fwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)in, ldi, (T*)out, ldo, idx,
                B, H, W, C, k, stride, pad, Ho, Wo);
    return MDCV_OK;
  });
}

int mdcv_maxpool_bwd(int dtype, const void* dout, int ldo, const unsigned char* idx, void* din, int ldi, int B, int H, int W, int C, int k, int stride,
                     int pad, void* stream) {
  if (!dout || !din || !idx || (C & 7) || k < 1 || k > 15 || stride < 1 || pad < 0 || 2 * pad >= k + (k == 1) || H + 2 * pad < k || W + 2 * pad < k) return MDCV_EARG;
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const long long n = (long long)B * H * W * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(maxpool_bwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)dout, ldo, idx, (T*)din, ldi,
                B, H, W, C, k, stride, pad, Ho, Wo);
    return MDCV_OK;
  });
}

int mdcv_upsample_fwd(int dtype, const void* in, int ldi, void* out, int ldo, int B, int H, int W, int C, int scale, void* stream) {
  if (!in || !out || (C & 7) || scale < 1 || scale > 64) return MDCV_EARG;
  const long long n = (long long)B * H * W * scale * scale * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(upsample_fwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)in, ldi, (T*)out, ldo, B, H, W, C, scale);
    return MDCV_OK;
  });
}

int mdcv_upsample_bwd(int dtype, const void* dout, int ldo, void* din, int ldi, int B, int H, int W, int C, int scale, void* stream) {
  if (!dout || !din || (C & 7) || scale < 1 || scale > 64) return MDCV_EARG;
  const long long n = (long long)B * H * W * C;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    MDCV_LAUNCH(upsample_bwd_kernel<T>, dim3(ew_grid(n / ET<T>::VEC)), dim3(256), 0, (hipStream_t)stream, (const T*)dout, ldo, (T*)din, ldi, B, H, W, C, scale);
    return MDCV_OK;
  });
}

}  // extern "C"
