// The per-image descriptor of csrc/imgfx.hip (blur / noise / contrast / sharpen on a finished [B,3,H,W] batch) and its check, which runs
// on the host (MDCV_EARG before any launch) and again in the kernel on the device copy (a failing image is written as zeros).
#pragma once
#include <math.h>

#define MDCV_IMGFX_DESC 24
#define IMGFX_MAX_R 7                            // blur radius: sigma < 5 under imgaug 0.3.0's kernel-size rule
#define IMGFX_MAX_PIXELS (4096LL * 4096LL)       // 3 * H * W stays inside 32 bits: the noise counter is one unsigned int
#define IMGFX_MIN_SIDE 16                        // a halo of IMGFX_MAX_R + 1 reflects once

namespace {

enum { X_BLUR = 0, X_R = 1, X_Q = 2, X_NOISE = 10, X_PER_CHANNEL = 11, X_SEED = 12, X_SCALE = 13, X_CONTRAST = 15, X_LUT = 16, X_SHARPEN = 17,
       X_KC = 18, X_KN = 19, X_RES0 = 20 };

__host__ __device__ inline float imgfx_bits_f32(int v) {
  union { int i; float f; } u;
  u.i = v;
  return u.f;
}

__host__ __device__ inline double imgfx_bits_f64(const int* p) {
  union { unsigned long long i; double f; } u;
  u.i = (unsigned long long)(unsigned)p[0] | ((unsigned long long)(unsigned)p[1] << 32);
  return u.f;
}

// Only the table index locates memory; the rest keeps the arithmetic inside what the semantics define (and inside int): flags are flags,
// the half table (centre first) is a non-negative symmetric 8-bit kernel of sum 256 with nothing beyond its radius, the noise scale and
// the two sharpen coefficients are finite and no larger than imgaug's own parameter ranges allow (alpha in [0, 1]: centre 1 + 8 alpha,
// neighbour -alpha; the loader draws alpha <= 0.5 and scale <= 7.65).  Every field is checked whether or not its flag is set: the loader
// writes the identity (r 1, table {256}, scale 0, coefficients 1 and 0) for an op that is off.
__host__ __device__ inline bool fx_ok(const int* d, int n_luts) {
  const int flags[5] = {d[X_BLUR], d[X_NOISE], d[X_PER_CHANNEL], d[X_CONTRAST], d[X_SHARPEN]};
  for (int k = 0; k < 5; ++k)
    if (flags[k] != 0 && flags[k] != 1) return false;
  const int r = d[X_R];
  if (r < 1 || r > IMGFX_MAX_R) return false;
  int sum = 0;
  for (int k = 0; k <= IMGFX_MAX_R; ++k) {
    const int q = d[X_Q + k];
    if (q < 0 || q > 256 || (k > r && q != 0)) return false;
    sum += k == 0 ? q : 2 * q;
  }
  if (sum != 256) return false;
  const double s = imgfx_bits_f64(d + X_SCALE);
  if (!(s >= 0.0 && s <= 255.0)) return false;
  if (d[X_CONTRAST] && (d[X_LUT] < 0 || d[X_LUT] >= n_luts)) return false;
  const float kc = imgfx_bits_f32(d[X_KC]), kn = imgfx_bits_f32(d[X_KN]);
  if (!(kc >= 0.0f && kc <= 16.0f) || !(kn >= -2.0f && kn <= 2.0f)) return false;
  for (int k = X_RES0; k < MDCV_IMGFX_DESC; ++k)
    if (d[k] != 0) return false;
  return true;
}

}  // namespace
