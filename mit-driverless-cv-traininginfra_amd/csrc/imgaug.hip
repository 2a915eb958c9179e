// Real-image detector batches with the reference's training augmentation (CVC-YOLOv3/utils/datasets.py:226-242): torchvision 0.3's
// ColorJitter (brightness / contrast / saturation / hue in a shuffled order) and F.affine (BILINEAR, fill 127) between the patch crop
// and to_grayscale / hflip / to_tensor.  Both are thin glue over Pillow, and the bytes equal Pillow 12.2's:
//   blend      Image.blend under ImageEnhance: float32 d + alpha * (i - d), truncated; clipped to 0..255 first when alpha is outside [0, 1]
//   hue        convert('HSV') (float with a few double steps, Convert.c rgb2hsv), a wrapping uint8 shift of H, convert('RGB') (float)
//   affine     Geometry.c's generic transform: the inverse map and the bilinear blend of four clamped taps in double, truncated
// The matrix comes from the host (libm, float64); nothing here evaluates a transcendental.  Built with -ffp-contract=off: every product
// and sum rounds on its own, as the C that Pillow is built from does on x86-64.
// Launches per augmented batch: imgload_hpass (csrc/imgload.hip), patch_u8 (the uint8 RGBX patch), jitter_stats (only when some image's
// jitter is on: the integer luma sum that Contrast's grey needs), apply.  blockIdx.z is the image.
#include "imgload_desc.h"

#define MDCV_IMGAUG_DESC 24
#define IMGAUG_MAX_PIXELS (4096LL * 4096LL)      // H * W * 255 stays inside 32 bits: the luma sum is one unsigned int per image

namespace {

enum { A_MATRIX = 0, A_JITTER = 12, A_ORDER = 13, A_BRIGHT = 17, A_CONTRAST = 18, A_SAT = 19, A_HUE = 20, A_AFFINE = 21, A_RES0 = 22, A_RES1 = 23 };
enum { OP_BRIGHT, OP_CONTRAST, OP_SAT, OP_HUE };

__host__ __device__ inline float bits_f32(int v) {
  union { int i; float f; } u;
  u.i = v;
  return u.f;
}

__host__ __device__ inline double bits_f64(const int* p) {
  union { unsigned long long i; double f; } u;
  u.i = (unsigned long long)(unsigned)p[0] | ((unsigned long long)(unsigned)p[1] << 32);
  return u.f;
}

// Nothing in an augmentation descriptor indexes memory (every tap is clamped to the patch), so this only keeps the arithmetic inside what
// the semantics define: flags are flags, the order is a permutation, factors and matrix entries are finite.
__host__ __device__ inline bool aug_ok(const int* a) {
  if ((a[A_JITTER] != 0 && a[A_JITTER] != 1) || (a[A_AFFINE] != 0 && a[A_AFFINE] != 1)) return false;
  int seen = 0;
  for (int k = 0; k < 4; ++k) {
    if (a[A_ORDER + k] < 0 || a[A_ORDER + k] > 3) return false;
    seen |= 1 << a[A_ORDER + k];
  }
  if (seen != 15) return false;
  for (int k = A_BRIGHT; k <= A_SAT; ++k) {
    const float f = bits_f32(a[k]);
    if (!(f >= 0.0f && f <= 16.0f)) return false;
  }
  if (a[A_HUE] < 0 || a[A_HUE] > 255) return false;
  for (int k = 0; k < 6; ++k) {
    const double m = bits_f64(a + A_MATRIX + 2 * k);
    if (!(m >= -1e9 && m <= 1e9)) return false;
  }
  return a[A_RES0] == 0 && a[A_RES1] == 0;
}

struct Rgb { int r, g, b; };

__device__ __forceinline__ int luma(const Rgb& p) { return (p.r * 19595 + p.g * 38470 + p.b * 7471 + 0x8000) >> 16; }     // Pillow convert('L')

__device__ __forceinline__ int blend1(int d, int i, float alpha, bool inside) {     // ImagingBlend, one byte
  const float t = (float)d + alpha * (float)(i - d);
  if (inside) return (int)t;                                  // t is in [0, 255]: (UINT8)t
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ Rgb blend(int d, const Rgb& p, float alpha) {
  const bool inside = alpha >= 0.0f && alpha <= 1.0f;
  return Rgb{blend1(d, p.r, alpha, inside), blend1(d, p.g, alpha, inside), blend1(d, p.b, alpha, inside)};
}

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// adjust_hue: Convert.c rgb2hsv, H += shift (uint8), hsv2rgb
__device__ inline Rgb hue_rotate(const Rgb& p, int shift) {
  const int maxc = max(p.r, max(p.g, p.b)), minc = min(p.r, min(p.g, p.b));
  int uh = 0, us = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - p.r) / cr, gc = (float)(maxc - p.g) / cr, bc = (float)(maxc - p.b) / cr;
    float h;
    if (p.r == maxc) h = bc - gc;
    else if (p.g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double t = (double)h / 6.0 + 1.0;                 // in [5/6, 11/6]: fmod(t, 1.0) is t - floor(t), exact
    h = (float)(t - floor(t));
    uh = clip255((int)((double)h * 255.0));
    us = clip255((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 255;
  if (us == 0) return Rgb{maxc, maxc, maxc};
  const float v = (float)maxc;
  const float hh = (float)uh * 6.0f / 255.0f;
  const float fi = floorf(hh);
  const float f = hh - fi;
  const float fs = (float)us / 255.0f;
  const int pp = clip255((int)roundf(v * (1.0f - fs)));
  const int q = clip255((int)roundf(v * (1.0f - fs * f)));
  const int t = clip255((int)roundf(v * (1.0f - fs * (1.0f - f))));
  switch ((int)fi % 6) {
    case 0: return Rgb{maxc, t, pp};
    case 1: return Rgb{q, maxc, pp};
    case 2: return Rgb{pp, maxc, t};
    case 3: return Rgb{pp, q, maxc};
    case 4: return Rgb{t, pp, maxc};
    default: return Rgb{maxc, pp, q};
  }
}

// ColorJitter's chain on one pixel.  `mean` < 0: stop in front of the contrast op (what the statistics pass needs).
__device__ inline Rgb jitter_chain(Rgb p, const int* a, int mean) {
  for (int k = 0; k < 4; ++k) {
    const int op = a[A_ORDER + k];
    if (op == OP_BRIGHT) p = blend(0, p, bits_f32(a[A_BRIGHT]));
    else if (op == OP_SAT) p = blend(luma(p), p, bits_f32(a[A_SAT]));
    else if (op == OP_HUE) p = hue_rotate(p, a[A_HUE]);
    else {
      if (mean < 0) return p;
      p = blend(mean, p, bits_f32(a[A_CONTRAST]));
    }
  }
  return p;
}

__device__ __forceinline__ Rgb unpack(unsigned v) { return Rgb{(int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u)}; }

// The uint8 patch: imgload_vpass_kernel's pixel without hflip / convert('L') / /255, as [B][H][W] RGBX.  Also clears the luma sums.
__global__ __launch_bounds__(256) void imgaug_patch_u8_kernel(const int* __restrict__ desc, const long long* __restrict__ fref,
                                                              const int* __restrict__ coefs, long long n_coefs, long long src_bytes,
                                                              long long pool_bytes, int max_scr_w, int max_scr_h, int H, int W,
                                                              const unsigned char* __restrict__ ws, unsigned* __restrict__ patch,
                                                              unsigned* __restrict__ sums) {
  __shared__ int sdesc[MDCV_IMGLOAD_DESC];
  __shared__ long long sfref[MDCV_IMGLOAD_FREF];
  const int b = blockIdx.z, tid = threadIdx.x;
  const long long* f = imgload_stage_desc(sdesc, sfref, desc, fref, b, tid);
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) sums[b] = 0u;
  __syncthreads();
  const bool ok = image_ok(sdesc, f, n_coefs, src_bytes, pool_bytes, max_scr_w, max_scr_h);
  const int x = blockIdx.x * 64 + (tid & 63);
  if (x >= W) return;
  unsigned* pb = patch + (size_t)b * H * W;
  const unsigned char* sb = ws + (size_t)b * max_scr_w * max_scr_h * 3;
  for (int y = blockIdx.y * 4 + (tid >> 6); y < H; y += gridDim.y * 4) {
    int v0 = 0, v1 = 0, v2 = 0;
    if (ok) imgload_patch_pixel(sdesc, coefs, sb, max_scr_w, x, y, v0, v1, v2);
    pb[(size_t)y * W + x] = (unsigned)v0 | ((unsigned)v1 << 8) | ((unsigned)v2 << 16) | 0xff000000u;
  }
}

// Contrast's grey is int(mean(L) + 0.5) of the patch as it is when the contrast op runs: apply the (pointwise) ops in front of it, form L
// and sum it.  Integer adds: the sum does not depend on the order, so it is the same bits every run.  Wave reduction, then one atomic per
// workgroup.
__global__ __launch_bounds__(256) void imgaug_jitter_stats_kernel(const int* __restrict__ aug, int H, int W, const unsigned* __restrict__ patch,
                                                                  unsigned* __restrict__ sums) {
  __shared__ int sa[MDCV_IMGAUG_DESC];
  __shared__ unsigned part[4];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (tid < MDCV_IMGAUG_DESC) sa[tid] = aug[(size_t)b * MDCV_IMGAUG_DESC + tid];
  __syncthreads();
  if (!aug_ok(sa) || !sa[A_JITTER]) return;                   // uniform over the workgroup
  const int x = blockIdx.x * 64 + (tid & 63);
  const unsigned* pb = patch + (size_t)b * H * W;
  unsigned acc = 0;
  if (x < W)
    for (int y = blockIdx.y * 4 + (tid >> 6); y < H; y += gridDim.y * 4) acc += (unsigned)luma(jitter_chain(unpack(pb[(size_t)y * W + x]), sa, -1));
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) atomicAdd(sums + b, part[0] + part[1] + part[2] + part[3]);
}

// Per output pixel: the inverse affine map in double, four clamped taps each through the jitter chain, the bilinear blend, then exactly
// what imgload_vpass_kernel does behind its pixel: convert('L'), mirrored store, /255 into [B,C,H,W] fp32.  An image with neither jitter
// nor affine is copied (the same bytes as the two-launch path); an image whose descriptor fails the check is written as zeros.
__global__ __launch_bounds__(256) void imgaug_apply_kernel(const int* __restrict__ desc, const long long* __restrict__ fref,
                                                           const int* __restrict__ aug, long long n_coefs, long long src_bytes,
                                                           long long pool_bytes, int max_scr_w, int max_scr_h, int C, int H, int W,
                                                           const unsigned* __restrict__ patch, const unsigned* __restrict__ sums,
                                                           float* __restrict__ out) {
  __shared__ int sa[MDCV_IMGAUG_DESC];
  __shared__ int sdesc[MDCV_IMGLOAD_DESC];
  __shared__ long long sfref[MDCV_IMGLOAD_FREF];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (tid >= 64 && tid < 64 + MDCV_IMGAUG_DESC) sa[tid - 64] = aug[(size_t)b * MDCV_IMGAUG_DESC + tid - 64];
  const long long* f = imgload_stage_desc(sdesc, sfref, desc, fref, b, tid);
  __syncthreads();
  const bool ok = aug_ok(sa) && image_ok(sdesc, f, n_coefs, src_bytes, pool_bytes, max_scr_w, max_scr_h);
  const int ox = blockIdx.x * 64 + (tid & 63);
  if (ox >= W) return;
  const int x = ok && sdesc[D_FLIP] ? W - 1 - ox : ox;
  const size_t plane = (size_t)H * W;
  float* ob = out + (size_t)b * C * plane;
  const unsigned* pb = patch + (size_t)b * plane;
  const bool jit = ok && sa[A_JITTER], aff = ok && sa[A_AFFINE];
  const int mean = (int)((double)sums[b] / (double)((long long)H * W) + 0.5);
  double m[6];
  for (int k = 0; k < 6; ++k) m[k] = bits_f64(sa + A_MATRIX + 2 * k);
  for (int oy = blockIdx.y * 4 + (tid >> 6); oy < H; oy += gridDim.y * 4) {
    Rgb v{0, 0, 0};
    if (ok && !aff) {
      v = unpack(pb[(size_t)oy * W + x]);
      if (jit) v = jitter_chain(v, sa, mean);
    } else if (ok) {
      const double xo = (double)x + 0.5, yo = (double)oy + 0.5;
      double xin = m[0] * xo + m[1] * yo + m[2];
      double yin = m[3] * xo + m[4] * yo + m[5];
      if (xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H) {
        xin -= 0.5;
        yin -= 0.5;
        const double fx = floor(xin), fy = floor(yin);
        const double dx = xin - fx, dy = yin - fy;
        const int xi = (int)fx, yi = (int)fy;                 // in [-1, W - 1] x [-1, H - 1]
        const int x0 = max(xi, 0), x1 = min(xi + 1, W - 1), y0 = max(yi, 0), y1 = min(yi + 1, H - 1);
        Rgb p00 = unpack(pb[(size_t)y0 * W + x0]), p01 = unpack(pb[(size_t)y0 * W + x1]);
        Rgb p10 = unpack(pb[(size_t)y1 * W + x0]), p11 = unpack(pb[(size_t)y1 * W + x1]);
        if (jit) {
          p00 = jitter_chain(p00, sa, mean); p01 = jitter_chain(p01, sa, mean);
          p10 = jitter_chain(p10, sa, mean); p11 = jitter_chain(p11, sa, mean);
        }
        auto lerp = [dx, dy](int a00, int a01, int a10, int a11) {
          const double v1 = (double)a00 + (double)(a01 - a00) * dx;
          const double v2 = (double)a10 + (double)(a11 - a10) * dx;
          return (int)(v1 + (v2 - v1) * dy);                  // in [0, 255]: (UINT8)v
        };
        v = Rgb{lerp(p00.r, p01.r, p10.r, p11.r), lerp(p00.g, p01.g, p10.g, p11.g), lerp(p00.b, p01.b, p10.b, p11.b)};
      } else {
        v = Rgb{127, 127, 127};
      }
    }
    float* o = ob + (size_t)oy * W + ox;
    if (C == 1) {
      o[0] = (float)luma(v) / 255.0f;
    } else {
      o[0] = (float)v.r / 255.0f; o[plane] = (float)v.g / 255.0f; o[2 * plane] = (float)v.b / 255.0f;
    }
  }
}

inline long long patch_bytes(int B, int H, int W) { return ((long long)B * H * W * 4 + 255) / 256 * 256; }

// Both entry points: fref_host == fref == nullptr is the staged form.
int imgaug_batch_impl(const int* desc_host, const int* desc, const long long* fref_host, const long long* fref, const int* aug_host,
                      const int* aug, int B, const int* coefs, long long n_coefs, const unsigned char* src, long long src_bytes,
                      const unsigned char* pool, long long pool_bytes, int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace,
                      void* aug_workspace, float* out, void* stream) {
  if (!desc_host || !desc || !aug_host || !aug || !coefs || !out || !aug_workspace) return MDCV_EARG;
  if (B <= 0 || B > 65535 || n_coefs <= 0 || src_bytes < 0 || (src_bytes > 0 && !src)) return MDCV_EARG;
  if (pool_bytes < 0 || pool_bytes > IMGLOAD_MAX_POOL || (pool_bytes > 0 && !pool)) return MDCV_EARG;
  if (max_scr_w < 0 || max_scr_h < 0 || (!workspace && (long long)max_scr_w * max_scr_h > 0)) return MDCV_EARG;
  if ((C != 1 && C != 3) || H <= 0 || W <= 0 || (long long)H * W > IMGAUG_MAX_PIXELS) return MDCV_EARG;
  bool any_jitter = false;
  for (int b = 0; b < B; ++b) {
    if (!image_ok(desc_host + (size_t)b * MDCV_IMGLOAD_DESC, fref_host ? fref_host + (size_t)b * MDCV_IMGLOAD_FREF : nullptr, n_coefs,
                  src_bytes, pool_bytes, max_scr_w, max_scr_h))
      return MDCV_EARG;
    if (!aug_ok(aug_host + (size_t)b * MDCV_IMGAUG_DESC)) return MDCV_EARG;
    any_jitter = any_jitter || aug_host[(size_t)b * MDCV_IMGAUG_DESC + A_JITTER] != 0;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned* patch = (unsigned*)aug_workspace;
  unsigned* sums = (unsigned*)((char*)aug_workspace + patch_bytes(B, H, W));
  if ((long long)max_scr_w * max_scr_h > 0) {
    const int rc = imgload_launch_hpass(desc, fref, B, coefs, n_coefs, src, src_bytes, pool, pool_bytes, max_scr_w, max_scr_h, workspace, stream);
    if (rc != MDCV_OK) return rc;
  }
  const dim3 grid((unsigned)(W + 63) / 64, (unsigned)(H + 3) / 4 < 64u ? (unsigned)(H + 3) / 4 : 64u, (unsigned)B);
  MDCV_LAUNCH(imgaug_patch_u8_kernel, grid, dim3(256), 0, st, desc, fref, coefs, n_coefs, src_bytes, pool_bytes, max_scr_w, max_scr_h, H, W,
              (const unsigned char*)workspace, patch, sums);
  MDCV_CHECK_LAUNCH();
  if (any_jitter) {
    MDCV_LAUNCH(imgaug_jitter_stats_kernel, grid, dim3(256), 0, st, aug, H, W, (const unsigned*)patch, sums);
    MDCV_CHECK_LAUNCH();
  }
  MDCV_LAUNCH(imgaug_apply_kernel, grid, dim3(256), 0, st, desc, fref, aug, n_coefs, src_bytes, pool_bytes, max_scr_w, max_scr_h, C, H, W,
              (const unsigned*)patch, (const unsigned*)sums, out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // namespace

extern "C" {

long long mdcv_imgaug_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > IMGAUG_MAX_PIXELS) return MDCV_EARG;
  return patch_bytes(B, H, W) + (long long)B * 4;
}

int mdcv_imgload_aug_batch(const int* desc_host, const int* desc, const int* aug_host, const int* aug, int B, const int* coefs, long long n_coefs,
                           const unsigned char* src, long long src_bytes, int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace,
                           void* aug_workspace, float* out, void* stream) {
  return imgaug_batch_impl(desc_host, desc, nullptr, nullptr, aug_host, aug, B, coefs, n_coefs, src, src_bytes, nullptr, 0, max_scr_w,
                           max_scr_h, C, H, W, workspace, aug_workspace, out, stream);
}

int mdcv_imgload_aug_frames_batch(const int* desc_host, const int* desc, const long long* fref_host, const long long* fref, const int* aug_host,
                                  const int* aug, int B, const int* coefs, long long n_coefs, const unsigned char* src, long long src_bytes,
                                  const unsigned char* pool, long long pool_bytes, int max_scr_w, int max_scr_h, int C, int H, int W,
                                  void* workspace, void* aug_workspace, float* out, void* stream) {
  if (!fref_host || !fref) return MDCV_EARG;
  return imgaug_batch_impl(desc_host, desc, fref_host, fref, aug_host, aug, B, coefs, n_coefs, src, src_bytes, pool, pool_bytes, max_scr_w,
                           max_scr_h, C, H, W, workspace, aug_workspace, out, stream);
}

}  // extern "C"
