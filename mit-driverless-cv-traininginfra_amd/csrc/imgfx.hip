// The reference's four imgaug options (CVC-YOLOv3/utils/datasets.py:253-295: GaussianBlur, AdditiveGaussianNoise, SigmoidContrast, Sharpen
// of imgaug 0.3.0 over OpenCV 4.1) on a finished detector batch: [B,3,H,W] fp32 holding u / 255 in, the same out, one launch, blockIdx.z
// the image.  The ops work on the bytes, in this order, each behind its own flag (DESIGN §16.3 defines every step):
//   blur      separable, BORDER_REFLECT_101, OpenCV's 8-bit fixed point: sum q * src (16 bits, unrounded), then (sum q * t + 32768) >> 16
//   noise     + clip(rint(scale * z), -255, 255), clipped to 0..255; z a 12-term Irwin-Hall normal from a counter-based integer hash of
//             (seed, sample counter): one draw per (y, x, c), or per (y, x) shared by the channels
//   contrast  a 256-entry table computed on the host
//   sharpen   rint((double)kc * centre + (double)kn * (sum of the 8 neighbours)), BORDER_REFLECT_101, clipped to 0..255
// Everything is integer or one correctly rounded float / double operation; nothing here evaluates a transcendental.  Built with
// -ffp-contract=off.  A workgroup owns a 64 x 16 tile: the source bytes of the tile and a halo of r + 1 go to LDS through reflected
// indices, the blur's two passes, the noise and the table run in LDS at in-image positions only, and the sharpen reflects its own taps
// into those (REFLECT_101 of the blurred, noised image is not the blur of the reflected source's noise).
#include "common.h"
#include "imgfx_desc.h"
#include "../../include/mdcv_hip.h"

#define FX_TW 64
#define FX_TH 16
#define FX_PW (FX_TW + 2)                        // the tile and the sharpen's ring of 1
#define FX_PH (FX_TH + 2)
#define FX_SW (FX_PW + 2 * IMGFX_MAX_R)          // ... and the blur's ring of r
#define FX_SH (FX_PH + 2 * IMGFX_MAX_R)

namespace {

// csrc/synth.hip's mixer, and its two-round keyed word with the word index j where synth.hip has its stream number
__device__ __forceinline__ unsigned fx_hash32(unsigned x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned fx_word(unsigned seed, unsigned n, unsigned j) {
  return fx_hash32(fx_hash32(seed * 0x9E3779B1u + j * 0x85EBCA77u + n * 0xC2B2AE3Du) + 0x27D4EB2Fu);
}

// The value AddElementwise adds for sample counter n: twelve 16-bit uniforms summed (mean 393210, variance 65536^2 (1 - 2^-32)), scaled in
// double (one product, an exact division by 2^16), rounded half to even, clipped to +-255.  |scale * S| <= 255 * 393210 < 2^27.
__device__ __forceinline__ int fx_noise(unsigned seed, unsigned n, double scale) {
  int S = 0;
  for (unsigned j = 0; j < 6; ++j) {
    const unsigned h = fx_word(seed, n, j);
    S += (int)(h & 0xffffu) + (int)(h >> 16);
  }
  const int v = (int)rint(scale * (double)(S - 393210) / 65536.0);
  return v < -255 ? -255 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int fx_clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// BORDER_REFLECT_101 of an index at most n - 1 outside [0, n); farther out (LDS cells no in-image pixel reads) it is clamped
__device__ __forceinline__ int fx_reflect(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// the byte an input float stands for; anything that is not u / 255 lands on some byte
__device__ __forceinline__ int fx_byte(float f) {
  f = f >= 0.0f ? (f <= 1.0f ? f : 1.0f) : 0.0f;
  return (int)rintf(f * 255.0f);
}

__global__ __launch_bounds__(256) void imgfx_kernel(const int* __restrict__ fx, const unsigned char* __restrict__ luts, int n_luts, int H, int W,
                                                    int tiles_x, const float* __restrict__ src, float* __restrict__ dst) {
  __shared__ int sd[MDCV_IMGFX_DESC];
  __shared__ unsigned char s_src[3][FX_SH][FX_SW];           // source bytes, origin (ty0 - 1 - r, tx0 - 1 - r)
  __shared__ unsigned short s_row[3][FX_SH][FX_PW];          // horizontal pass, origin (ty0 - 1 - r, tx0 - 1)
  __shared__ unsigned char s_pix[3][FX_PH][FX_PW];           // blur + noise + table, origin (ty0 - 1, tx0 - 1)
  __shared__ unsigned char s_lut[256];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (tid < MDCV_IMGFX_DESC) sd[tid] = fx[(size_t)b * MDCV_IMGFX_DESC + tid];
  __syncthreads();
  const bool ok = fx_ok(sd, n_luts);
  const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * FX_TW, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * FX_TH;
  const size_t plane = (size_t)H * W;
  const float* sb = src + (size_t)b * 3 * plane;
  float* db = dst + (size_t)b * 3 * plane;
  const bool blur = ok && sd[X_BLUR], noise = ok && sd[X_NOISE], contrast = ok && sd[X_CONTRAST], sharpen = ok && sd[X_SHARPEN];
  const int ox = tid & 63;

  if (!(blur || noise || contrast || sharpen)) {              // no flag: the floats themselves; a bad descriptor: zeros (uniform over the workgroup)
    const int x = tx0 + ox;
    if (x < W)
      for (int oy = tid >> 6; oy < FX_TH && ty0 + oy < H; oy += 4)
        for (int c = 0; c < 3; ++c) {
          const size_t at = c * plane + (size_t)(ty0 + oy) * W + x;
          db[at] = ok ? sb[at] : 0.0f;
        }
    return;
  }

  // an op that is off runs as its identity: radius 0 with the one tap 256 gives (256 * 256 * u + 32768) >> 16 == u
  const int r = blur ? sd[X_R] : 0;
  int q[IMGFX_MAX_R + 1];
  for (int k = 0; k <= IMGFX_MAX_R; ++k) q[k] = blur ? sd[X_Q + k] : (k == 0 ? 256 : 0);
  s_lut[tid] = contrast ? luts[(size_t)sd[X_LUT] * 256 + tid] : (unsigned char)tid;

  const int sw = FX_PW + 2 * r, sh = FX_PH + 2 * r;
  for (int i = tid; i < 3 * sh * sw; i += 256) {
    const int c = i / (sh * sw), rem = i - c * (sh * sw);
    const int yy = rem / sw, xx = rem - yy * sw;
    const int gy = fx_reflect(ty0 - 1 - r + yy, H), gx = fx_reflect(tx0 - 1 - r + xx, W);
    s_src[c][yy][xx] = (unsigned char)fx_byte(sb[c * plane + (size_t)gy * W + gx]);
  }
  __syncthreads();

  for (int i = tid; i < 3 * sh * FX_PW; i += 256) {           // rows of the halo too: the vertical pass reads them
    const int c = i / (sh * FX_PW), rem = i - c * (sh * FX_PW);
    const int yy = rem / FX_PW, px = rem - yy * FX_PW;
    const unsigned char* p = &s_src[c][yy][px + r];
    int t = q[0] * (int)p[0];
    for (int k = 1; k <= r; ++k) t += q[k] * ((int)p[-k] + (int)p[k]);
    s_row[c][yy][px] = (unsigned short)t;                     // <= 256 * 255
  }
  __syncthreads();

  const unsigned seed = (unsigned)sd[X_SEED];
  const bool per_channel = sd[X_PER_CHANNEL] != 0;
  const double scale = imgfx_bits_f64(sd + X_SCALE);
  for (int i = tid; i < FX_PH * FX_PW; i += 256) {
    const int py = i / FX_PW, px = i - py * FX_PW;
    const int y = ty0 - 1 + py, x = tx0 - 1 + px;
    if (y < 0 || y >= H || x < 0 || x >= W) continue;         // never read: the sharpen reflects its taps to in-image positions
    const unsigned at = (unsigned)y * (unsigned)W + (unsigned)x;
    int add = 0;
    if (noise && !per_channel) add = fx_noise(seed, at, scale);
    for (int c = 0; c < 3; ++c) {
      int t = q[0] * (int)s_row[c][py + r][px];
      for (int k = 1; k <= r; ++k) t += q[k] * ((int)s_row[c][py + r - k][px] + (int)s_row[c][py + r + k][px]);
      int v = (t + 32768) >> 16;
      if (noise) v = fx_clip255(v + (per_channel ? fx_noise(seed, at * 3u + (unsigned)c, scale) : add));
      s_pix[c][py][px] = s_lut[v];
    }
  }
  __syncthreads();

  const int x = tx0 + ox;
  if (x >= W) return;
  const double kc = (double)imgfx_bits_f32(sd[X_KC]), kn = (double)imgfx_bits_f32(sd[X_KN]);
  const int xl = fx_reflect(x - 1, W) - (tx0 - 1), xr = fx_reflect(x + 1, W) - (tx0 - 1), xc = ox + 1;
  for (int oy = tid >> 6; oy < FX_TH && ty0 + oy < H; oy += 4) {
    const int y = ty0 + oy;
    const int yu = fx_reflect(y - 1, H) - (ty0 - 1), yd = fx_reflect(y + 1, H) - (ty0 - 1), yc = oy + 1;
    for (int c = 0; c < 3; ++c) {
      int v = s_pix[c][yc][xc];
      if (sharpen) {
        const int s8 = (int)s_pix[c][yu][xl] + (int)s_pix[c][yu][xc] + (int)s_pix[c][yu][xr] + (int)s_pix[c][yc][xl] + (int)s_pix[c][yc][xr] +
                       (int)s_pix[c][yd][xl] + (int)s_pix[c][yd][xc] + (int)s_pix[c][yd][xr];
        v = fx_clip255((int)rint(kc * (double)v + kn * (double)s8));          // both products are exact: one rounding
      }
      db[c * plane + (size_t)y * W + x] = (float)v / 255.0f;
    }
  }
}

}  // namespace

extern "C" {

int mdcv_imgfx_batch(const int* fx_host, const int* fx, int B, const unsigned char* luts, int n_luts, int C, int H, int W, const float* src,
                     float* dst, void* stream) {
  if (!fx_host || !fx || !src || !dst) return MDCV_EARG;
  if (B <= 0 || B > 65535 || n_luts < 0 || (n_luts > 0 && !luts)) return MDCV_EARG;
  if (C != 3 || H < IMGFX_MIN_SIDE || W < IMGFX_MIN_SIDE || (long long)H * W > IMGFX_MAX_PIXELS) return MDCV_EARG;
  const unsigned long long bytes = (unsigned long long)B * 3ull * (unsigned long long)H * (unsigned long long)W * 4ull;
  const unsigned long long s0 = (unsigned long long)(size_t)src, d0 = (unsigned long long)(size_t)dst;
  if (s0 < d0 + bytes && d0 < s0 + bytes) return MDCV_EARG;    // out of place: a tile reads its neighbours' halo
  for (int b = 0; b < B; ++b)
    if (!fx_ok(fx_host + (size_t)b * MDCV_IMGFX_DESC, n_luts)) return MDCV_EARG;
  const int tiles_x = (W + FX_TW - 1) / FX_TW, tiles_y = (H + FX_TH - 1) / FX_TH;      // at most 2^24 / (16 * 16) tiles
  const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, 1u, (unsigned)B);
  MDCV_LAUNCH(imgfx_kernel, grid, dim3(256), 0, (hipStream_t)stream, fx, luts, n_luts, H, W, tiles_x, src, dst);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
