// Real-image detector batches: the image half of ImageLabelDataset.__getitem__ (CVC-YOLOv3/utils/datasets.py:124-315) after the decode.
// Pillow's 8-bit convolution resize (libImaging/Resample.c: separable, horizontal pass into a uint8 image first, 22-bit fixed-point
// coefficients, accumulator seeded with 1 << 21, clipped to 0..255), with the 127 padding and patch crop around it, convert('L'), hflip
// and to_tensor's /255.  The coefficient tables are computed on the host in float64 exactly as Pillow computes them (mdcv/data/images.py)
// and arrive with the pixels; the device only does integer multiply-adds, so the bytes equal Pillow's.
// Two launches per batch whatever the mix of frame sizes: blockIdx.z is the image, and each image's descriptor bounds its own work.
#include "common.h"

#include "imgload_desc.h"

namespace {

// Horizontal pass: scratch[b][i][j] = resize of window row (row0 + i) at resized column j; rows outside the window are the 127 canvas.
// 64 columns x 4 rows per workgroup, rows grid-strided; a lane keeps its column's table entry for all of its rows.
// The window's bytes are either staged (packed rows of 3 * win_w at src + src_off) or a rectangle of a cached frame in `pool`, named by
// the image's row of `fref`; only the base pointer and the row pitch differ, the taps and the canvas are the same.
__global__ __launch_bounds__(256) void imgload_hpass_kernel(const int* __restrict__ desc, const long long* __restrict__ fref,
                                                            const int* __restrict__ coefs, long long n_coefs,
                                                            const unsigned char* __restrict__ src, long long src_bytes,
                                                            const unsigned char* __restrict__ pool, long long pool_bytes, int max_scr_w,
                                                            int max_scr_h, unsigned char* __restrict__ ws) {
  __shared__ int sdesc[MDCV_IMGLOAD_DESC];
  __shared__ long long sfref[MDCV_IMGLOAD_FREF];
  const int b = blockIdx.z, tid = threadIdx.x;
  const long long* f = imgload_stage_desc(sdesc, sfref, desc, fref, b, tid);
  __syncthreads();
  if (!image_ok(sdesc, f, n_coefs, src_bytes, pool_bytes, max_scr_w, max_scr_h)) return;
  const int scr_w = sdesc[D_SCR_W], scr_h = sdesc[D_SCR_H];
  const int j = blockIdx.x * 64 + (tid & 63);
  if (blockIdx.x * 64 >= scr_w) return;                        // whole workgroup past this image's columns
  const int ks = sdesc[D_KSX], win_w = sdesc[D_WIN_W], win_h = sdesc[D_WIN_H], row0 = sdesc[D_ROW0];
  const int* e = coefs + sdesc[D_CX_OFF] + (size_t)(j < scr_w ? j : scr_w - 1) * (ks + 2);
  const int x0 = e[0];
  const int cnt = e[1] < ks ? e[1] : ks;
  const bool pooled = f && f[F_OFF] != -1;
  const size_t pitch = pooled ? (size_t)f[F_PITCH] : (size_t)win_w * 3;
  const unsigned char* s = pooled ? pool + f[F_OFF] + (size_t)f[F_Y0] * pitch + 3 * (size_t)f[F_X0] : src + sdesc[D_SRC_OFF];
  unsigned char* o = ws + (size_t)b * max_scr_w * max_scr_h * 3;
  if (j >= scr_w) return;
  for (int i = blockIdx.y * 4 + (tid >> 6); i < scr_h; i += gridDim.y * 4) {
    const int wy = row0 + i;
    const bool row_in = wy >= 0 && wy < win_h;
    const unsigned char* r = s + (size_t)(row_in ? wy : 0) * pitch;
    int a0 = 1 << (IMGLOAD_PREC - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < cnt; ++t) {
      const int x = x0 + t;
      const int k = e[2 + t];
      int v0 = 127, v1 = 127, v2 = 127;
      if (row_in && x >= 0 && x < win_w) { v0 = r[3 * x]; v1 = r[3 * x + 1]; v2 = r[3 * x + 2]; }
      a0 += v0 * k; a1 += v1 * k; a2 += v2 * k;
    }
    unsigned char* p = o + ((size_t)i * max_scr_w + j) * 3;
    p[0] = (unsigned char)clip8(a0); p[1] = (unsigned char)clip8(a1); p[2] = (unsigned char)clip8(a2);
  }
}

// Vertical pass and everything after it: resize along y from the scratch, 127 padding / 0 outside, convert('L'), hflip, /255, NCHW fp32.
__global__ __launch_bounds__(256) void imgload_vpass_kernel(const int* __restrict__ desc, const long long* __restrict__ fref,
                                                            const int* __restrict__ coefs, long long n_coefs, long long src_bytes,
                                                            long long pool_bytes, int max_scr_w, int max_scr_h, int C, int H, int W,
                                                            const unsigned char* __restrict__ ws, float* __restrict__ out) {
  __shared__ int sdesc[MDCV_IMGLOAD_DESC];
  __shared__ long long sfref[MDCV_IMGLOAD_FREF];
  const int b = blockIdx.z, tid = threadIdx.x;
  const long long* f = imgload_stage_desc(sdesc, sfref, desc, fref, b, tid);
  __syncthreads();
  const bool ok = image_ok(sdesc, f, n_coefs, src_bytes, pool_bytes, max_scr_w, max_scr_h);
  const int ox = blockIdx.x * 64 + (tid & 63);
  if (ox >= W) return;
  const size_t plane = (size_t)H * W;
  float* ob = out + (size_t)b * C * plane;
  const unsigned char* sb = ws + (size_t)b * max_scr_w * max_scr_h * 3;
  for (int oy = blockIdx.y * 4 + (tid >> 6); oy < H; oy += gridDim.y * 4) {
    int v0 = 0, v1 = 0, v2 = 0;
    if (ok) imgload_patch_pixel(sdesc, coefs, sb, max_scr_w, sdesc[D_FLIP] ? W - 1 - ox : ox, oy, v0, v1, v2);
    float* o = ob + (size_t)oy * W + ox;
    if (C == 1) {
      const int l = (v0 * 19595 + v1 * 38470 + v2 * 7471 + 0x8000) >> 16;     // Pillow convert('L')
      o[0] = (float)l / 255.0f;
    } else {
      o[0] = (float)v0 / 255.0f; o[plane] = (float)v1 / 255.0f; o[2 * plane] = (float)v2 / 255.0f;
    }
  }
}

}  // namespace

int imgload_launch_hpass(const int* desc, const long long* fref, int B, const int* coefs, long long n_coefs, const unsigned char* src,
                         long long src_bytes, const unsigned char* pool, long long pool_bytes, int max_scr_w, int max_scr_h, void* workspace,
                         void* stream) {
  const unsigned char* s = src ? src : reinterpret_cast<const unsigned char*>(coefs);      // no window bytes at all: every read is the canvas
  const unsigned char* q = pool ? pool : s;                                                 // no pool: no reference passes with pool_bytes 0
  const unsigned gy = (unsigned)(max_scr_h + 3) / 4 < 64u ? (unsigned)(max_scr_h + 3) / 4 : 64u;
  MDCV_LAUNCH(imgload_hpass_kernel, dim3((unsigned)(max_scr_w + 63) / 64, gy, (unsigned)B), dim3(256), 0, (hipStream_t)stream, desc, fref,
              coefs, n_coefs, s, src_bytes, q, pool_bytes, max_scr_w, max_scr_h, (unsigned char*)workspace);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

namespace {

// Both entry points: fref_host == fref == nullptr is the staged form.
int imgload_batch_impl(const int* desc_host, const int* desc, const long long* fref_host, const long long* fref, int B, const int* coefs,
                       long long n_coefs, const unsigned char* src, long long src_bytes, const unsigned char* pool, long long pool_bytes,
                       int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace, float* out, void* stream) {
  if (!desc_host || !desc || !coefs || !out || B <= 0 || B > 65535 || n_coefs <= 0 || src_bytes < 0 || (src_bytes > 0 && !src)) return MDCV_EARG;
  if (pool_bytes < 0 || pool_bytes > IMGLOAD_MAX_POOL || (pool_bytes > 0 && !pool)) return MDCV_EARG;
  if (max_scr_w < 0 || max_scr_h < 0 || (!workspace && (long long)max_scr_w * max_scr_h > 0)) return MDCV_EARG;
  if ((C != 1 && C != 3) || H <= 0 || W <= 0) return MDCV_EARG;
  for (int b = 0; b < B; ++b)
    if (!image_ok(desc_host + (size_t)b * MDCV_IMGLOAD_DESC, fref_host ? fref_host + (size_t)b * MDCV_IMGLOAD_FREF : nullptr, n_coefs,
                  src_bytes, pool_bytes, max_scr_w, max_scr_h))
      return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* ws = (const unsigned char*)workspace;
  if ((long long)max_scr_w * max_scr_h > 0) {
    const int rc = imgload_launch_hpass(desc, fref, B, coefs, n_coefs, src, src_bytes, pool, pool_bytes, max_scr_w, max_scr_h, workspace, stream);
    if (rc != MDCV_OK) return rc;
  }
  const unsigned gy = (unsigned)(H + 3) / 4 < 64u ? (unsigned)(H + 3) / 4 : 64u;
  MDCV_LAUNCH(imgload_vpass_kernel, dim3((unsigned)(W + 63) / 64, gy, (unsigned)B), dim3(256), 0, st, desc, fref, coefs, n_coefs, src_bytes,
              pool_bytes, max_scr_w, max_scr_h, C, H, W, ws, out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // namespace

extern "C" {

long long mdcv_imgload_workspace_bytes(int B, int max_scr_w, int max_scr_h) {
  if (B <= 0 || max_scr_w < 0 || max_scr_h < 0) return MDCV_EARG;
  return (long long)B * max_scr_w * max_scr_h * 3;
}

int mdcv_imgload_batch(const int* desc_host, const int* desc, int B, const int* coefs, long long n_coefs, const unsigned char* src,
                       long long src_bytes, int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace, float* out, void* stream) {
  return imgload_batch_impl(desc_host, desc, nullptr, nullptr, B, coefs, n_coefs, src, src_bytes, nullptr, 0, max_scr_w, max_scr_h, C, H, W,
                            workspace, out, stream);
}

int mdcv_imgload_frames_batch(const int* desc_host, const int* desc, const long long* fref_host, const long long* fref, int B, const int* coefs,
                              long long n_coefs, const unsigned char* src, long long src_bytes, const unsigned char* pool, long long pool_bytes,
                              int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace, float* out, void* stream) {
  if (!fref_host || !fref) return MDCV_EARG;
  return imgload_batch_impl(desc_host, desc, fref_host, fref, B, coefs, n_coefs, src, src_bytes, pool, pool_bytes, max_scr_w, max_scr_h, C, H, W,
                            workspace, out, stream);
}

}  // extern "C"
