// Real-image detector batches: the image half of ImageLabelDataset.__getitem__ (CVC-YOLOv3/utils/datasets.py:124-315) after the decode.
// Pillow's 8-bit convolution resize (libImaging/Resample.c: separable, horizontal pass into a uint8 image first, 22-bit fixed-point
// coefficients, accumulator seeded with 1 << 21, clipped to 0..255), with the 127 padding and patch crop around it, convert('L'), hflip
// and to_tensor's /255.  The coefficient tables are computed on the host in float64 exactly as Pillow computes them (mdcv/data/images.py)
// and arrive with the pixels; the device only does integer multiply-adds, so the bytes equal Pillow's.
// Two launches per batch whatever the mix of frame sizes: blockIdx.z is the image, and each image's descriptor bounds its own work.
#include "common.h"

#define MDCV_IMGLOAD_DESC 20
#define IMGLOAD_PREC 22            // Pillow: PRECISION_BITS = 32 - 8 - 2
#define IMGLOAD_MAX_KSIZE 4096

namespace {

enum { D_SRC_OFF, D_WIN_W, D_WIN_H, D_KSX, D_KSY, D_CX_OFF, D_CY_OFF, D_SCR_W, D_SCR_H, D_ROW0, D_NY, D_OX_OFF, D_OY_OFF,
       D_PAD_X0, D_PAD_X1, D_PAD_Y0, D_PAD_Y1, D_FLIP, D_RES0, D_RES1 };

// Every offset and extent a descriptor names lies inside the buffers it indexes.  The same test runs on the host (MDCV_EARG) and in both
// kernels (on the device copy, which the host never sees): no descriptor can make a kernel read or write outside its buffers.
__host__ __device__ inline bool desc_ok(const int* d, long long n_coefs, long long src_bytes, int max_scr_w, int max_scr_h) {
  if (d[D_SRC_OFF] < 0 || d[D_WIN_W] < 0 || d[D_WIN_H] < 0) return false;
  if ((long long)d[D_SRC_OFF] + 3LL * d[D_WIN_W] * d[D_WIN_H] > src_bytes) return false;
  if (d[D_KSX] < 1 || d[D_KSX] > IMGLOAD_MAX_KSIZE || d[D_KSY] < 1 || d[D_KSY] > IMGLOAD_MAX_KSIZE) return false;
  if (d[D_SCR_W] < 0 || d[D_SCR_W] > max_scr_w || d[D_SCR_H] < 0 || d[D_SCR_H] > max_scr_h || d[D_NY] < 0) return false;
  if (d[D_CX_OFF] < 0 || (long long)d[D_CX_OFF] + (long long)d[D_SCR_W] * (d[D_KSX] + 2) > n_coefs) return false;
  if (d[D_CY_OFF] < 0 || (long long)d[D_CY_OFF] + (long long)d[D_NY] * (d[D_KSY] + 2) > n_coefs) return false;
  if (d[D_FLIP] != 0 && d[D_FLIP] != 1) return false;
  return d[D_RES0] == 0 && d[D_RES1] == 0;
}

__device__ __forceinline__ int clip8(int v) {     // Pillow's clip8: v >> PRECISION_BITS clamped to 0..255
  v >>= IMGLOAD_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Horizontal pass: scratch[b][i][j] = resize of window row (row0 + i) at resized column j; rows outside the window are the 127 canvas.
// 64 columns x 4 rows per workgroup, rows grid-strided; a lane keeps its column's table entry for all of its rows.
__global__ __launch_bounds__(256) void imgload_hpass_kernel(const int* __restrict__ desc, const int* __restrict__ coefs, long long n_coefs,
                                                            const unsigned char* __restrict__ src, long long src_bytes, int max_scr_w,
                                                            int max_scr_h, unsigned char* __restrict__ ws) {
  __shared__ int sdesc[MDCV_IMGLOAD_DESC];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (tid < MDCV_IMGLOAD_DESC) sdesc[tid] = desc[(size_t)b * MDCV_IMGLOAD_DESC + tid];
  __syncthreads();
  if (!desc_ok(sdesc, n_coefs, src_bytes, max_scr_w, max_scr_h)) return;
  const int scr_w = sdesc[D_SCR_W], scr_h = sdesc[D_SCR_H];
  const int j = blockIdx.x * 64 + (tid & 63);
  if (blockIdx.x * 64 >= scr_w) return;                        // whole workgroup past this image's columns
  const int ks = sdesc[D_KSX], win_w = sdesc[D_WIN_W], win_h = sdesc[D_WIN_H], row0 = sdesc[D_ROW0];
  const int* e = coefs + sdesc[D_CX_OFF] + (size_t)(j < scr_w ? j : scr_w - 1) * (ks + 2);
  const int x0 = e[0];
  const int cnt = e[1] < ks ? e[1] : ks;
  const unsigned char* s = src + sdesc[D_SRC_OFF];
  unsigned char* o = ws + (size_t)b * max_scr_w * max_scr_h * 3;
  if (j >= scr_w) return;
  for (int i = blockIdx.y * 4 + (tid >> 6); i < scr_h; i += gridDim.y * 4) {
    const int wy = row0 + i;
    const bool row_in = wy >= 0 && wy < win_h;
    const unsigned char* r = s + (size_t)(row_in ? wy : 0) * win_w * 3;
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
__global__ __launch_bounds__(256) void imgload_vpass_kernel(const int* __restrict__ desc, const int* __restrict__ coefs, long long n_coefs,
                                                            long long src_bytes, int max_scr_w, int max_scr_h, int C, int H, int W,
                                                            const unsigned char* __restrict__ ws, float* __restrict__ out) {
  __shared__ int sdesc[MDCV_IMGLOAD_DESC];
  const int b = blockIdx.z, tid = threadIdx.x;
  if (tid < MDCV_IMGLOAD_DESC) sdesc[tid] = desc[(size_t)b * MDCV_IMGLOAD_DESC + tid];
  __syncthreads();
  const bool ok = desc_ok(sdesc, n_coefs, src_bytes, max_scr_w, max_scr_h);
  const int ox = blockIdx.x * 64 + (tid & 63);
  if (ox >= W) return;
  const size_t plane = (size_t)H * W;
  float* ob = out + (size_t)b * C * plane;
  const unsigned char* sb = ws + (size_t)b * max_scr_w * max_scr_h * 3;
  for (int oy = blockIdx.y * 4 + (tid >> 6); oy < H; oy += gridDim.y * 4) {
    int v0 = 0, v1 = 0, v2 = 0;
    if (ok) {
      const int xr = (sdesc[D_FLIP] ? W - 1 - ox : ox) + sdesc[D_OX_OFF];
      const int yr = oy + sdesc[D_OY_OFF];
      if (xr >= 0 && xr < sdesc[D_SCR_W] && yr >= 0 && yr < sdesc[D_NY]) {
        const int ks = sdesc[D_KSY], scr_h = sdesc[D_SCR_H];
        const int* e = coefs + sdesc[D_CY_OFF] + (size_t)yr * (ks + 2);
        const int y0 = e[0];
        const int cnt = e[1] < ks ? e[1] : ks;
        int a0 = 1 << (IMGLOAD_PREC - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < cnt; ++t) {
          const int y = y0 + t;
          if (y < 0 || y >= scr_h) continue;                   // only a corrupt table gets here
          const unsigned char* p = sb + ((size_t)y * max_scr_w + xr) * 3;
          const int k = e[2 + t];
          a0 += (int)p[0] * k; a1 += (int)p[1] * k; a2 += (int)p[2] * k;
        }
        v0 = clip8(a0); v1 = clip8(a1); v2 = clip8(a2);
      } else if (xr >= sdesc[D_PAD_X0] && xr < sdesc[D_PAD_X1] && yr >= sdesc[D_PAD_Y0] && yr < sdesc[D_PAD_Y1]) {
        v0 = v1 = v2 = 127;
      }
    }
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

extern "C" {

long long mdcv_imgload_workspace_bytes(int B, int max_scr_w, int max_scr_h) {
  if (B <= 0 || max_scr_w < 0 || max_scr_h < 0) return MDCV_EARG;
  return (long long)B * max_scr_w * max_scr_h * 3;
}

int mdcv_imgload_batch(const int* desc_host, const int* desc, int B, const int* coefs, long long n_coefs, const unsigned char* src,
                       long long src_bytes, int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace, float* out, void* stream) {
  if (!desc_host || !desc || !coefs || !out || B <= 0 || B > 65535 || n_coefs <= 0 || src_bytes < 0 || (src_bytes > 0 && !src)) return MDCV_EARG;
  if (max_scr_w < 0 || max_scr_h < 0 || (!workspace && (long long)max_scr_w * max_scr_h > 0)) return MDCV_EARG;
  if ((C != 1 && C != 3) || H <= 0 || W <= 0) return MDCV_EARG;
  for (int b = 0; b < B; ++b)
    if (!desc_ok(desc_host + (size_t)b * MDCV_IMGLOAD_DESC, n_coefs, src_bytes, max_scr_w, max_scr_h)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* s = src ? src : reinterpret_cast<const unsigned char*>(coefs);      // no window bytes at all: every read is the canvas
  unsigned char* ws = (unsigned char*)workspace;
  if ((long long)max_scr_w * max_scr_h > 0) {
    const unsigned gy = (unsigned)(max_scr_h + 3) / 4 < 64u ? (unsigned)(max_scr_h + 3) / 4 : 64u;
    MDCV_LAUNCH(imgload_hpass_kernel, dim3((unsigned)(max_scr_w + 63) / 64, gy, (unsigned)B), dim3(256), 0, st, desc, coefs, n_coefs, s,
                src_bytes, max_scr_w, max_scr_h, ws);
    MDCV_CHECK_LAUNCH();
  }
  const unsigned gy = (unsigned)(H + 3) / 4 < 64u ? (unsigned)(H + 3) / 4 : 64u;
  MDCV_LAUNCH(imgload_vpass_kernel, dim3((unsigned)(W + 63) / 64, gy, (unsigned)B), dim3(256), 0, st, desc, coefs, n_coefs, src_bytes,
              max_scr_w, max_scr_h, C, H, W, ws, out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
