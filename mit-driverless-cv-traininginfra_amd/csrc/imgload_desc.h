// The per-image descriptor of the real-image loader and the patch pixel it describes, shared by csrc/imgload.hip (the two-launch path) and
// csrc/imgaug.hip (the augmented path, which needs the same patch as uint8 before it jitters and warps it).
#pragma once
#include "common.h"

#define MDCV_IMGLOAD_DESC 20
#define IMGLOAD_PREC 22            // Pillow: PRECISION_BITS = 32 - 8 - 2
#define IMGLOAD_MAX_KSIZE 4096

// csrc/imgload.hip: enqueue the horizontal pass alone (internal; both batch entry points validate their descriptors first)
int imgload_launch_hpass(const int* desc, int B, const int* coefs, long long n_coefs, const unsigned char* src, long long src_bytes,
                         int max_scr_w, int max_scr_h, void* workspace, void* stream);

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

// One pixel of the uint8 patch: the vertical resize at patch position (x, oy) from the horizontal pass's scratch `sb`, the 127 padding
// around the resized image, 0 outside both.
__device__ __forceinline__ void imgload_patch_pixel(const int* sdesc, const int* __restrict__ coefs, const unsigned char* __restrict__ sb,
                                                    int max_scr_w, int x, int oy, int& v0, int& v1, int& v2) {
  v0 = v1 = v2 = 0;
  const int xr = x + sdesc[D_OX_OFF];
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

}  // namespace
