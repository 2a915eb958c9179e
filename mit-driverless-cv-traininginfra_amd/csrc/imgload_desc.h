// The per-image descriptor of the real-image loader and the patch pixel it describes, shared by csrc/imgload.hip (the two-launch path) and
// csrc/imgaug.hip (the augmented path, which needs the same patch as uint8 before it jitters and warps it).
#pragma once
#include "common.h"

#define MDCV_IMGLOAD_DESC 20
#define IMGLOAD_PREC 22            // Pillow: PRECISION_BITS = 32 - 8 - 2
#define IMGLOAD_MAX_KSIZE 4096

#define MDCV_IMGLOAD_FREF 4         // long longs per image in the frame-reference table: {off or -1 for "staged", pitch, x0, y0}
#define IMGLOAD_MAX_POOL (1LL << 60)

// csrc/imgload.hip: enqueue the horizontal pass alone (internal; both batch entry points validate their descriptors first).
// fref == nullptr: every image reads its staged window in `src`.
int imgload_launch_hpass(const int* desc, const long long* fref, int B, const int* coefs, long long n_coefs, const unsigned char* src,
                         long long src_bytes, const unsigned char* pool, long long pool_bytes, int max_scr_w, int max_scr_h, void* workspace,
                         void* stream);

namespace {

enum { D_SRC_OFF, D_WIN_W, D_WIN_H, D_KSX, D_KSY, D_CX_OFF, D_CY_OFF, D_SCR_W, D_SCR_H, D_ROW0, D_NY, D_OX_OFF, D_OY_OFF,
       D_PAD_X0, D_PAD_X1, D_PAD_Y0, D_PAD_Y1, D_FLIP, D_RES0, D_RES1 };

enum { F_OFF, F_PITCH, F_X0, F_Y0 };

// Every offset and extent a descriptor names lies inside the buffers it indexes.  The same test runs on the host (MDCV_EARG) and in the
// kernels (on the device copy, which the host never sees): no descriptor can make a kernel read or write outside its buffers.
// It has two halves.  staged_ok / fref_ok: the pixels the horizontal pass reads lie inside `src` / inside the pool.  geom_ok: everything
// behind the source (tables, scratch, flags), which the downstream kernels need whichever buffer the pixels came from.
__host__ __device__ inline bool staged_ok(const int* d, long long src_bytes) {
  if (d[D_SRC_OFF] < 0 || d[D_WIN_W] < 0 || d[D_WIN_H] < 0) return false;
  return (long long)d[D_SRC_OFF] + 3LL * d[D_WIN_W] * d[D_WIN_H] <= src_bytes;
}

__host__ __device__ inline bool geom_ok(const int* d, long long n_coefs, int max_scr_w, int max_scr_h) {
  if (d[D_WIN_W] < 0 || d[D_WIN_H] < 0) return false;
  if (d[D_KSX] < 1 || d[D_KSX] > IMGLOAD_MAX_KSIZE || d[D_KSY] < 1 || d[D_KSY] > IMGLOAD_MAX_KSIZE) return false;
  if (d[D_SCR_W] < 0 || d[D_SCR_W] > max_scr_w || d[D_SCR_H] < 0 || d[D_SCR_H] > max_scr_h || d[D_NY] < 0) return false;
  if (d[D_CX_OFF] < 0 || (long long)d[D_CX_OFF] + (long long)d[D_SCR_W] * (d[D_KSX] + 2) > n_coefs) return false;
  if (d[D_CY_OFF] < 0 || (long long)d[D_CY_OFF] + (long long)d[D_NY] * (d[D_KSY] + 2) > n_coefs) return false;
  if (d[D_FLIP] != 0 && d[D_FLIP] != 1) return false;
  return d[D_RES0] == 0 && d[D_RES1] == 0;
}

__host__ __device__ inline bool desc_ok(const int* d, long long n_coefs, long long src_bytes, int max_scr_w, int max_scr_h) {
  return staged_ok(d, src_bytes) && geom_ok(d, n_coefs, max_scr_w, max_scr_h);
}

// A window referenced in place: pixel (wy, x) is pool[off + (y0 + wy) * pitch + 3 * (x0 + x)].  Good when off, x0, y0 >= 0,
// pitch >= 3 * (x0 + win_w) and off + (y0 + win_h - 1) * pitch + 3 * (x0 + win_w) <= pool_bytes, in 64 bits; the product is tested by
// a division so that no value can wrap it (pool_bytes <= IMGLOAD_MAX_POOL bounds every sum).
__host__ __device__ inline bool fref_ok(const int* d, const long long* f, long long pool_bytes) {
  if (d[D_WIN_W] < 0 || d[D_WIN_H] < 0 || pool_bytes < 0 || pool_bytes > IMGLOAD_MAX_POOL) return false;
  const long long off = f[F_OFF], pitch = f[F_PITCH], x0 = f[F_X0], y0 = f[F_Y0];
  if (off < 0 || x0 < 0 || y0 < 0 || off > pool_bytes || x0 > pool_bytes || y0 > pool_bytes) return false;
  const long long row_bytes = 3 * (x0 + d[D_WIN_W]);
  if (pitch < row_bytes) return false;
  const long long rows = y0 + d[D_WIN_H] - 1;               // full pitches in front of the last row, -1 for an empty window at y0 = 0
  if (rows <= 0) return off + rows * pitch + row_bytes <= pool_bytes;
  const long long room = pool_bytes - off - row_bytes;
  return room >= 0 && pitch <= room / rows;
}

// One image of a batch: `f` is its row of the frame-reference table, nullptr when the batch has none (the two staged entry points).
__host__ __device__ inline bool image_ok(const int* d, const long long* f, long long n_coefs, long long src_bytes, long long pool_bytes,
                                         int max_scr_w, int max_scr_h) {
  if (!f) return desc_ok(d, n_coefs, src_bytes, max_scr_w, max_scr_h);
  if (f[F_OFF] == -1) return desc_ok(d, n_coefs, src_bytes, max_scr_w, max_scr_h);      // staged: the other three words are not read
  return fref_ok(d, f, pool_bytes) && geom_ok(d, n_coefs, max_scr_w, max_scr_h);
}

// The per-image prologue of every kernel: descriptor (and frame reference, when the batch has a table) into LDS.  Call from all threads.
__device__ __forceinline__ const long long* imgload_stage_desc(int* sdesc, long long* sfref, const int* __restrict__ desc,
                                                              const long long* __restrict__ fref, int b, int tid) {
  if (tid < MDCV_IMGLOAD_DESC) sdesc[tid] = desc[(size_t)b * MDCV_IMGLOAD_DESC + tid];
  if (fref && tid >= 32 && tid < 32 + MDCV_IMGLOAD_FREF) sfref[tid - 32] = fref[(size_t)b * MDCV_IMGLOAD_FREF + tid - 32];
  return fref ? sfref : nullptr;
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
