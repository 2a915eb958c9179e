// The tail of single_img_detect (CVC-YOLOv3/detect.py:99-104) for a whole batch in one launch: every kept box of every frame is mapped
// from detector to frame coordinates and its outline is drawn into the decoded frame where it lies in a device pool (uint8, HWC, RGB, rows
// of 3 * W bytes: the pool mdcv_imgload_frames_batch reads).  The reference does this on the host, four .item() reads and one
// ImageDraw.rectangle per box.  Grid (K, B), one workgroup per (box slot, frame); a slot k >= count[b] exits at once, so the host never
// reads the counts.  Per box:
//   a. map       (double)v / ratio - pad in IEEE double, as Python computes `x.item() / ratio - pad_w` (detect.py:100-103) -> frame_boxes
//   b. validate  x1 < x0 or y1 < y0 (as doubles: where Pillow raises), or a coordinate that is not finite or has magnitude >= 2^30 (where
//                C's conversion to int is undefined): not drawn, rect (0, 0, -1, -1), skipped[b] += 1
//   c. truncate  (int) of the double, toward zero -> rects
//   d. outline   Pillow 12.2's ImagingDrawRectangle for width 1 without fill: rows y0 and y1 from x0 to x1 inclusive; columns x0 and x1
//                over every row between y0 + 1 and y1 inclusive, in either order -- with y1 == y0 that is row y0 + 1, which then gets the
//                two end pixels (Pillow's quirk, reproduced); everything clipped to the frame
// ONE colour per launch: overlapping boxes, of one workgroup or of several, store identical bytes to a pixel, so no order between
// workgroups (or between the lanes of one) is needed and the result does not depend on any.  That is why there are no per-box colours.
// Stores: a horizontal edge is one contiguous run of 3 * n bytes holding R G B R G B ...; its lanes write the 4-byte-aligned dwords of the
// run, one per lane, consecutive lanes consecutive addresses (the dword's bytes depend on its offset modulo 3: three patterns), and single
// bytes only for the at most 3 + 3 bytes in front of and behind them.  The vertical edges are 3 bytes per row, a row pitch apart: byte
// stores, one pixel per lane.  Plain vector stores only.  The launch is latency-sized (a box's outline is a few hundred bytes to a few KB):
// 256 lanes cover the perimeter of a typical box in one or two trips; no LDS, no barrier, a handful of registers.
// mdcv_detect_map_boxes runs steps a to c alone (the same kernel with `draw` off, so the same bytes in frame_boxes / rects / skipped): the
// cone pipeline maps first, reads the crops out of the untouched frames, and draws afterwards (csrc/kpt_detect.hip).
// Built with -ffp-contract=off like the other byte-exact units (the map is a division and a subtraction: nothing to contract, and kept so).
#include "common.h"
#include "detect_desc.h"

namespace {

constexpr double kLimit = 1073741824.0;        // 2^30

struct DrawArgs {
  const long long* desc;
  const float* boxes;
  const int* count;
  int K;
  unsigned char* pool;
  long long pool_bytes;
  unsigned c0, c1, c2;
  double* frame_boxes;
  int* rects;
  int* skipped;
  int draw;                                      // 0: mdcv_detect_map_boxes, steps a to c only
};

struct Ink { unsigned c0, c1, c2, p0, p1, p2; };      // the three bytes, and the dword of a run at byte offsets 0, 1, 2 modulo 3

__device__ __forceinline__ unsigned pick3(int i, unsigned a, unsigned b, unsigned c) { return i == 0 ? a : (i == 1 ? b : c); }

// the run of n pixels that starts at p: bytes c0 c1 c2 c0 ...
__device__ __forceinline__ void store_run(unsigned char* p, int n, const Ink& k, int tid) {
  const int bytes = 3 * n;
  int head = (int)((4 - ((uintptr_t)p & 3)) & 3);
  if (head > bytes) head = bytes;
  const int nd = (bytes - head) >> 2;
  const int tail0 = head + 4 * nd;
  unsigned* q = reinterpret_cast<unsigned*>(p + head);
  for (int j = tid; j < nd; j += 256) q[j] = pick3((head + 4 * j) % 3, k.p0, k.p1, k.p2);
  if (tid < head) p[tid] = (unsigned char)pick3(tid % 3, k.c0, k.c1, k.c2);
  if (tid < bytes - tail0) p[tail0 + tid] = (unsigned char)pick3((tail0 + tid) % 3, k.c0, k.c1, k.c2);
}

__global__ __launch_bounds__(256) void detect_draw_kernel(DrawArgs A) {
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (k >= A.count[b]) return;
  const long long* d = A.desc + (size_t)b * MDCV_DETECT_DESC;
  const double ratio = detect_desc_ratio(d);
  const double pw = (double)d[DD_PAD_W], ph = (double)d[DD_PAD_H];
  const size_t slot = ((size_t)b * A.K + k) * 4;
  const float* bx = A.boxes + slot;
  double v[4];
  v[0] = (double)bx[0] / ratio - pw;
  v[1] = (double)bx[1] / ratio - ph;
  v[2] = (double)bx[2] / ratio - pw;
  v[3] = (double)bx[3] / ratio - ph;
  bool ok = !(v[2] < v[0]) && !(v[3] < v[1]);
#pragma unroll
  for (int j = 0; j < 4; ++j) ok = ok && (fabs(v[j]) < kLimit);          // false for NaN and +-inf as well
  int r[4] = {0, 0, -1, -1};
  if (ok) {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (int)v[j];
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { A.frame_boxes[slot + j] = v[j]; A.rects[slot + j] = r[j]; }
    if (!ok) atomicAdd(A.skipped + b, 1);                                 // integer: the total does not depend on the order
  }
  // the host entry validated its copy of the table; the device copy is checked again so that no descriptor can index outside the pool
  if (!A.draw || !ok || !detect_frame_ok(d, A.pool_bytes)) return;
  const int W = (int)d[DD_W], H = (int)d[DD_H];
  const size_t pitch = (size_t)3 * W;
  unsigned char* __restrict__ frame = A.pool + d[DD_OFF];
  const unsigned c0 = A.c0, c1 = A.c1, c2 = A.c2;
  const int x0 = r[0], y0 = r[1], x1 = r[2], y1 = r[3];
  const int cx0 = x0 < 0 ? 0 : x0, cx1 = x1 > W - 1 ? W - 1 : x1;
  if (cx0 <= cx1) {
    const Ink ink{c0, c1, c2, c0 | (c1 << 8) | (c2 << 16) | (c0 << 24), c1 | (c2 << 8) | (c0 << 16) | (c1 << 24),
                  c2 | (c0 << 8) | (c1 << 16) | (c2 << 24)};
    if (y0 >= 0 && y0 < H) store_run(frame + (size_t)y0 * pitch + (size_t)3 * cx0, cx1 - cx0 + 1, ink, tid);
    if (y1 != y0 && y1 >= 0 && y1 < H) store_run(frame + (size_t)y1 * pitch + (size_t)3 * cx0, cx1 - cx0 + 1, ink, tid);
  }
  int lo = y0 + 1, hi = y1 > y0 + 1 ? y1 : y0 + 1;                        // |coordinates| < 2^30: no overflow
  if (lo < 0) lo = 0;
  if (hi > H - 1) hi = H - 1;
  const bool in0 = x0 >= 0 && x0 < W, in1 = x1 >= 0 && x1 < W;
  if (hi < lo || !(in0 || in1)) return;
  const int items = 2 * (hi - lo + 1);                                   // <= 2^25
  for (int i = tid; i < items; i += 256) {
    const int side = i & 1, y = lo + (i >> 1);
    if (side ? in1 : in0) {
      unsigned char* p = frame + (size_t)y * pitch + (size_t)3 * (side ? x1 : x0);
      p[0] = (unsigned char)c0; p[1] = (unsigned char)c1; p[2] = (unsigned char)c2;
    }
  }
}

}  // namespace

extern "C" {

// both entry points: the same checks, the same memset, the same kernel; `draw` == 0 stops a box after its tables are written
static int map_or_draw(const long long* desc_host, const long long* desc, int B, const float* boxes, const int* count, int K,
                       unsigned char* pool, long long pool_bytes, int red, int green, int blue, double* frame_boxes, int* rects,
                       int* skipped, int draw, void* stream) {
  if (B < 0 || K < 0 || B > 65535 || K > 65535 || pool_bytes < 0 || pool_bytes > (1ll << 60)) return MDCV_EARG;
  if (red < 0 || red > 255 || green < 0 || green > 255 || blue < 0 || blue > 255) return MDCV_EARG;
  if (B == 0) return MDCV_OK;
  if (!desc_host || !desc || !count || !skipped || (draw && !pool && pool_bytes > 0)) return MDCV_EARG;
  if (K > 0 && (!boxes || !frame_boxes || !rects)) return MDCV_EARG;
  for (int b = 0; b < B; ++b) {
    const long long* d = desc_host + (size_t)b * MDCV_DETECT_DESC;
    const double ratio = detect_desc_ratio(d);
    if (!detect_frame_ok(d, pool_bytes) || !(ratio > 0.0) || !(ratio < kLimit)) return MDCV_EARG;
  }
  if (K == 0) return MDCV_OK;                                            // nothing can be kept: nothing is launched or written
  hipError_t e = hipMemsetAsync(skipped, 0, (size_t)B * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  DrawArgs a{desc, boxes, count, K, pool, pool_bytes, (unsigned)red, (unsigned)green, (unsigned)blue, frame_boxes, rects, skipped, draw};
  MDCV_LAUNCH(detect_draw_kernel, dim3((unsigned)K, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_detect_draw_boxes(const long long* desc_host, const long long* desc, int B, const float* boxes, const int* count, int K,
                           unsigned char* pool, long long pool_bytes, int red, int green, int blue, double* frame_boxes, int* rects,
                           int* skipped, void* stream) {
  return map_or_draw(desc_host, desc, B, boxes, count, K, pool, pool_bytes, red, green, blue, frame_boxes, rects, skipped, 1, stream);
}

int mdcv_detect_map_boxes(const long long* desc_host, const long long* desc, int B, const float* boxes, const int* count, int K,
                          long long pool_bytes, double* frame_boxes, int* rects, int* skipped, void* stream) {
  return map_or_draw(desc_host, desc, B, boxes, count, K, nullptr, pool_bytes, 0, 0, 0, frame_boxes, rects, skipped, 0, stream);
}

}  // extern "C"
