// Cone key points on whole frames, drawn on the device: the three launches between the detector's rects and the annotated pixels
// (mdcv/yolo/detect.py FrameConeDetector, mdcv/rektnet/detect.py KeypointDetector; RektNet/detect.py and RektNet/utils.py:61-66).
//
//   a. mdcv_crop_resize_frames_u8   every kept box of every frame is cut out of the frame WHERE IT LIES in the device pool (uint8, HWC, RGB,
//      rows of 3 * W bytes at unaligned offsets) and resized to S x S with mdcv_kptload_batch's rule: cv2's 8-bit INTER_LINEAR in 11-bit
//      fixed point (resize_u8.h), then (float)(u8 / 255.0), planes B, G, R -- the pool is RGB, so plane p reads byte 2 - p of a pixel.
//      Grid (per, B, 3): one workgroup per (box slot, frame, plane).  The row of a crop is the number of boxes WITH a crop in front of it
//      in (frame, slot) order: every workgroup counts them itself from rects / count / desc (at most B * per window tests, 256 lanes, one
//      integer LDS atomic each), so there is no second launch, no grid barrier and no host read.  That count bounds the launch: B * per is
//      limited to 2^20, where the slowest workgroup makes 4096 trips of a few integer compares; at the production 16 x 200 it is 13.
//      Workgroup (0, 0, 0) also counts all of them -> total.  The resize itself is 32 * S bytes of taps in LDS and S * S outputs of 4
//      byte loads each; store-bound like kptload_kernel, 16 bytes per lane where S % 4 == 0.
//   b. mdcv_kpt_draw_points   cv2.circle(img, c, 2, colour, -1) for the 7 key points of every cone.  One workgroup per cone; lane t < 91
//      owns pixel t % 13 of the 13-pixel disc of point t / 13 and stores its 3 bytes only if NO LATER point covers that pixel: the later
//      points of its own cone (7 centres in LDS) and the 7 points of every later cone of the same image (the run of rows behind it with
//      the same owner), whose centres the workgroup recomputes 36 cones at a time into LDS.  So each pixel is stored by exactly one lane
//      of the whole launch -- the last writer of the reference's sequential loop -- and no order between lanes or workgroups is relied on.
//      The disc of radius 2 is |dx| + |dy| <= 2.  Bound: (cones of one image / 36) trips of two barriers; a few KB stored in all.
//   c. mdcv_kpt_heatmap_mosaic   RektNet/detect.py:40-48.  Grid (7, B), one workgroup per map: min / max through LDS (fminf / fmaxf and a
//      NaN flag: the result does not depend on the order), then one byte per element.  S * S floats in twice, S * S bytes out.
//
// Plain vector stores and plain C++ only.  Byte-exact against tests/helpers/kpt_draw_numpy.py, so built with -ffp-contract=off like
// detect_draw.hip and kptload.hip: (double)pt * w is one IEEE product, and kernel c's float32 subtraction and division round one by one.
// The division must be the correctly rounded one: that is hipcc's default (-fhip-fp32-correctly-rounded-divide-sqrt); building this file
// with -fno-hip-fp32-correctly-rounded-divide-sqrt or -ffast-math breaks the mosaic's parity with NumPy.
#include "common.h"
#include "detect_desc.h"
#include "resize_u8.h"

namespace {

constexpr double kLimit = 1073741824.0;        // 2^30
constexpr int kMaxPairs = 1 << 20;             // B * per of kernel a, M of kernel b
constexpr int kChunk = 36;                     // cones per LDS refill of kernel b: 252 points

// ------------------------------------------------------------------------------------------------------------------------- kernel a
struct CropArgs {
  const long long* desc; int B;
  const unsigned char* pool; long long pool_bytes;
  const int* rects; const int* count;
  int K, per, S, vec;
  float* crops; int* owner; int* window; int* total;
};

// the clipped window of slot k of frame b, both ends inclusive; false: the box has no crop
__device__ __forceinline__ bool crop_window(const CropArgs& A, int b, int k, int& x0, int& y0, int& w, int& h) {
  const long long* d = A.desc + (size_t)b * MDCV_DETECT_DESC;
  if (k >= A.count[b] || !detect_frame_ok(d, A.pool_bytes)) return false;
  const int W = (int)d[DD_W], H = (int)d[DD_H];
  const int* r = A.rects + ((size_t)b * A.K + k) * 4;
  const int cx0 = r[0] > 0 ? r[0] : 0, cy0 = r[1] > 0 ? r[1] : 0;
  const int cx1 = r[2] < W - 1 ? r[2] : W - 1, cy1 = r[3] < H - 1 ? r[3] : H - 1;
  if (cx1 < cx0 || cy1 < cy0) return false;                               // the skipped rect (0, 0, -1, -1) ends here
  x0 = cx0; y0 = cy0; w = cx1 - cx0 + 1; h = cy1 - cy0 + 1;               // inside [0, 2^24): no overflow
  return w <= MDCV_KPTLOAD_MAX_SIDE && h <= MDCV_KPTLOAD_MAX_SIDE;
}

// boxes with a crop among the first `n` (frame, slot) pairs, image-major; every lane gets the sum
__device__ __forceinline__ int crops_before(const CropArgs& A, int n, int* acc, int tid) {
  if (tid == 0) *acc = 0;
  __syncthreads();
  int mine = 0, x0, y0, w, h;
  for (int i = tid; i < n; i += 256) mine += crop_window(A, i / A.per, i % A.per, x0, y0, w, h) ? 1 : 0;
  if (mine) atomicAdd(acc, mine);                                         // integer: the sum does not depend on the order
  __syncthreads();
  const int sum = *acc;
  __syncthreads();
  return sum;
}

__global__ __launch_bounds__(256) void crop_frames_kernel(CropArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = blockIdx.x, b = blockIdx.y, plane = blockIdx.z, tid = threadIdx.x, S = A.S;
  int* x0 = reinterpret_cast<int*>(smem);                      // byte offset of the tap's channel inside a frame row
  int *x1 = x0 + S, *a0 = x0 + 2 * S, *a1 = x0 + 3 * S;
  int *y0 = x0 + 4 * S, *y1 = x0 + 5 * S, *b0 = x0 + 6 * S, *b1 = x0 + 7 * S;   // y0, y1: window row
  int* acc = x0 + 8 * S;
  if (k == 0 && b == 0 && plane == 0) {
    const int all = crops_before(A, A.B * A.per, acc, tid);
    if (tid == 0) *A.total = all;
  }
  int wx, wy, w, h;
  if (!crop_window(A, b, k, wx, wy, w, h)) return;             // uniform over the workgroup
  const int m = crops_before(A, b * A.per + k, acc, tid);
  if (plane == 0 && tid == 0) {
    A.owner[2 * (size_t)m] = b; A.owner[2 * (size_t)m + 1] = k;
    int* win = A.window + 4 * (size_t)m;
    win[0] = wx; win[1] = wy; win[2] = w; win[3] = h;
  }
  const int ch = 2 - plane;                                    // the frame is RGB, the output B, G, R
  for (int i = tid; i < 2 * S; i += 256) {
    int i0, i1, c0, c1;
    if (i < S) {
      make_tap_u8(i, S, w, true, i0, i1, c0, c1);
      x0[i] = i0 * 3 + ch; x1[i] = i1 * 3 + ch; a0[i] = c0; a1[i] = c1;
    } else {
      const int j = i - S;
      make_tap_u8(j, S, h, false, i0, i1, c0, c1);
      y0[j] = i0; y1[j] = i1; b0[j] = c0; b1[j] = c1;
    }
  }
  __syncthreads();
  const long long* d = A.desc + (size_t)b * MDCV_DETECT_DESC;
  const size_t pitch = (size_t)3 * (size_t)d[DD_W];
  const unsigned char* __restrict__ src = A.pool + d[DD_OFF] + (size_t)wy * pitch + (size_t)3 * wx;
  float* __restrict__ out = A.crops + ((size_t)m * 3 + plane) * S * S;
  if (A.vec) {
    const int S4 = S >> 2;
    for (int i = tid; i < S * S4; i += 256) {
      const int y = i / S4, x = (i - y * S4) * 4;
      const unsigned char* r0 = src + (size_t)y0[y] * pitch;
      const unsigned char* r1 = src + (size_t)y1[y] * pitch;
      const int c0 = b0[y], c1 = b1[y];
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e0 = (int)r0[x0[x + j]] * a0[x + j] + (int)r0[x1[x + j]] * a1[x + j];
        const int e1 = (int)r1[x0[x + j]] * a0[x + j] + (int)r1[x1[x + j]] * a1[x + j];
        o[j] = blend_rows_u8(c0, e0, c1, e1);
      }
      *reinterpret_cast<f32x4_t*>(out + (size_t)i * 4) = o;
    }
  } else {
    for (int i = tid; i < S * S; i += 256) {
      const int y = i / S, x = i - y * S;
      const unsigned char* r0 = src + (size_t)y0[y] * pitch;
      const unsigned char* r1 = src + (size_t)y1[y] * pitch;
      const int e0 = (int)r0[x0[x]] * a0[x] + (int)r0[x1[x]] * a1[x];
      const int e1 = (int)r1[x0[x]] * a0[x] + (int)r1[x1[x]] * a1[x];
      out[i] = blend_rows_u8(b0[y], e0, b1[y], e1);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------- kernel b
struct PointArgs {
  const long long* desc; int n_images;
  unsigned char* pool; long long pool_bytes;
  const float* pts; const int* window; const int* owner; int M;
  unsigned char ink[21];
  int* centers; int* skipped;
};

// a cone can be drawn when its image exists, the image's descriptor is good and its window lies inside the image
__device__ __forceinline__ bool cone_ok(const PointArgs& A, int m, int img) {
  if (img < 0 || img >= A.n_images) return false;
  const long long* d = A.desc + (size_t)img * MDCV_DETECT_DESC;
  if (!detect_frame_ok(d, A.pool_bytes)) return false;
  const int* win = A.window + 4 * (size_t)m;
  const long long W = d[DD_W], H = d[DD_H];
  return win[0] >= 0 && win[1] >= 0 && win[2] >= 1 && win[3] >= 1 && (long long)win[0] + win[2] <= W && (long long)win[1] + win[3] <= H;
}

// the centre of key point i of cone m (whose cone_ok holds): window origin + (int)((double)pt * side), toward zero; false: not drawn
__device__ __forceinline__ bool point_center(const PointArgs& A, int m, int i, int& cx, int& cy) {
  const int* win = A.window + 4 * (size_t)m;
  const float* p = A.pts + ((size_t)m * 7 + i) * 2;
  const double px = (double)p[0] * (double)win[2], py = (double)p[1] * (double)win[3];
  if (!(fabs(px) < kLimit) || !(fabs(py) < kLimit)) return false;         // NaN and +-inf fail this too
  cx = win[0] + (int)px; cy = win[1] + (int)py;                           // |.| < 2^24 + 2^30
  return true;
}

__device__ __forceinline__ bool covers(int cx, int cy, int px, int py) {   // px, py inside a frame: the differences fit an int
  const int dx = px - cx, dy = py - cy;
  return (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= 2;
}

__global__ __launch_bounds__(256) void kpt_draw_kernel(PointArgs A) {
  __shared__ int own_x[7], own_y[7], own_ok[7];
  __shared__ int lx[7 * kChunk], ly[7 * kChunk], lok[7 * kChunk];
  __shared__ int run_end;
  const int m = blockIdx.x, tid = threadIdx.x;
  const int img = A.owner[2 * (size_t)m];
  const bool good = cone_ok(A, m, img);
  if (tid == 0) run_end = A.M;
  __syncthreads();
  if (tid < 7) {
    int cx = -1, cy = -1;
    const bool ok = good && point_center(A, m, tid, cx, cy);
    if (!ok) {
      cx = cy = -1;
      if (img >= 0 && img < A.n_images) atomicAdd(A.skipped + img, 1);    // integer: the total does not depend on the order
    }
    own_x[tid] = cx; own_y[tid] = cy; own_ok[tid] = ok ? 1 : 0;
    int* c = A.centers + ((size_t)m * 7 + tid) * 2;
    c[0] = cx; c[1] = cy;
  }
  for (int j = m + 1 + tid; j < A.M; j += 256)                            // the run of later cones of this image ends at the first other owner
    if (A.owner[2 * (size_t)j] != img) { atomicMin(&run_end, j); break; }
  __syncthreads();
  if (!good) return;                                                      // uniform
  const long long* d = A.desc + (size_t)img * MDCV_DETECT_DESC;
  const int W = (int)d[DD_W], H = (int)d[DD_H];
  const int p = tid / 13, f = tid - 13 * p;                               // lanes 0..90: point p, footprint pixel f
  int px = 0, py = 0;
  bool alive = false;
  if (tid < 91 && own_ok[p]) {
    const int dy = f < 5 ? 0 : (f < 8 ? -1 : (f < 11 ? 1 : (f == 11 ? -2 : 2)));
    const int dx = f < 5 ? f - 2 : (f < 8 ? f - 6 : (f < 11 ? f - 9 : 0));
    px = own_x[p] + dx; py = own_y[p] + dy;
    alive = px >= 0 && px < W && py >= 0 && py < H;                       // clipped to the image, not to the window
    for (int q = p + 1; q < 7; ++q) alive = alive && !(own_ok[q] && covers(own_x[q], own_y[q], px, py));
  }
  const int end = run_end;
  for (int base = m + 1; base < end; base += kChunk) {
    if (tid < 7 * kChunk) {
      const int j = base + tid / 7;
      int cx = 0, cy = 0;
      const bool ok = j < end && cone_ok(A, j, img) && point_center(A, j, tid % 7, cx, cy);
      lx[tid] = cx; ly[tid] = cy; lok[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    if (alive)
      for (int q = 0; q < 7 * kChunk; ++q) alive = alive && !(lok[q] && covers(lx[q], ly[q], px, py));
    __syncthreads();
  }
  if (alive) {
    unsigned char* o = A.pool + d[DD_OFF] + ((size_t)py * W + px) * 3;
    o[0] = A.ink[3 * p]; o[1] = A.ink[3 * p + 1]; o[2] = A.ink[3 * p + 2];
  }
}

// ------------------------------------------------------------------------------------------------------------------------- kernel c
__global__ __launch_bounds__(256) void heatmap_mosaic_kernel(const float* __restrict__ hm, int S, unsigned char* __restrict__ out) {
  __shared__ float lo[256], hi[256];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const size_t n = (size_t)S * S, at = ((size_t)blockIdx.y * 7 + blockIdx.x) * n;
  const float* __restrict__ x = hm + at;
  if (tid == 0) bad = 0;
  float mn = INFINITY, mx = -INFINITY;
  bool nan = false;
  for (size_t i = tid; i < n; i += 256) {
    const float v = x[i];
    nan = nan || v != v;
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  lo[tid] = mn; hi[tid] = mx;
  __syncthreads();
  if (nan) bad = 1;
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { lo[tid] = fminf(lo[tid], lo[tid + s]); hi[tid] = fmaxf(hi[tid], hi[tid + s]); }
    __syncthreads();
  }
  const float cmin = lo[0], span = hi[0] - cmin;
  const bool flat = bad != 0 || span == 0.f;                              // NumPy's min / max of a map with a NaN are NaN: every value NaN -> 0
  for (size_t i = tid; i < n; i += 256) {
    const float v = (x[i] - cmin) / span;
    const double t = rint((double)v * 255.0);                             // ties to even
    out[at + i] = flat || !(t > 0.0) ? 0 : (t > 255.0 ? 255 : (unsigned char)(int)t);
  }
}

}  // namespace

extern "C" {

int mdcv_crop_resize_frames_u8(const long long* desc_host, const long long* desc, int B, const unsigned char* pool, long long pool_bytes,
                               const int* rects, const int* count, int K, int max_per_frame, int S, float* crops, int* owner, int* window,
                               int* total, void* stream) {
  if (B < 1 || K < 1 || max_per_frame < 1 || B > 65535 || K > 65535 || pool_bytes < 1 || pool_bytes > (1ll << 60)) return MDCV_EARG;
  if (S < MDCV_KPTLOAD_MIN_SIZE || S > MDCV_KPTLOAD_MAX_SIZE) return MDCV_EARG;
  if (!desc_host || !desc || !pool || !rects || !count || !crops || !owner || !window || !total) return MDCV_EARG;
  const int per = max_per_frame < K ? max_per_frame : K;
  if ((long long)B * per > kMaxPairs) return MDCV_EARG;
  for (int b = 0; b < B; ++b)
    if (!detect_frame_ok(desc_host + (size_t)b * MDCV_DETECT_DESC, pool_bytes)) return MDCV_EARG;
  const int vec = (S % 4 == 0 && ((uintptr_t)crops & 15) == 0) ? 1 : 0;
  CropArgs a{desc, B, pool, pool_bytes, rects, count, K, per, S, vec, crops, owner, window, total};
  MDCV_LAUNCH(crop_frames_kernel, dim3((unsigned)per, (unsigned)B, 3), dim3(256), (size_t)(32 * S + 16), (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_kpt_draw_points(const long long* desc_host, const long long* desc, int n_images, unsigned char* pool, long long pool_bytes,
                         const float* pts, const int* window, const int* owner, int M, const unsigned char* colours, int* centers,
                         int* skipped, void* stream) {
  if (n_images < 1 || n_images > 65535 || M < 0 || M > kMaxPairs || pool_bytes < 1 || pool_bytes > (1ll << 60)) return MDCV_EARG;
  if (!desc_host || !desc || !pool || !colours || !skipped) return MDCV_EARG;
  if (M > 0 && (!pts || !window || !owner || !centers)) return MDCV_EARG;
  for (int b = 0; b < n_images; ++b)
    if (!detect_frame_ok(desc_host + (size_t)b * MDCV_DETECT_DESC, pool_bytes)) return MDCV_EARG;
  hipError_t e = hipMemsetAsync(skipped, 0, (size_t)n_images * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (M == 0) return MDCV_OK;
  PointArgs a{desc, n_images, pool, pool_bytes, pts, window, owner, M, {}, centers, skipped};
  for (int i = 0; i < 21; ++i) a.ink[i] = colours[i];
  MDCV_LAUNCH(kpt_draw_kernel, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_kpt_heatmap_mosaic(const float* hm, int B, int S, unsigned char* out, void* stream) {
  if (B < 0 || B > 65535 || S < 1 || S > MDCV_KPTLOAD_MAX_SIDE) return MDCV_EARG;
  if (B == 0) return MDCV_OK;
  if (!hm || !out) return MDCV_EARG;
  MDCV_LAUNCH(heatmap_mosaic_kernel, dim3(7, (unsigned)B), dim3(256), 0, (hipStream_t)stream, hm, S, out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
