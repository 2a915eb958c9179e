// Weight EMA for gfx950 (wave = 64 lanes): an exponential moving average of the flat fp32 parameter buffer and of the BatchNorm running
// statistics in one shadow buffer, driven from a control block in device memory -- so a training step averages, or leaves the average
// alone when the gradient guard dropped the step, without a host read.  Contract: include/mdcv_hip.h; arithmetic and ordering: DESIGN §27.
//
//   mdcv_ema_advance           one thread: the guard's decision, the decay of this update (fp64 rule, rounded once), the update count
//   mdcv_ema_update            e = e + omd * (p - e) over a contiguous 16-byte aligned range; apply == 0: returns before touching memory
//   mdcv_ema_update_segments   the same over a device table of (source, shadow offset, length) rows: one launch for every BatchNorm statistic
//   mdcv_ema_swap(_segments)   exchange live and shadow words in place; twice = identity
//
// The file is built with -ffp-contract=off: the subtraction, the product and the sum each round on their own, and tests/weight_ema_ref.py
// restates them in NumPy and is compared as bits.  The range kernels are HBM-bound (12 bytes per element: p and e read, e written; the swap
// 16): float4 per lane, two independent float4 per lane in flight, a grid capped at MDCV_EMA_MAX_GRID workgroups that strides over the rest.
#include "../../include/mdcv_hip.h"
#include "common.h"

namespace {

constexpr int THREADS = MDCV_EMA_THREADS;

__device__ __forceinline__ float ema1(float e, float p, float omd) {
  const float diff = p - e;
  const float step = omd * diff;
  return e + step;
}

__device__ __forceinline__ float4 ema4(float4 e, uint4 pu, float omd) {
  e.x = ema1(e.x, __uint_as_float(pu.x), omd);
  e.y = ema1(e.y, __uint_as_float(pu.y), omd);
  e.z = ema1(e.z, __uint_as_float(pu.z), omd);
  e.w = ema1(e.w, __uint_as_float(pu.w), omd);
  return e;
}

__global__ void ema_advance_kernel(mdcv_ema_block* __restrict__ blk, const mdcv_grad_guard_block* __restrict__ guard, float decay, long long warmup) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int apply = guard ? guard->apply : 1;
  if (!apply) {                                          // the optimizer dropped this step: the update count and the decay stay
    blk->apply = 0;
    return;
  }
  const long long t = blk->updates;
  const double ramp = (1.0 + (double)t) / ((double)warmup + (double)t);
  const double d64 = fmin((double)decay, ramp);
  const float d = (float)d64;
  blk->d = d;
  blk->omd = 1.0f - d;
  blk->apply = 1;
  blk->updates = t + 1;
}

// p is loaded non-temporally: behind the optimizer update (and, in the pipelined step, behind the re-pack of the group) this pass is the
// last reader of the parameters until the next step rewrites them.  e is read and written with the default policy.
__global__ __launch_bounds__(THREADS) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, long long n,
                                                             const mdcv_ema_block* __restrict__ blk) {
  if (blk->apply == 0) return;
  const float omd = blk->omd;
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * THREADS;
  float4* e4 = reinterpret_cast<float4*>(e);
  const float4* p4 = reinterpret_cast<const float4*>(p);
  long long i = blockIdx.x * (long long)THREADS + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {             // two float4 of each side in flight per lane
    const uint4 pa = mdcv_ld_stream(p4 + i), pb = mdcv_ld_stream(p4 + i + stride);
    const float4 ea = e4[i], eb = e4[i + stride];
    e4[i] = ema4(ea, pa, omd);
    e4[i + stride] = ema4(eb, pb, omd);
  }
  if (i < n4) e4[i] = ema4(e4[i], mdcv_ld_stream(p4 + i), omd);
  const long long tail = (n4 << 2) + threadIdx.x;        // n & 3 elements behind the last float4
  if (blockIdx.x == 0 && tail < n) e[tail] = ema1(e[tail], p[tail], omd);
}

__global__ __launch_bounds__(THREADS) void ema_swap_kernel(unsigned* __restrict__ e, unsigned* __restrict__ p, long long n) {
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * THREADS;
  uint4* e4 = reinterpret_cast<uint4*>(e);
  uint4* p4 = reinterpret_cast<uint4*>(p);
  for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < n4; i += stride) {
    const uint4 a = e4[i], b = p4[i];
    e4[i] = b;
    p4[i] = a;
  }
  const long long tail = (n4 << 2) + threadIdx.x;
  if (blockIdx.x == 0 && tail < n) {
    const unsigned a = e[tail], b = p[tail];
    e[tail] = b;
    p[tail] = a;
  }
}

// a row the shadow buffer cannot hold is skipped by every thread alike (the table is the caller's, on the device: it is checked here)
__device__ __forceinline__ bool row_ok(const mdcv_ema_segment& r, long long ema_elems) {
  return r.src != nullptr && r.offset >= 0 && r.length >= 0 && r.offset <= ema_elems && r.length <= ema_elems - r.offset;
}

// Workgroup b takes rows b, b + gridDim.x, ..; its threads stride over the row.  Scalar accesses: the sources are wherever torch put
// them (4-byte aligned), the rows are 1 .. 1024 elements, and all 144 of YOLOv3 together are 110 KB.
__global__ __launch_bounds__(THREADS) void ema_update_segments_kernel(float* __restrict__ e, long long ema_elems, const mdcv_ema_segment* __restrict__ table,
                                                                      int n_segments, const mdcv_ema_block* __restrict__ blk) {
  if (blk->apply == 0) return;
  const float omd = blk->omd;
  for (int r = blockIdx.x; r < n_segments; r += gridDim.x) {
    const mdcv_ema_segment row = table[r];
    if (!row_ok(row, ema_elems)) continue;
    float* dst = e + row.offset;
    for (long long i = threadIdx.x; i < row.length; i += THREADS) dst[i] = ema1(dst[i], row.src[i], omd);
  }
}

__global__ __launch_bounds__(THREADS) void ema_swap_segments_kernel(unsigned* __restrict__ e, long long ema_elems, const mdcv_ema_segment* __restrict__ table,
                                                                    int n_segments) {
  for (int r = blockIdx.x; r < n_segments; r += gridDim.x) {
    const mdcv_ema_segment row = table[r];
    if (!row_ok(row, ema_elems)) continue;
    unsigned* dst = e + row.offset;
    unsigned* src = reinterpret_cast<unsigned*>(const_cast<float*>(row.src));
    for (long long i = threadIdx.x; i < row.length; i += THREADS) {
      const unsigned a = dst[i], b = src[i];
      dst[i] = b;
      src[i] = a;
    }
  }
}

inline unsigned range_grid(long long n) {
  long long g = (n / 4 + THREADS - 1) / THREADS;
  if (g > MDCV_EMA_MAX_GRID) g = MDCV_EMA_MAX_GRID;
  if (g < 1) g = 1;
  return (unsigned)g;
}

inline unsigned segment_grid(int n_segments) { return (unsigned)(n_segments < 1024 ? n_segments : 1024); }

}  // namespace

extern "C" {

int mdcv_ema_advance(mdcv_ema_block* block, const mdcv_grad_guard_block* guard, float decay, long long warmup, void* stream) {
  if (!block || ((uintptr_t)block & 7) || ((uintptr_t)guard & 7) || !(decay >= 0.f && decay < 1.f) || warmup < 1) return MDCV_EARG;
  MDCV_LAUNCH(ema_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, block, guard, decay, warmup);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_ema_update(float* ema, const float* params, long long n, const mdcv_ema_block* block, void* stream) {
  if (!ema || !params || !block || n < 0 || (((uintptr_t)ema | (uintptr_t)params) & 15) || ((uintptr_t)block & 7)) return MDCV_EARG;
  if (n == 0) return MDCV_OK;
  MDCV_LAUNCH(ema_update_kernel, dim3(range_grid(n)), dim3(THREADS), 0, (hipStream_t)stream, ema, params, n, block);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_ema_update_segments(float* ema, long long ema_elems, const mdcv_ema_segment* table, int n_segments, const mdcv_ema_block* block,
                             void* stream) {
  if (!ema || ema_elems < 0 || n_segments < 0 || (n_segments > 0 && !table) || !block) return MDCV_EARG;
  if (((uintptr_t)ema & 3) || ((uintptr_t)table & 7) || ((uintptr_t)block & 7)) return MDCV_EARG;
  if (n_segments == 0) return MDCV_OK;
  MDCV_LAUNCH(ema_update_segments_kernel, dim3(segment_grid(n_segments)), dim3(THREADS), 0, (hipStream_t)stream, ema, ema_elems, table, n_segments,
              block);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_ema_swap(float* ema, float* params, long long n, void* stream) {
  if (!ema || !params || n < 0 || (((uintptr_t)ema | (uintptr_t)params) & 15)) return MDCV_EARG;
  if (n == 0) return MDCV_OK;
  // overlapping sides would not be an exchange
  const uintptr_t a = (uintptr_t)ema, b = (uintptr_t)params, bytes = (uintptr_t)n * 4;
  if (a < b + bytes && b < a + bytes) return MDCV_EARG;
  MDCV_LAUNCH(ema_swap_kernel, dim3(range_grid(n)), dim3(THREADS), 0, (hipStream_t)stream, reinterpret_cast<unsigned*>(ema),
              reinterpret_cast<unsigned*>(params), n);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_ema_swap_segments(float* ema, long long ema_elems, const mdcv_ema_segment* table, int n_segments, void* stream) {
  if (!ema || ema_elems < 0 || n_segments < 0 || (n_segments > 0 && !table)) return MDCV_EARG;
  if (((uintptr_t)ema & 3) || ((uintptr_t)table & 7)) return MDCV_EARG;
  if (n_segments == 0) return MDCV_OK;
  MDCV_LAUNCH(ema_swap_segments_kernel, dim3(segment_grid(n_segments)), dim3(THREADS), 0, (hipStream_t)stream, reinterpret_cast<unsigned*>(ema),
              ema_elems, table, n_segments);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
