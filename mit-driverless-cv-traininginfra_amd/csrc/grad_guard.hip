// Gradient guard for gfx950 (wave = 64 lanes): the global norm of the flat fp32 gradient buffer, the clip coefficient, the decision to
// drop a step with a non-finite gradient, and optimizer updates that take all of it from a control block in device memory -- so a
// training step is measured, clipped or skipped without a host read.  Contract: include/mdcv_hip.h; arithmetic and ordering: DESIGN §26.
//
//   mdcv_grad_sumsq            one pass over g: one fp64 partial per chunk of MDCV_GRAD_GUARD_CHUNK consecutive elements
//   mdcv_grad_guard_finalize   one workgroup: partials -> sumsq, norm, coef, scale, apply, counters, bias corrections, history ring
//   mdcv_adam_step_guarded /   adam_kernel / sgd_kernel of optim.hip element for element, hyper-parameters of the step from the block;
//   mdcv_sgd_step_guarded      apply == 0: every thread returns before it touches p, g or the state
//
// Every sum below has an order that is a function of n alone (no atomics, no dependence on the grid or on which workgroup runs when), and
// the file is built with -ffp-contract=off: tests/gradguard_ref.py restates each operation in NumPy and is compared as bits.
#include "../../include/mdcv_hip.h"
#include "common.h"

namespace {

constexpr int CHUNK = MDCV_GRAD_GUARD_CHUNK;          // 4096 elements = 1024 float4 = 4 rounds of 256 threads
constexpr int ROUNDS = CHUNK / 4 / 256;
static_assert(ROUNDS * 256 * 4 == CHUNK, "a chunk is a whole number of 256-thread float4 rounds");

// 256 values -> one, the same way everywhere in this file: the xor butterfly inside each wave (offsets 32, 16, .. 1; after it every lane of
// a wave holds the wave's sum), lane 0 of each wave to red[wave], then ((red[0] + red[1]) + red[2]) + red[3] by thread 0.  The caller
// alternates `red` between two slots from one use to the next, so a single barrier per use is enough: a slot is written again only
// behind the barrier of the use in between, which thread 0 reaches after it has read the slot.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];        // (only thread 0's value is used)
}

// Thread t of the workgroup that owns chunk c adds, in this order, the squares of elements c*4096 + (r*256 + t)*4 + e for r = 0..3,
// e = 0..3, each formed in double (exact: 48 significant bits at most; no overflow: |x| < 2^128).  Elements at or beyond n add +0.0.
// Plain loads: the update that follows reads the same gradient again, so the lines should stay in L2 / MALL.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n, long long n_chunks, double* __restrict__ partials) {
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  int slot = 0;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x, slot ^= 1) {
    const long long base = c * CHUNK + (long long)tid * 4;
    float4 x[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const long long i = base + (long long)r * 1024;
      if (i + 4 <= n) {
        x[r] = *reinterpret_cast<const float4*>(g + i);
      } else {                                         // the scalar tail of the last chunk (n is no multiple of 4) and what lies beyond n
        x[r].x = i < n ? g[i] : 0.f;
        x[r].y = i + 1 < n ? g[i + 1] : 0.f;
        x[r].z = i + 2 < n ? g[i + 2] : 0.f;
        x[r].w = 0.f;
      }
    }
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const double a = (double)x[r].x, b = (double)x[r].y, cc = (double)x[r].z, d = (double)x[r].w;
      acc += a * a; acc += b * b; acc += cc * cc; acc += d * d;
    }
    const double s = block_sum_256(acc, red[slot]);
    if (tid == 0) partials[c] = s;
  }
}

// beta^t by square-and-multiply from the low bit up: r and x start at 1 and beta; for each bit of t, low to high: r = r * x if the bit is
// set, then x = x * x while higher bits remain.  Each product rounds once (IEEE double); the host restates it operation for operation.
__device__ double pow_d(double beta, long long t) {
  double r = 1.0, x = beta;
  while (t > 0) {
    if (t & 1) r = r * x;
    t >>= 1;
    if (t > 0) x = x * x;
  }
  return r;
}

// ONE workgroup.  Thread t adds partials t, t + 256, .. in that order; block_sum_256 joins the 256 sums; thread 0 writes the block.
__global__ __launch_bounds__(256) void grad_guard_finalize_kernel(const double* __restrict__ partials, long long n_partials, float grad_scale,
                                                                  float max_norm, int skip_nonfinite, double beta1, double beta2,
                                                                  mdcv_grad_guard_block* __restrict__ blk, float* __restrict__ history, int ring) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
  const double sumsq = block_sum_256(acc, red);
  if (threadIdx.x != 0) return;
  const int finite = isfinite(sumsq) ? 1 : 0;           // every square is finite iff its gradient is; a finite sum of them cannot overflow
  const float norm = (float)(fabs((double)grad_scale) * sqrt(sumsq));
  const float coef = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;     // torch.nn.utils.clip_grad_norm_
  const int apply = (finite || !skip_nonfinite) ? 1 : 0;
  const long long attempted = blk->attempted, applied = blk->applied;
  const long long t = applied + 1;                       // the step about to be applied: a skipped one never happened
  blk->sumsq = sumsq;
  blk->norm = norm;
  blk->coef = coef;
  blk->scale = grad_scale * coef;
  blk->bc1 = (float)(1.0 - pow_d(beta1, t));
  blk->bc2_sqrt = (float)sqrt(1.0 - pow_d(beta2, t));
  if (finite && norm > blk->max_norm_seen) blk->max_norm_seen = norm;
  blk->finite = finite;
  blk->apply = apply;
  blk->attempted = attempted + 1;
  if (apply) blk->applied = applied + 1; else blk->skipped += 1;
  if (apply && finite && coef < 1.f) blk->clipped += 1;
  if (history && ring > 0) history[attempted % ring] = norm;
}

// adam_kernel of optim.hip: the same expressions in the same order.  grad_scale, bc1 and bc2_sqrt come from the block; blk->apply == 0
// (uniform over the grid) returns before anything else is read.
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                           long long n, const mdcv_grad_guard_block* __restrict__ blk, float lr, float beta1,
                                                           float beta2, float eps, float weight_decay) {
  if (blk->apply == 0) return;
  const float grad_scale = blk->scale, bc1 = blk->bc1, bc2_sqrt = blk->bc2_sqrt;
  const long long n4 = n >> 2;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* P = &pp.x; const float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = G[e] * grad_scale + weight_decay * P[e];
      M[e] = beta1 * M[e] + (1.f - beta1) * gr;
      V[e] = beta2 * V[e] + (1.f - beta2) * gr * gr;
      P[e] -= (lr / bc1) * M[e] / (sqrtf(V[e]) / bc2_sqrt + eps);
    }
    reinterpret_cast<float4*>(p)[i] = pp; reinterpret_cast<float4*>(m)[i] = mm; reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float gr = g[i] * grad_scale + weight_decay * p[i];
    m[i] = beta1 * m[i] + (1.f - beta1) * gr;
    v[i] = beta2 * v[i] + (1.f - beta2) * gr * gr;
    p[i] -= (lr / bc1) * m[i] / (sqrtf(v[i]) / bc2_sqrt + eps);
  }
}

// sgd_kernel of optim.hip.  "First step" = no step was applied before this one; the finalize in front has already counted this one, so
// that reads applied == 1.
__global__ __launch_bounds__(256) void sgd_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n,
                                                          const mdcv_grad_guard_block* __restrict__ blk, float lr, float momentum, float weight_decay) {
  if (blk->apply == 0) return;
  const float grad_scale = blk->scale;
  const int first_step = blk->applied == 1 ? 1 : 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float gr = g[i] * grad_scale + weight_decay * p[i];
    if (momentum != 0.f) {
      const float b = first_step ? gr : momentum * buf[i] + gr;
      buf[i] = b;
      gr = b;
    }
    p[i] -= lr * gr;
  }
}

}  // namespace

extern "C" {

int mdcv_grad_sumsq(const float* grads, long long n, double* partials, void* stream) {
  if (!grads || !partials || n < 1 || ((uintptr_t)grads & 15) || ((uintptr_t)partials & 7)) return MDCV_EARG;
  const long long n_chunks = (n + CHUNK - 1) / CHUNK;
  const long long g = n_chunks < MDCV_GRAD_GUARD_MAX_GRID ? n_chunks : MDCV_GRAD_GUARD_MAX_GRID;
  MDCV_LAUNCH(grad_sumsq_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, grads, n, n_chunks, partials);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_grad_guard_finalize(const double* partials, long long n_partials, float grad_scale, float max_norm, int skip_nonfinite, double beta1,
                             double beta2, mdcv_grad_guard_block* block, float* history, int ring, void* stream) {
  if (!partials || !block || n_partials < 1 || ((uintptr_t)partials & 7) || ((uintptr_t)block & 7) || ring < 0 || (ring > 0 && !history)) return MDCV_EARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return MDCV_EARG;
  MDCV_LAUNCH(grad_guard_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, grad_scale, max_norm, skip_nonfinite,
              beta1, beta2, block, history, ring);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, const mdcv_grad_guard_block* block,
                           float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !block || n < 0) return MDCV_EARG;
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return MDCV_EARG;
  if ((uintptr_t)block & 7) return MDCV_EARG;
  long long g = (n / 4 + 255) / 256; if (g > 4096) g = 4096; if (g < 1) g = 1;
  MDCV_LAUNCH(adam_guarded_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, block, lr, beta1,
              beta2, eps, weight_decay);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_sgd_step_guarded(float* params, const float* grads, float* momentum_buf, long long n, const mdcv_grad_guard_block* block, float lr,
                          float momentum, float weight_decay, void* stream) {
  if (!params || !grads || (momentum != 0.f && !momentum_buf) || !block || n < 0 || ((uintptr_t)block & 7)) return MDCV_EARG;
  long long g = (n + 255) / 256; if (g > 8192) g = 8192; if (g < 1) g = 1;
  MDCV_LAUNCH(sgd_guarded_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, n, block, lr, momentum,
              weight_decay);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
