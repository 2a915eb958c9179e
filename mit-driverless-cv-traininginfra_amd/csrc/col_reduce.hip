// Per-channel reductions for gfx950: partial rows -> fp64 accumulators, the column-owner reduce + finalize of the BatchNorm forward
// statistics and backward sums, the in-place row fold in front of it, and column sums (bias gradients).
#include "strip.h"

namespace {

// ---------------------------------------------------------------- BatchNorm statistics
// partial[rows][nsums][C] (fp32, from the conv epilogue) -> accum[nsums][C] (fp64)
// block = 64 columns x 4 row lanes, each block covers 128 rows: coalesced 256-byte row reads, one atomic per column per block
__global__ __launch_bounds__(256) void partial_reduce_kernel(const float* __restrict__ partial, int rows, int cols, double* __restrict__ accum) {
  __shared__ double red[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int r0 = blockIdx.y * 128;
  double s = 0.0;
  if (c < cols) {
    const int r1 = min(rows, r0 + 128);
    for (int r = r0 + ry; r < r1; r += 4) s += (double)partial[(size_t)r * cols + c];
  }
  red[ry][cx] = s;
  __syncthreads();
  if (ry == 0 && c < cols) atomicAdd(&accum[c], red[0][cx] + red[1][cx] + red[2][cx] + red[3][cx]);
}

// accum[0]=sum, accum[1]=sumsq over `count` samples per channel -> batch mean / biased var -> scale, shift ; running stats
__global__ void bn_finalize_kernel(double* __restrict__ accum, double count, const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ running_mean, float* __restrict__ running_var, float momentum, float eps,
                                   float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ mean_out,
                                   float* __restrict__ invstd_out, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double s = accum[c], q = accum[C + c];
  accum[c] = 0.0; accum[C + c] = 0.0;                 // ready for the next step
  const double mean = s / count;
  double var = q / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma[c], b = beta[c];
  scale[c] = g * invstd;
  shift[c] = b - (float)mean * g * invstd;
  mean_out[c] = (float)mean;
  invstd_out[c] = invstd;
  if (running_mean) {
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// ---------------------------------------------------------------- column-owner reduce + finalize
// One launch instead of (partial-row reduce with fp64 atomics -> finalize): a workgroup OWNS 16 channels, sums their partial rows
// itself (64 row lanes x 16 channels, 64-byte segments per row) and finalizes them.  No atomics, no second dependent launch,
// deterministic.  Used while the partial buffer is small (rows <= COLFIN_MAX_ROWS); the 208^2 / 416^2 layers keep the two-stage path.
constexpr int COLFIN_MAX_ROWS = 4096;
struct ColFinArgs {
  const float* partial; int rows, nsums, C; double count;
  // MODE 0: forward statistics -> scale / shift / running stats
  const float* gamma; const float* beta; float* rm; float* rv; float momentum, eps; float* scale; float* shift; float* mean; float* invstd;
  // MODE 1: backward sums -> dgamma, dbeta, coefficient vectors; BN #1 uses sums (0, 1), BN #2 (fused residual pair) sums (0, 2)
  const float* g1; const float* mean1; const float* is1; float* dg1; float* db1; float* cA1; float* cB1; float* cC1;
  const float* g2; const float* mean2; const float* is2; float* dg2; float* db2; float* cA2; float* cB2; float* cC2;
};

__device__ __forceinline__ void bwd_coeffs(double sg, double sgx, double count, float gamma, float mean, float invstd, float* dg, float* db,
                                           float* cA, float* cB, float* cC, int c) {
  dg[c] = (float)sgx;
  db[c] = (float)sg;
  const double g = gamma, is = invstd, mu = mean;
  const double mg = sg / count, mgx = sgx / count;
  cA[c] = (float)(g * is);
  cB[c] = (float)(-g * is * is * mgx);
  cC[c] = (float)(-g * is * mg + g * is * is * mu * mgx);
}

// backward finalize: accum[0]=sum g, accum[kx]=sum g*xhat  ->  dgamma, dbeta and the per-channel coefficients of
//    dy = cA*g + cB*y + cC   ( = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)) )
__global__ void bn_bwd_finalize_kernel(double* __restrict__ accum, int kx, int zero_after, double count, const float* __restrict__ gamma,
                                       const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ cA, float* __restrict__ cB, float* __restrict__ cC,
                                       int C, int nsums) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double sg = accum[c], sgx = accum[(size_t)kx * C + c];
  if (zero_after) for (int k = 0; k < nsums; ++k) accum[(size_t)k * C + c] = 0.0;
  dgamma[c] = (float)sgx;
  dbeta[c] = (float)sg;
  const double g = gamma[c], is = invstd[c], mu = mean[c];
  const double mg = sg / count, mgx = sgx / count;
  cA[c] = (float)(g * is);
  cB[c] = (float)(-g * is * is * mgx);
  cC[c] = (float)(-g * is * mg + g * is * is * mu * mgx);
}

// More than COLFIN_MAX_ROWS partial rows (RektNet's 80x80 x 256-image tensors: 12 800 rows per layer; YOLOv3's 208^2 / 416^2 layers): fold them
// to COLFIN_FOLD_ROWS rows first, IN PLACE and without atomics: block (column group, j) sums the rows j, j + R, j + 2R, ... of its 16 columns
// and writes row j -- it is the only block that reads the rows it writes.  Fixed order -> deterministic.  (The earlier path, 128-row blocks +
// one fp64 atomic per column per block + a finalize launch, took 37 us per RektNet layer.)
constexpr int COLFIN_FOLD_ROWS = 64;
__global__ __launch_bounds__(1024) void rows_fold_kernel(float* __restrict__ partial, int rows, int cols) {
  __shared__ double red[64][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx, j = blockIdx.y;
  double s = 0.0;
  if (c < cols) {
#pragma unroll 4
    for (int r = j + COLFIN_FOLD_ROWS * ry; r < rows; r += COLFIN_FOLD_ROWS * 64) s += (double)partial[(size_t)r * cols + c];
  }
  red[ry][cx] = s;
  __syncthreads();
  if (ry < 16) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) t += red[ry * 4 + k][cx];
    red[ry * 4][cx] = t;
  }
  __syncthreads();
  if (ry == 0 && c < cols) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k * 4][cx];
    partial[(size_t)j * cols + c] = (float)t;
  }
}

// rows -> at most COLFIN_MAX_ROWS rows (returns the new row count); `partial` is scratch of the caller and is consumed
static int fold_rows(float* partial, int rows, int cols, hipStream_t st) {
  if (rows <= COLFIN_MAX_ROWS) return rows;
  MDCV_LAUNCH(rows_fold_kernel, dim3((unsigned)cdiv(cols, 16), (unsigned)COLFIN_FOLD_ROWS), dim3(1024), 0, st, partial, rows, cols);
  return COLFIN_FOLD_ROWS;
}

template <int MODE>
__global__ __launch_bounds__(1024) void bn_colfinal_kernel(ColFinArgs a) {
  __shared__ double red[3][64][16];
  __shared__ double tot[3][16];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (c < a.C) {
    const size_t stride = (size_t)a.nsums * a.C;
    const float* p = a.partial + c;
    if (a.nsums == 1) {
#pragma unroll 4
      for (int r = ry; r < a.rows; r += 64) s0 += (double)p[r * stride];
    } else if (a.nsums == 2) {
#pragma unroll 4
      for (int r = ry; r < a.rows; r += 64) { s0 += (double)p[r * stride]; s1 += (double)p[r * stride + a.C]; }
    } else {
#pragma unroll 4
      for (int r = ry; r < a.rows; r += 64) { s0 += (double)p[r * stride]; s1 += (double)p[r * stride + a.C]; s2 += (double)p[r * stride + 2 * a.C]; }
    }
  }
  red[0][ry][cx] = s0; red[1][ry][cx] = s1; red[2][ry][cx] = s2;
  __syncthreads();
  if (ry < 3) {
    double t = 0.0;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) t += red[ry][k][cx];
    tot[ry][cx] = t;
  }
  __syncthreads();
  if (ry != 0 || c >= a.C) return;
  if (MODE == 0) {
    const double mean = tot[0][cx] / a.count;
    double var = tot[1][cx] / a.count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
    const float g = a.gamma[c], b = a.beta[c];
    a.scale[c] = g * invstd;
    a.shift[c] = b - (float)mean * g * invstd;
    a.mean[c] = (float)mean;
    a.invstd[c] = invstd;
    if (a.rm) {
      const double unbiased = a.count > 1.0 ? var * a.count / (a.count - 1.0) : var;
      a.rm[c] = (1.f - a.momentum) * a.rm[c] + a.momentum * (float)mean;
      a.rv[c] = (1.f - a.momentum) * a.rv[c] + a.momentum * (float)unbiased;
    }
  } else if (MODE == 2) {
    a.scale[c] = (float)tot[0][cx];            // plain column sum (bias gradient)
  } else if (MODE == 3) {                      // sums from the fused data gradient: second sum is sum g*(y - mean), not yet / std
    bwd_coeffs(tot[0][cx], tot[1][cx] * (double)a.is1[c], a.count, a.g1[c], a.mean1[c], a.is1[c], a.dg1, a.db1, a.cA1, a.cB1, a.cC1, c);
  } else {
    bwd_coeffs(tot[0][cx], tot[1][cx], a.count, a.g1[c], a.mean1[c], a.is1[c], a.dg1, a.db1, a.cA1, a.cB1, a.cC1, c);
    if (a.nsums == 3) bwd_coeffs(tot[0][cx], tot[2][cx], a.count, a.g2[c], a.mean2[c], a.is2[c], a.dg2, a.db2, a.cA2, a.cB2, a.cC2, c);
  }
}

// ---------------------------------------------------------------- per-channel column sum (bias gradients of BN-less convs)
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int ldc, int M, int C, double* __restrict__ accum, int PB, int CV, int PPI) {
  constexpr int VEC = ET<T>::VEC;
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x;
  const bool active = tid < PPI * CV;
  const int cv = active ? tid % CV : 0, pi = active ? tid / CV : 0;
  float s[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] = 0.f;
  const long long p0 = (long long)blockIdx.x * PB, p1 = min((long long)M, p0 + PB);
  if (active)
    for (long long p = p0 + pi; p < p1; p += PPI) {
      float v[VEC];
      ET<T>::unpack(*reinterpret_cast<const uint4*>(x + p * ldc + cv * VEC), v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] += v[e];
    }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[tid * 8 + e] = s[e];
  __syncthreads();
  if (active && pi == 0) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float t = 0.f;
      for (int q = 0; q < PPI; ++q) t += red[(q * CV + cv) * 8 + e];
      atomicAdd(&accum[cv * VEC + e], (double)t);
    }
  }
}
// same strip walk, but every block stores its [C] partial row (no atomics); bn_colfinal_kernel<2> sums the rows
template <typename T>
__global__ __launch_bounds__(256) void colsum_rows_kernel(const T* __restrict__ x, int ldc, int M, int C, float* __restrict__ partial, int PB, int CV, int PPI) {
  constexpr int VEC = ET<T>::VEC;
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x;
  const bool active = tid < PPI * CV;
  const int cv = active ? tid % CV : 0, pi = active ? tid / CV : 0;
  float s[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] = 0.f;
  const long long p0 = (long long)blockIdx.x * PB, p1 = min((long long)M, p0 + PB);
  if (active)
    for (long long p = p0 + pi; p < p1; p += PPI) {
      float v[VEC];
      ET<T>::unpack(*reinterpret_cast<const uint4*>(x + p * ldc + cv * VEC), v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) s[e] += v[e];
    }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[tid * 8 + e] = s[e];
  __syncthreads();
  if (active && pi == 0) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float t = 0.f;
      for (int q = 0; q < PPI; ++q) t += red[(q * CV + cv) * 8 + e];
      partial[(size_t)blockIdx.x * C + cv * VEC + e] = t;
    }
  }
}
__global__ void accum_to_f32_kernel(double* __restrict__ accum, float* __restrict__ out, int n, int zero_after) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (float)accum[i];
  if (zero_after) accum[i] = 0.0;
}

}  // namespace

int launch_partial_reduce(const float* partial, int rows, int cols, double* accum, hipStream_t st) {
  MDCV_LAUNCH(partial_reduce_kernel, dim3((unsigned)cdiv(cols, 64), (unsigned)cdiv(rows, 128)), dim3(256), 0, st, partial, rows, cols, accum);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int launch_bn_colfinal_bwd(const float* partial, int rows, int nsums, int C, double count, const BnBwdCoefs& bn1, const BnBwdCoefs& bn2,
                           hipStream_t st) {
  ColFinArgs f = {};
  f.partial = partial; f.rows = rows; f.nsums = nsums; f.C = C; f.count = count;
  f.g1 = bn1.gamma; f.mean1 = bn1.mean; f.is1 = bn1.invstd; f.dg1 = bn1.dgamma; f.db1 = bn1.dbeta; f.cA1 = bn1.cA; f.cB1 = bn1.cB; f.cC1 = bn1.cC;
  f.g2 = bn2.gamma; f.mean2 = bn2.mean; f.is2 = bn2.invstd; f.dg2 = bn2.dgamma; f.db2 = bn2.dbeta; f.cA2 = bn2.cA; f.cB2 = bn2.cB; f.cC2 = bn2.cC;
  MDCV_LAUNCH(bn_colfinal_kernel<1>, dim3((unsigned)cdiv(C, 16)), dim3(1024), 0, st, f);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

extern "C" {

int mdcv_partial_reduce(const float* partial, int rows, int nsums, int C, double* accum, void* stream) {
  if (!partial || !accum || rows < 1) return MDCV_EARG;
  return launch_partial_reduce(partial, rows, nsums * C, accum, (hipStream_t)stream);
}

int mdcv_bn_finalize(double* accum, double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps, float* scale, float* shift, float* mean, float* invstd, int C, void* stream) {
  if (!accum || !gamma || !beta || !scale || !shift || !mean || !invstd) return MDCV_EARG;
  MDCV_LAUNCH(bn_finalize_kernel, dim3((unsigned)cdiv(C, 128)), dim3(128), 0, (hipStream_t)stream, accum, count, gamma, beta,
                     running_mean, running_var, momentum, eps, scale, shift, mean, invstd, C);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

// conv-epilogue partial rows -> batch statistics -> scale / shift (+ running stats): one launch while the partial buffer is small
int mdcv_bn_stats_finalize(float* partial, int rows, double* accum, double count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift, float* mean,
                           float* invstd, int C, void* stream) {
  if (!partial || !accum || rows < 1 || !gamma || !beta || !scale || !shift || !mean || !invstd) return MDCV_EARG;
  rows = fold_rows(partial, rows, 2 * C, (hipStream_t)stream);      // (large buffers: folded in place first)
  MDCV_CHECK_LAUNCH();
  ColFinArgs a = {};
  a.partial = partial; a.rows = rows; a.nsums = 2; a.C = C; a.count = count; a.gamma = gamma; a.beta = beta; a.rm = running_mean;
  a.rv = running_var; a.momentum = momentum; a.eps = eps; a.scale = scale; a.shift = shift; a.mean = mean; a.invstd = invstd;
  MDCV_LAUNCH(bn_colfinal_kernel<0>, dim3((unsigned)cdiv(C, 16)), dim3(1024), 0, (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_bn_bwd_finalize(double* accum, int kx, int nsums, int zero_after, double count, const float* gamma, const float* mean,
                         const float* invstd, float* dgamma, float* dbeta, float* cA, float* cB, float* cC, int C, void* stream) {
  if (!accum || !gamma || !dgamma || !dbeta || !cA || !cB || !cC) return MDCV_EARG;
  MDCV_LAUNCH(bn_bwd_finalize_kernel, dim3((unsigned)cdiv(C, 128)), dim3(128), 0, (hipStream_t)stream, accum, kx, zero_after, count,
                     gamma, mean, invstd, dgamma, dbeta, cA, cB, cC, C, nsums);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_bn_bwd_finalize_rows(float* partial, int rows, int C, double count, const float* gamma, const float* mean,
                              const float* invstd, float* dgamma, float* dbeta, float* cA, float* cB, float* cC, void* stream) {
  if (!partial || rows < 1 || !gamma || !mean || !invstd || !dgamma || !dbeta || !cA || !cB || !cC) return MDCV_EARG;
  rows = fold_rows(partial, rows, 2 * C, (hipStream_t)stream);
  MDCV_CHECK_LAUNCH();
  ColFinArgs f = {};
  f.partial = partial; f.rows = rows; f.nsums = 2; f.C = C; f.count = count;
  f.g1 = gamma; f.mean1 = mean; f.is1 = invstd; f.dg1 = dgamma; f.db1 = dbeta; f.cA1 = cA; f.cB1 = cB; f.cC1 = cC;
  MDCV_LAUNCH(bn_colfinal_kernel<3>, dim3((unsigned)cdiv(C, 16)), dim3(1024), 0, (hipStream_t)stream, f);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_colsum(int dtype, const void* x, int ldc, int M, int C, double* accum, void* stream) {
  if (!x || !accum || (C & 7)) return MDCV_EARG;
  return launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const Strip s = make_strip<T>(M, C, kReduceBlocks);
    if (s.CV > 256) return MDCV_EARG;
    MDCV_LAUNCH(colsum_kernel<T>, dim3((unsigned)cdiv(M, s.PB)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldc, M, C, accum, s.PB, s.CV, s.PPI);
    return MDCV_OK;
  });
}

// column sums without atomics: per-block partial rows (partial_ws: mdcv_colsum_ws_floats floats) + one column-owner launch
int mdcv_colsum_ws_floats(int dtype, int M, int C) {
  const Strip s = dtype == MDCV_BF16 ? make_strip<bf16_t>(M, C, kReduceBlocks) : make_strip<float>(M, C, kReduceBlocks);
  return cdiv(M, s.PB) * C;
}
int mdcv_colsum_f32(int dtype, const void* x, int ldc, int M, int C, float* partial_ws, float* out, void* stream) {
  if (!x || !partial_ws || !out || (C & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  int rows = 0;
  const int rc = launch_by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    const Strip s = make_strip<T>(M, C, kReduceBlocks);
    if (s.CV > 256) return MDCV_EARG;
    rows = cdiv(M, s.PB);
    MDCV_LAUNCH(colsum_rows_kernel<T>, dim3((unsigned)rows), dim3(256), 0, st, (const T*)x, ldc, M, C, partial_ws, s.PB, s.CV, s.PPI);
    return MDCV_OK;
  });
  if (rc != MDCV_OK) return rc;
  ColFinArgs f = {};
  f.partial = partial_ws; f.rows = rows; f.nsums = 1; f.C = C; f.count = 1.0; f.scale = out;
  MDCV_LAUNCH(bn_colfinal_kernel<2>, dim3((unsigned)cdiv(C, 16)), dim3(1024), 0, st, f);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_accum_to_f32(double* accum, float* out, int n, int zero_after, void* stream) {
  MDCV_LAUNCH(accum_to_f32_kernel, dim3((unsigned)cdiv(n, 128)), dim3(128), 0, (hipStream_t)stream, accum, out, n, zero_after);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
