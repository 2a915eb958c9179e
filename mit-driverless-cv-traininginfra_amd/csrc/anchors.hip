// Batched Lloyd iterations for the anchor k-means of dataset preparation (gfx950, wave64): N boxes (h, w) in fp64, K clusters, R
// independent restarts, every result reproducible bit for bit by NumPy + math.fsum (tests/helpers/anchor_refs.py).
//
//   assignment / update   <- CVC-YOLOv3/generate_kmeans_dataset_csvs.py:16-28, the loop of main at 139-149
//
// Arithmetic (contract: include/mdcv_hip.h).  Assignment: for k in index order q = fl(fl(dh*dh) + fl(dw*dw)), d = sqrt(q) correctly rounded,
// the first minimum wins, a NaN centroid never wins.  Update: c[k] = fl(S_k / n_k) with S_k the EXACT sum of the members rounded once to
// nearest-even.  The sums are exact because they are integers: a coordinate x (finite, |x| < 2^14, a multiple of 2^-64) is the integer
// X = x * 2^64, |X| < 2^78, split into three 32-bit digits that are added, with the sign, to three signed 64-bit words -- 2^24 boxes of digits
// below 2^32 stay below 2^56 -- first in LDS per workgroup, then with agent-scope integer atomics into the restart's global words.  Integer
// addition is associative: the totals do not depend on the order in which lanes or workgroups land.  The words are folded into one signed
// 128-bit integer and converted to fp64 by hand with round-to-nearest-even (kmeans_words_to_double).
//
// One launch per iteration.  Step t's prologue computes the centroids from the words step t-1 left (step 0: from the initial centroids), so
// the update needs neither a launch of its own nor a ticket with a fence: the kernel boundary that the next assignment needs anyway is the
// hand-off.  Every workgroup repeats the 2K conversions of its restart (a few hundred integer instructions).  The words rotate over three
// sets: step t reads set (t-1)%3, adds to set t%3 and clears set (t+1)%3, which step t-1 read last.
//
// Because the sums are exact, an unchanged assignment reproduces the same centroids: steps after a restart's fixed point are no-ops and the
// host may enqueue them blindly in chunks.  Per restart the device records converged_at, the first step whose assignment equals the previous
// one; mdcv_kmeans_steps ends a chunk with one small launch that writes the record the host reads.
#include <stdint.h>

#include "../../include/mdcv_hip.h"
#include "common.h"

namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_WORDS = 7;                    // per cluster: h digits 0..2, w digits 0..2, member count
constexpr int KM_TAIL = 3;                     // per restart behind the clusters: changed assignments, distortion low / high
constexpr int KM_MAXK = MDCV_KMEANS_MAX_K;
constexpr int KM_MAXR = MDCV_KMEANS_MAX_R;

__host__ __device__ inline size_t km_set_words(int K) { return (size_t)K * KM_WORDS + KM_TAIL; }

// workspace: [cent0: R*K*2 doubles][acc: 3 sets * R * (K*7 + 3) int64][conv: R int64]
struct KmWs {
  double* cent0;
  long long* acc;
  long long* conv;
};
__host__ __device__ inline KmWs km_ws(void* ws, int K, int R) {
  KmWs w;
  w.cent0 = reinterpret_cast<double*>(ws);
  w.acc = reinterpret_cast<long long*>(w.cent0 + (size_t)R * K * 2);
  w.conv = w.acc + 3 * (size_t)R * km_set_words(K);
  return w;
}
__host__ __device__ inline long long* km_set(const KmWs& w, int K, int R, int set, int r) {
  return w.acc + ((size_t)set * R + r) * km_set_words(K);
}

// x = X * 2^-64 exactly (the caller guarantees finite, |x| < 2^14, a multiple of 2^-64): the three 32-bit digits of |X| with x's sign
__device__ __forceinline__ void kmeans_digits(double x, long long d[3]) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const int e = (int)((u >> 52) & 0x7ff);
  unsigned long long m = u & 0xfffffffffffffULL;
  d[0] = d[1] = d[2] = 0;
  if (e == 0) return;                               // zero (a subnormal is no multiple of 2^-64)
  m |= 1ULL << 52;
  const int s = e - 1075 + 64;                      // X = m * 2^s, s <= 13 - 52 + 64 = 25
  unsigned long long lo, hi;
  if (s >= 0) {
    const int sh = s > 25 ? 25 : s;                 // (out of contract: stays in bounds)
    lo = m << sh;
    hi = sh ? m >> (64 - sh) : 0;
  } else {
    lo = s > -64 ? m >> (-s) : 0;                   // exact: the low bits are zero by contract
    hi = 0;
  }
  d[0] = (long long)(lo & 0xffffffffULL);
  d[1] = (long long)(lo >> 32);
  d[2] = (long long)hi;
  if (u >> 63) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; }
}

// (d0 + d1 * 2^32 + d2 * 2^64) * 2^-64 -> fp64, round-to-nearest-even, by hand on two 64-bit halves
__device__ __forceinline__ double kmeans_words_to_double(long long d0, long long d1, long long d2) {
  unsigned long long lo = (unsigned long long)d0;
  long long hi = d0 < 0 ? -1 : 0;
  const unsigned long long a = (unsigned long long)d1 << 32;
  const unsigned long long lo1 = lo + a;
  hi += (d1 >> 32) + (lo1 < lo ? 1 : 0);
  lo = lo1;
  hi += d2;
  const bool neg = hi < 0;
  unsigned long long mh = (unsigned long long)hi, ml = lo;
  if (neg) {
    ml = ~ml + 1;
    mh = ~mh + (ml == 0 ? 1 : 0);
  }
  if ((mh | ml) == 0) return 0.0;
  const int p = mh ? 127 - __clzll((long long)mh) : 63 - __clzll((long long)ml);   // the top bit
  unsigned long long keep;
  int shift = 0;
  if (p <= 52) {
    keep = ml;
  } else {
    shift = p - 52;                                 // 1..75
    unsigned long long rem_hi, rem_lo, half_hi, half_lo;
    if (shift < 64) {
      keep = (ml >> shift) | (mh << (64 - shift));  // (mh < 2^(p - 63): nothing of it is lost)
      rem_hi = 0;
      rem_lo = ml & ((1ULL << shift) - 1);
      half_hi = 0;
      half_lo = 1ULL << (shift - 1);
    } else {
      const int s2 = shift - 64;                    // 0..11
      keep = mh >> s2;
      rem_hi = s2 ? mh & ((1ULL << s2) - 1) : 0;
      rem_lo = ml;
      half_hi = s2 ? 1ULL << (s2 - 1) : 0;
      half_lo = s2 ? 0 : 1ULL << 63;
    }
    const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
    const bool tie = rem_hi == half_hi && rem_lo == half_lo;
    if (above || (tie && (keep & 1))) keep += 1;    // (2^53 at most: still exact as a double)
  }
  const double scale = __longlong_as_double((long long)(1023 + shift - 64) << 52);   // 2^(shift - 64), a normal number
  const double v = (double)keep * scale;            // exact: a 53-bit integer times a power of two
  return neg ? -v : v;
}

// the centroid (k, coordinate j) of a restart from one set of words; an empty cluster gives NaN, as np.mean([]) does
__device__ __forceinline__ double kmeans_centroid(const long long* set, int k, int j) {
  const long long* w = set + (size_t)k * KM_WORDS;
  const long long n = w[6];
  if (n == 0) return __builtin_nan("");
  return kmeans_words_to_double(w[3 * j], w[3 * j + 1], w[3 * j + 2]) / (double)n;
}

// the restart's fixed point: the first step t >= 1 whose assignment equals step t-1's
__device__ __forceinline__ void kmeans_note_converged(const KmWs& w, int K, int R, int r, int t) {
  if (t >= 1 && w.conv[r] < 0 && km_set(w, K, R, t % 3, r)[(size_t)K * KM_WORDS] == 0) w.conv[r] = t;
}

__global__ __launch_bounds__(64) void kmeans_init_kernel(void* ws, const double* __restrict__ pts, const int* __restrict__ init, int N,
                                                         int K, int R) {
  const KmWs w = km_ws(ws, K, R);
  const int r = blockIdx.x, j = threadIdx.x;
  if (j < 2 * K) {
    const int i = init[(size_t)r * K + (j >> 1)];
    w.cent0[((size_t)r * K) * 2 + j] = (i >= 0 && i < N) ? pts[(size_t)i * 2 + (j & 1)] : __builtin_nan("");
  }
  if (j == 0) w.conv[r] = -1;
}

// grid (ceil(N / 256), R): one thread per box and restart
__global__ __launch_bounds__(KM_THREADS) void kmeans_step_kernel(void* ws, const double* __restrict__ pts, unsigned char* __restrict__ assign,
                                                                 int N, int K, int R, int t) {
  __shared__ double cent[KM_MAXK * 2];
  __shared__ long long lacc[KM_MAXK * KM_WORDS + KM_TAIL];
  const KmWs w = km_ws(ws, K, R);
  const int r = blockIdx.y, tid = threadIdx.x;
  const int nw = K * KM_WORDS + KM_TAIL;
  if (tid < 2 * K)
    cent[tid] = t == 0 ? w.cent0[((size_t)r * K) * 2 + tid] : kmeans_centroid(km_set(w, K, R, (t + 2) % 3, r), tid >> 1, tid & 1);
  for (int j = tid; j < nw; j += KM_THREADS) lacc[j] = 0;
  if (blockIdx.x == 0) {
    long long* nxt = km_set(w, K, R, (t + 1) % 3, r);           // read last by step t-1
    for (int j = tid; j < nw; j += KM_THREADS) nxt[j] = 0;
    if (tid == 0) kmeans_note_converged(w, K, R, r, t - 1);
  }
  __syncthreads();
  const int i = blockIdx.x * KM_THREADS + tid;
  if (i < N) {
    const double h = pts[(size_t)i * 2], wd = pts[(size_t)i * 2 + 1];
    double best = __builtin_inf(), bq = 0.0;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
      const double dh = h - cent[2 * k], dw = wd - cent[2 * k + 1];
      const double q = dh * dh + dw * dw;             // three roundings: the file is compiled with -ffp-contract=off
      const double d = __dsqrt_rn(q);
      if (d < best) { best = d; bq = q; bi = k; }   // strict: the first minimum wins; a NaN compares false
    }
    unsigned char* ap = assign + (size_t)r * N + i;
    if (t == 0 || *ap != (unsigned char)bi) {
      *ap = (unsigned char)bi;
      atomicAdd(reinterpret_cast<unsigned long long*>(&lacc[K * KM_WORDS]), 1ULL);
    }
    long long dg[3];
    unsigned long long* la = reinterpret_cast<unsigned long long*>(&lacc[bi * KM_WORDS]);
    kmeans_digits(h, dg);
    for (int j = 0; j < 3; ++j) if (dg[j]) atomicAdd(la + j, (unsigned long long)dg[j]);
    kmeans_digits(wd, dg);
    for (int j = 0; j < 3; ++j) if (dg[j]) atomicAdd(la + 3 + j, (unsigned long long)dg[j]);
    atomicAdd(la + 6, 1ULL);
    const unsigned long long fx = (unsigned long long)(bq * 0x1p32);      // floor(q * 2^32): q <= 2^31, the product is exact
    atomicAdd(reinterpret_cast<unsigned long long*>(&lacc[K * KM_WORDS + 1]), fx & 0xffffffffULL);
    atomicAdd(reinterpret_cast<unsigned long long*>(&lacc[K * KM_WORDS + 2]), fx >> 32);
  }
  __syncthreads();
  long long* cur = km_set(w, K, R, t % 3, r);
  for (int j = tid; j < nw; j += KM_THREADS) {
    const long long v = lacc[j];
    if (v) __hip_atomic_fetch_add(cur + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid R, after step t: the record [R][MDCV_KMEANS_REC_HEAD + 2K] of 8-byte words the host reads
__global__ __launch_bounds__(64) void kmeans_record_kernel(void* ws, long long* __restrict__ rec, int K, int R, int t) {
  __shared__ int nanc;
  const KmWs w = km_ws(ws, K, R);
  const int r = blockIdx.x, j = threadIdx.x;
  if (j == 0) {
    nanc = 0;
    kmeans_note_converged(w, K, R, r, t);
  }
  __syncthreads();
  const long long* set = km_set(w, K, R, t % 3, r);
  long long* out = rec + (size_t)r * (MDCV_KMEANS_REC_HEAD + 2 * K);
  if (j < 2 * K) {
    const double c = kmeans_centroid(set, j >> 1, j & 1);
    if (c != c) atomicOr(&nanc, 1);
    out[MDCV_KMEANS_REC_HEAD + j] = __double_as_longlong(c);
  }
  __syncthreads();
  if (j == 0) {
    out[0] = w.conv[r];
    out[1] = set[(size_t)K * KM_WORDS + 1];
    out[2] = set[(size_t)K * KM_WORDS + 2];
    out[3] = nanc;
  }
}

bool km_shape_ok(long long N, int K, int R) { return K >= 1 && K <= KM_MAXK && R >= 1 && R <= KM_MAXR && N >= 1 && N < (1LL << 24); }

}  // namespace

extern "C" {

long long mdcv_kmeans_workspace_bytes(long long N, int K, int R) {
  if (!km_shape_ok(N, K, R)) return MDCV_EARG;
  return (long long)(((size_t)R * K * 2 + 3 * (size_t)R * km_set_words(K) + (size_t)R) * 8);
}

int mdcv_kmeans_begin(void* ws, const double* points, const int* init, long long N, int K, int R, void* stream) {
  if (!ws || !points || !init || !km_shape_ok(N, K, R)) return MDCV_EARG;
  const hipError_t e = hipMemsetAsync(ws, 0, (size_t)mdcv_kmeans_workspace_bytes(N, K, R), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  MDCV_LAUNCH(kmeans_init_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, ws, points, init, (int)N, K, R);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_kmeans_steps(void* ws, const double* points, unsigned char* assign, long long* record, long long N, int K, int R, int t0,
                      int n_steps, void* stream) {
  if (!ws || !points || !assign || !record || !km_shape_ok(N, K, R) || t0 < 0 || n_steps < 1 || n_steps > (1 << 20) ||
      t0 > INT32_MAX - n_steps)
    return MDCV_EARG;
  const dim3 grid((unsigned)((N + KM_THREADS - 1) / KM_THREADS), (unsigned)R);
  for (int t = t0; t < t0 + n_steps; ++t) {
    MDCV_LAUNCH(kmeans_step_kernel, grid, dim3(KM_THREADS), 0, (hipStream_t)stream, ws, points, assign, (int)N, K, R, t);
    MDCV_CHECK_LAUNCH();
  }
  MDCV_LAUNCH(kmeans_record_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, ws, record, K, R, t0 + n_steps - 1);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
