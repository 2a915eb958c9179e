// Augmentation of a finished key-point batch (include/mdcv_kptaug.h): per image an affine warp of the crop (bilinear gather through
// the INVERSE map, edge replicate), a per-channel gain and bias, the seven key points through the FORWARD map (left/right swapped under a
// flip), and the seven heat-maps REGENERATED from the transformed points (kpt_heatmap.h at ow = oh = S, where cv2's resize is the identity).
// The host supplies both maps; nothing is inverted here.  An image whose transformed points leave [0, S] passes through as bits, and so does
// one whose descriptor says so or fails the check.  Every fp32 operation rounds on its own (built with -ffp-contract=off); a NumPy
// restatement (tests/kptaug_ref.py) reproduces all three outputs bit for bit.
//
// ONE launch, grid (C + 7, B): one workgroup per output plane, as kptload.hip does it -- planes 0..C-1 the image channels, the rest the
// heat-maps.  The decision (14 products through F, 28 comparisons) is taken by every thread from uniform loads: it costs less than sharing
// it.  The workgroup of plane 0 also writes the image's points and counters.  The gather reads the 4 S^2-byte source plane, which stays in
// L2 between its (up to four) reads per output pixel; with S % 4 == 0 and 16-byte-aligned buffers each lane stores 16 bytes, lanes
// consecutive along x.  A heat-map plane holds its two separable vectors in both stages in LDS: 32 S + 16 bytes, declared for S = 256 (8 KB).
#include "kpt_heatmap.h"
#include "kptaug_desc.h"
#include "../../include/mdcv_kptaug.h"

#define KPTAUG_THREADS 256
#define KPTAUG_K 7
#define KPTAUG_MIN_S 16                           // MIN_SIZE / MAX_SIZE of mdcv/data/crops.py
#define KPTAUG_MAX_S 256
#define KPTAUG_MAX_B 65535                        // grid.y

namespace {

struct KptAugArgs {
  const int* desc; int B, C, S, vec;
  const float* imgs; const float* hm; const float* pts;
  float* imgs_out; float* hm_out; float* pts_out;
  int* stats;
};

// the partner of key point k under a left/right flip: [0, 2, 1, 4, 3, 6, 5]
__device__ __forceinline__ int kptaug_perm(int k) { return k == 0 ? 0 : (((k - 1) ^ 1) + 1); }

// one point (x, y normalised by S) through the forward map, in pixel-index coordinates
__device__ __forceinline__ void kptaug_point(const float* F, const float* p, float Sf, float& X, float& Y) {
  const float px = p[0] * Sf, py = p[1] * Sf;
  X = (F[0] * px + F[1] * py) + F[2];
  Y = (F[3] * px + F[4] * py) + F[5];
}

__device__ __forceinline__ float kptaug_sample(const float* __restrict__ src, int S, float Sf, const float* I, float xf, float yf, float gain,
                                               float bias) {
  const float sx = fminf(fmaxf((I[0] * xf + I[1] * yf) + I[2], -1.f), Sf);        // a NaN becomes -1: fmaxf returns the other operand
  const float sy = fminf(fmaxf((I[3] * xf + I[4] * yf) + I[5], -1.f), Sf);
  const float xf0 = floorf(sx), yf0 = floorf(sy);
  const float fx = sx - xf0, fy = sy - yf0;
  const int xi = (int)xf0, yi = (int)yf0;                                         // in [-1, S]
  const int x0 = min(max(xi, 0), S - 1), x1 = min(max(xi + 1, 0), S - 1);
  const int y0 = min(max(yi, 0), S - 1), y1 = min(max(yi + 1, 0), S - 1);
  const float* r0 = src + y0 * S;
  const float* r1 = src + y1 * S;
  const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
  const float top = v00 + fx * (v01 - v00);
  const float bot = v10 + fx * (v11 - v10);
  const float v = top + fy * (bot - top);
  return fminf(fmaxf(v * gain + bias, 0.f), 1.f);
}

__device__ __forceinline__ void kptaug_copy(const float* __restrict__ in, float* __restrict__ out, int n, bool vec, int tid) {
  if (vec) {
    const uint4* i4 = reinterpret_cast<const uint4*>(in);
    uint4* o4 = reinterpret_cast<uint4*>(out);
    for (int i = tid; i < (n >> 2); i += KPTAUG_THREADS) o4[i] = i4[i];
  } else {
    const unsigned* i1 = reinterpret_cast<const unsigned*>(in);
    unsigned* o1 = reinterpret_cast<unsigned*>(out);
    for (int i = tid; i < n; i += KPTAUG_THREADS) o1[i] = i1[i];
  }
}

__global__ __launch_bounds__(KPTAUG_THREADS) void kptaug_kernel(KptAugArgs A) {
  __shared__ double s_rz[2 * KPTAUG_MAX_S], s_bl[2 * KPTAUG_MAX_S], s_sums[2];
  __shared__ int s_hot[2];
  const int plane = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, S = A.S, C = A.C;
  const float Sf = (float)S;
  const size_t pl = (size_t)S * S;

  int d[MDCV_KPTAUG_DESC];
  for (int k = 0; k < MDCV_KPTAUG_DESC; ++k) d[k] = A.desc[(size_t)b * MDCV_KPTAUG_DESC + k];
  const bool ok = kptaug_row_ok(d);
  float I[6], F[6];
  for (int k = 0; k < 6; ++k) { I[k] = __int_as_float(d[KA_INV + k]); F[k] = __int_as_float(d[KA_FWD + k]); }
  const float* p = A.pts + (size_t)b * KPTAUG_K * 2;
  bool valid = true;
  for (int k = 0; k < KPTAUG_K; ++k) {
    float X, Y;
    kptaug_point(F, p + 2 * k, Sf, X, Y);
    valid = valid && X >= 0.f && X <= Sf && Y >= 0.f && Y <= Sf;                  // a NaN fails
  }
  const bool wanted = ok && (d[KA_FLAGS] & KA_APPLY);
  const bool apply = wanted && valid;
  const bool swap = (d[KA_FLAGS] & KA_SWAP) != 0;

  if (plane == 0) {
    if (tid == 0) {
      if (!ok) atomicOr(A.stats + 3, 1);
      atomicAdd(A.stats + (apply ? 0 : wanted ? 1 : 2), 1);
    }
    if (tid < KPTAUG_K * 2) {
      const int k = tid >> 1;
      float* po = A.pts_out + (size_t)b * KPTAUG_K * 2;
      if (apply) {
        float X, Y;
        kptaug_point(F, p + 2 * (swap ? kptaug_perm(k) : k), Sf, X, Y);
        po[tid] = ((tid & 1) ? Y : X) / Sf;
      } else {
        reinterpret_cast<unsigned*>(po)[tid] = reinterpret_cast<const unsigned*>(p)[tid];
      }
    }
  }

  if (plane < C) {
    const float* __restrict__ src = A.imgs + ((size_t)b * C + plane) * pl;
    float* __restrict__ out = A.imgs_out + ((size_t)b * C + plane) * pl;
    if (!apply) {
      kptaug_copy(src, out, (int)pl, A.vec != 0, tid);
      return;
    }
    const float gain = __int_as_float(d[KA_GAIN + plane]), bias = __int_as_float(d[KA_BIAS + plane]);      // plane < C <= 3
    if (A.vec) {
      const int S4 = S >> 2;
      for (int i = tid; i < S * S4; i += KPTAUG_THREADS) {
        const int y = i / S4, x = (i - y * S4) * 4;
        const float yf = (float)y;
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = kptaug_sample(src, S, Sf, I, (float)(x + j), yf, gain, bias);
        *reinterpret_cast<f32x4_t*>(out + (size_t)i * 4) = o;
      }
    } else {
      for (int i = tid; i < S * S; i += KPTAUG_THREADS) {
        const int y = i / S, x = i - y * S;
        out[i] = kptaug_sample(src, S, Sf, I, (float)x, (float)y, gain, bias);
      }
    }
    return;
  }

  const int k = plane - C;                                                        // 0..6
  const float* __restrict__ src = A.hm + ((size_t)b * KPTAUG_K + k) * pl;
  float* __restrict__ out = A.hm_out + ((size_t)b * KPTAUG_K + k) * pl;
  if (!apply) {
    kptaug_copy(src, out, (int)pl, A.vec != 0, tid);
    return;
  }
  if (tid == 0) {
    float X, Y;
    kptaug_point(F, p + 2 * (swap ? kptaug_perm(k) : k), Sf, X, Y);               // both in [0, Sf]: the image is valid
    s_hot[0] = min((int)X, S - 1);
    s_hot[1] = min((int)Y, S - 1);
  }
  __syncthreads();
  kpthm::axes(s_rz, s_bl, s_sums, s_hot, 1, S, S, S, tid, KPTAUG_THREADS);
  kpthm::store(out, s_bl, s_sums, 1, S, tid, KPTAUG_THREADS, A.vec != 0);
}

bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
  const unsigned long long a0 = (unsigned long long)(size_t)a, b0 = (unsigned long long)(size_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" {

int mdcv_kptaug_batch(const int* desc_host, const int* desc, int B, int C, int S, int K, const float* imgs, const float* hm, const float* pts,
                      float* imgs_out, float* hm_out, float* pts_out, int* stats, void* stream) {
  if (!desc_host || !desc || !imgs || !hm || !pts || !imgs_out || !hm_out || !pts_out || !stats) return MDCV_EARG;
  if (B < 1 || B > KPTAUG_MAX_B || C < 1 || C > 3 || S < KPTAUG_MIN_S || S > KPTAUG_MAX_S || K != KPTAUG_K) return MDCV_EARG;
  const unsigned long long plane = (unsigned long long)S * S * 4ull;
  const void* buf[6] = {imgs, hm, pts, imgs_out, hm_out, pts_out};
  const unsigned long long len[6] = {(unsigned long long)B * C * plane, (unsigned long long)B * K * plane, (unsigned long long)B * K * 8ull,
                                     (unsigned long long)B * C * plane, (unsigned long long)B * K * plane, (unsigned long long)B * K * 8ull};
  for (int o = 3; o < 6; ++o)                                                     // an output against every input and the outputs behind it
    for (int i = 0; i < o; ++i)
      if (overlap(buf[o], len[o], buf[i], len[i])) return MDCV_EARG;
  for (int o = 3; o < 6; ++o)
    if (overlap(buf[o], len[o], stats, 16ull)) return MDCV_EARG;
  for (int b = 0; b < B; ++b)
    if (!kptaug_row_ok(desc_host + (size_t)b * MDCV_KPTAUG_DESC)) return MDCV_EARG;
  bool aligned = true;
  for (int i = 0; i < 6; ++i)
    if (i != 2 && i != 5 && ((uintptr_t)buf[i] & 15)) aligned = false;
  KptAugArgs a{desc, B, C, S, (S % 4 == 0 && aligned) ? 1 : 0, imgs, hm, pts, imgs_out, hm_out, pts_out, stats};
  hipLaunchKernelGGL(kptaug_kernel, dim3((unsigned)(C + KPTAUG_K), (unsigned)B), dim3(KPTAUG_THREADS), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCV_OK : (int)e;
}

}  // extern "C"
