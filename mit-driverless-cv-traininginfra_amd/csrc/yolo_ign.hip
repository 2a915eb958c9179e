// Opt-in prediction-IoU ignore rule of the fused YOLO head for gfx950 (libmdcv_ign.so, include/mdcv_ign.h): Darknet's
// `ignore_thresh`.  A cell without an owner whose PREDICTED box overlaps a labelled box of its own image by more than thr leaves the
// no-object term.  The definition is in the header.
//
// Unlike the class and the box loss (sparse: they walk label rows) this is DENSE: every one of the B*A*Gh*Gw predictions meets every
// label of its image.  The split:
//   grid = (image, slab of 256 cells), one LANE per cell, 4 waves per workgroup; no grid cap, so a workgroup's index IS its mask word
//   cell order inside an image is pixel-major, anchor-minor (q -> pixel q / A, anchor q % A): a wave reads the logits of 64 / A
//     neighbouring pixels, every anchor of them, so a 128-byte line of the logits plane is fetched by ONE wave, once.  With C = 1,
//     ldc = 24 (48-byte bf16 pixels) the 64 five-word groups of a wave lie in 1024 consecutive bytes, 8 whole lines; the head's
//     anchor-major order spreads them over 3072 bytes and fetches every line from three workgroups.  With C = 80, ldc = 256 a line
//     holds one group whatever the order (groups are 170 bytes apart): one line per cell, as in yolo_loss_kernel
//   the workgroup first compacts the REAL label rows of its image into LDS as (x1, y1, x2, y2, area): one row per lane, ballot, prefix
//     by popcount, wave bases through LDS; kRows rows per pass, ceil(T / kRows) passes, so any T is served
//   a lane that is owned, excluded by the batch-wide plane or past the image is inactive from the start and loads nothing; an active
//     lane loads x, y, w, h, conf as one vector (+ one word) where the address allows and decodes its box ONCE into registers
//   the row loop reads LDS at a wave-uniform address: a broadcast, no bank conflict; the test inter > thr * union has no division and
//     forms the union only where the overlap is positive; a wave leaves the loop when a ballot shows every active lane decided
//   the result is a ballot: one 64-bit word per wave, stored by lane 0; BCE(p, 0) of the ignored lanes is reduced per wave in fp64 (the
//     count is the popcount of the ballot), four waves through LDS, one atomic pair per workgroup, skipped when nothing was ignored
//   a one-thread finalize (a launch of its own for the reason yolo_head.hip gives) folds (S, n) into out7 and into acc[5] / acc[7] of
//     the HEAD workspace, so that mdcv_yolo_head_grad scales the remaining negatives by 1 / nN' unchanged, and zeroes (S, n)
//   the gradient pass runs the same (workgroup, lane) -> cell map over the mask words: a wave whose word is zero leaves at once, a
//     lane whose bit is set stores 0 * gscale into its cell's conf word
// Compiled with -ffp-contract=off: the decision is a threshold, every product and sum rounds on its own as the header states it.
#include "yolo_head_core.h"
#include "../../include/mdcv_ign.h"

namespace {

constexpr int kBlock = 256;                                   // lanes of a workgroup = cells of a slab
constexpr int kWaves = kBlock / 64;
constexpr int kRows = kBlock;                                 // label rows compacted per pass: one per lane

struct IgnArgs {
  const void* logits; const float* tg; const float* anchors; const int* owner; const int* ignore;
  double* acc; unsigned long long* mask;
  HeadGeom g;                                                 // (g.thresh is thr)
  int slabs;                                                  // ceil(A*Gh*Gw / kBlock)
};

// x, y, w, h, conf of one cell: four as one vector (bf16: one 8-byte or two 4-byte loads) where the address allows
template <typename T> struct V5;
template <> struct V5<float> {
  __device__ static __forceinline__ void ld(const float* p, float* z) {
    if (((uintptr_t)p & 15) == 0) { const float4 v = *reinterpret_cast<const float4*>(p); z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w; }
    else { z[0] = p[0]; z[1] = p[1]; z[2] = p[2]; z[3] = p[3]; }
    z[4] = p[4];
  }
};
template <> struct V5<bf16_t> {
  __device__ static __forceinline__ void ld(const bf16_t* p, float* z) {
    if (((uintptr_t)p & 3) == 0) {
      uint2 v;
      if (((uintptr_t)p & 7) == 0) v = *reinterpret_cast<const uint2*>(p);
      else { v.x = reinterpret_cast<const unsigned*>(p)[0]; v.y = reinterpret_cast<const unsigned*>(p)[1]; }
      z[0] = __uint_as_float(v.x << 16); z[1] = __uint_as_float(v.x & 0xffff0000u);
      z[2] = __uint_as_float(v.y << 16); z[3] = __uint_as_float(v.y & 0xffff0000u);
    } else { z[0] = bf2f(p[0]); z[1] = bf2f(p[1]); z[2] = bf2f(p[2]); z[3] = bf2f(p[3]); }
    z[4] = bf2f(p[4]);
  }
};

template <typename T>
__global__ __launch_bounds__(kBlock) void yolo_ign_mask_kernel(IgnArgs a) {
  __shared__ float rows[kRows][5];                            // x1 y1 x2 y2 area of the real rows of this pass, compacted
  __shared__ int wcount[kWaves];
  __shared__ double red[kWaves];
  __shared__ int redn[kWaves];
  const HeadGeom& g = a.g;
  const int b = blockIdx.x / a.slabs, slab = blockIdx.x - b * a.slabs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = g.A * g.Gh * g.Gw, q = slab * kBlock + threadIdx.x;
  bool active = q < per;
  float px1 = 0.f, py1 = 0.f, px2 = 0.f, py2 = 0.f, parea = 0.f, zc = 0.f;
  if (active) {
    const int pix = q / g.A, an = q - pix * g.A;
    const int j = pix / g.Gw, i = pix - j * g.Gw;
    active = a.owner[(((size_t)b * g.A + an) * g.Gh + j) * g.Gw + i] < 0 && a.ignore[pix] == 0;
    if (active) {
      float z[5];
      V5<T>::ld(reinterpret_cast<const T*>(a.logits) + ((size_t)b * g.Gh * g.Gw + pix) * g.ldc + an * (5 + g.C), z);
      const float px = sigmoidf_(z[0]) + (float)i, py = sigmoidf_(z[1]) + (float)j;
      const float pw = expf(fminf(z[2], 20.f)) * a.anchors[2 * an], ph = expf(fminf(z[3], 20.f)) * a.anchors[2 * an + 1];
      const float hw = pw * 0.5f, hh = ph * 0.5f;
      px1 = px - hw; px2 = px + hw; py1 = py - hh; py2 = py + hh;
      parea = pw * ph; zc = z[4];
    }
  }
  bool hit = false;
  for (int t0 = 0; t0 < g.T; t0 += kRows) {
    const int t = t0 + threadIdx.x;
    bool real = false;
    float gx = 0.f, gy = 0.f, gw = 0.f, gh = 0.f;
    if (t < g.T) {
      const float* r = a.tg + ((size_t)b * g.T + t) * 5;
      float s = r[0]; s = s + r[1]; s = s + r[2]; s = s + r[3]; s = s + r[4];     // the head's master_mask (assign_row)
      real = s > 0.f;
      gx = r[1] * (float)g.Gw; gy = r[2] * (float)g.Gh; gw = r[3] * (float)g.Gw; gh = r[4] * (float)g.Gh;
    }
    const unsigned long long m = __ballot(real);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) { base += w < wave ? wcount[w] : 0; total += wcount[w]; }
    if (real) {
      float* d = rows[base + __popcll(m & ((1ull << lane) - 1ull))];
      const float hw = gw * 0.5f, hh = gh * 0.5f;
      d[0] = gx - hw; d[1] = gy - hh; d[2] = gx + hw; d[3] = gy + hh; d[4] = gw * gh;
    }
    __syncthreads();
    for (int k = 0; k < total; ++k) {
      if (__ballot(active && !hit) == 0) break;               // every active lane of the wave is decided
      const float iw = fminf(px2, rows[k][2]) - fmaxf(px1, rows[k][0]);
      const float ih = fminf(py2, rows[k][3]) - fmaxf(py1, rows[k][1]);
      if (active && iw > 0.f && ih > 0.f) {
        const float inter = iw * ih;
        const float uni = parea + rows[k][4] - inter + 1e-7f;
        hit = hit || inter > g.thresh * uni;
      }
    }
    __syncthreads();                                          // rows / wcount are rewritten by the next pass
  }
  const unsigned long long hm = __ballot(hit);
  if (lane == 0) a.mask[(size_t)blockIdx.x * kWaves + wave] = hm;
  float bce = 0.f;
  if (hit) bce = -fmaxf(logf(1.f - sigmoidf_(zc)), -100.f);  // BCE(p, 0) as yolo_loss_kernel forms it
  const double s = wave_sum_d((double)bce);
  if (lane == 0) { red[wave] = s; redn[wave] = __popcll(hm); }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = redn[0] + redn[1] + redn[2] + redn[3];
    if (n != 0) {
      atomicAdd(a.acc + 0, red[0] + red[1] + red[2] + red[3]);
      atomicAdd(a.acc + 1, (double)n);
    }
  }
}

// out7[0], out7[6] += the change of loss_noobj ; ign_out = (n, nN') ; acc[5], acc[7] of the HEAD workspace become acc5 - S, nN' ; the
// sums are cleared for the next call.  n == 0: out7 and the head workspace keep every bit.
__global__ void yolo_ign_finalize_kernel(double* __restrict__ head_acc, double* __restrict__ acc, float k, float* __restrict__ out7,
                                         float* __restrict__ ign_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double S = acc[0], n = acc[1], acc5 = head_acc[5], nN = head_acc[7];
  const double left = nN - n;
  ign_out[0] = (float)n; ign_out[1] = (float)left;
  if (n == 0.0) return;
  const double rest = left == 0.0 ? 0.0 : acc5 - S;           // nothing left: the sum over an empty selection is 0, its mean NaN
  const float d = (float)((double)k * (rest / left - acc5 / nN));
  out7[0] += d; out7[6] += d;
  head_acc[5] = rest; head_acc[7] = left;
  acc[0] = 0.0; acc[1] = 0.0;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void yolo_ign_grad_kernel(const unsigned long long* __restrict__ mask, void* __restrict__ dlogits,
                                                               const float* __restrict__ gscale, int A, int C, int Gh, int Gw, int ldd, int slabs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = mask[(size_t)blockIdx.x * kWaves + wave];
  const int b = blockIdx.x / slabs, q = (blockIdx.x - b * slabs) * kBlock + threadIdx.x;
  if (((m >> lane) & 1ull) == 0 || q >= A * Gh * Gw) return;
  const int pix = q / A, an = q - pix * A;
  ET<T>::st(reinterpret_cast<T*>(dlogits) + ((size_t)b * Gh * Gw + pix) * ldd + an * (5 + C) + 4, 0.f * (gscale ? gscale[0] : 1.f));
}

static long long slabs_of(int A, int Gh, int Gw) { return ((long long)A * Gh * Gw + kBlock - 1) / kBlock; }

static bool bad_geometry(int dtype, int B, int A, int C, int Gh, int Gw) {
  if (dtype != MDCV_F32 && dtype != MDCV_BF16) return true;
  if (B < 1 || A < 1 || C < 1 || Gh < 1 || Gw < 1) return true;
  if (Gh > 4095 || Gw > 4095 || A > 127) return true;
  return (long long)B * slabs_of(A, Gh, Gw) > (1LL << 31) - 1;
}

}  // namespace

extern "C" {

long long mdcv_yolo_ign_workspace_bytes(int B, int A, int Gh, int Gw) {
  if (B < 1 || A < 1 || Gh < 1 || Gw < 1) return 16;
  return 16 + (long long)B * slabs_of(A, Gh, Gw) * kWaves * 8;      // (S, n) in fp64, then one 64-bit word per wave
}

int mdcv_yolo_ign_rows_per_pass(void) { return kRows; }

int mdcv_yolo_ign_loss(int dtype, const void* logits, int ldc, const float* targets, const float* anchors_scaled, int B, int T, int A, int C,
                       int Gh, int Gw, float thr, float no_object_loss, void* head_workspace, void* ign_workspace, float* out7,
                       float* ign_out, void* stream) {
  if (!logits || !targets || !anchors_scaled || !head_workspace || !ign_workspace || !out7 || !ign_out) return MDCV_EARG;
  if (bad_geometry(dtype, B, A, C, Gh, Gw) || T < 1 || (long long)A * (5 + C) > ldc || (long long)B * T > (1LL << 31) - (1LL << 16)) return MDCV_EARG;
  if (!(thr > 0.f && thr < 1.f) || ((uintptr_t)ign_workspace & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const HeadWs hw = head_ws(head_workspace, B, A, Gh, Gw);
  const int slabs = (int)slabs_of(A, Gh, Gw);
  IgnArgs a{logits, targets, anchors_scaled, hw.owner, hw.ignore, (double*)ign_workspace, (unsigned long long*)ign_workspace + 2,
            HeadGeom{B, T, A, C, Gh, Gw, ldc, thr}, slabs};
  const dim3 grid((unsigned)((long long)B * slabs));
  if (dtype == MDCV_BF16) hipLaunchKernelGGL(yolo_ign_mask_kernel<bf16_t>, grid, dim3(kBlock), 0, st, a);
  else hipLaunchKernelGGL(yolo_ign_mask_kernel<float>, grid, dim3(kBlock), 0, st, a);
  MDCV_CHECK_LAUNCH();
  hipLaunchKernelGGL(yolo_ign_finalize_kernel, dim3(1), dim3(64), 0, st, hw.acc, a.acc, no_object_loss, out7, ign_out);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int mdcv_yolo_ign_grad(int dtype, void* dlogits, int ldd, int Cpad, int B, int A, int C, int Gh, int Gw, const void* ign_workspace,
                       const float* gscale, void* stream) {
  if (!dlogits || !ign_workspace) return MDCV_EARG;
  if (bad_geometry(dtype, B, A, C, Gh, Gw) || (long long)A * (5 + C) > Cpad || ldd < Cpad || ((uintptr_t)ign_workspace & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  const int slabs = (int)slabs_of(A, Gh, Gw);
  const unsigned long long* mask = (const unsigned long long*)ign_workspace + 2;
  const dim3 grid((unsigned)((long long)B * slabs));
  if (dtype == MDCV_BF16) hipLaunchKernelGGL(yolo_ign_grad_kernel<bf16_t>, grid, dim3(kBlock), 0, st, mask, dlogits, gscale, A, C, Gh, Gw, ldd, slabs);
  else hipLaunchKernelGGL(yolo_ign_grad_kernel<float>, grid, dim3(kBlock), 0, st, mask, dlogits, gscale, A, C, Gh, Gw, ldd, slabs);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
