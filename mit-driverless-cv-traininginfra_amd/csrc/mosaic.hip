// Mosaic augmentation of a finished detector batch (include/mdcv_aug.h): every output image is composed from the corners of
// four images of the same batch, around a centre (xc, yc), and the labels of the four sources are shifted, clipped to their quadrant,
// filtered and packed.  The tiles are already at the network's size, so nothing is resampled: the pixels are a gather of fp32 words copied
// as bits, the labels a handful of single fp32 operations (built with -ffp-contract=off; a NumPy restatement reproduces them bit for bit).
// ONE launch: blockIdx.x < pix_blocks copy pixels, the B blocks behind them do the labels of one output image each.
//
// Pixels.  A wave owns one output row (b, c, y) at a time: left of xc it comes from one row of source s(2 qy), right of it from one row of
// source s(2 qy + 1).  Lanes take 16-byte cells of the OUTPUT address space (one dwordx4 store each; the cells cut by the row's ends are
// written word by word); the source run sits at xc mod 4 words against them, so it is loaded as dwords -- the wave still reads one
// contiguous span per run.
//
// Labels.  One workgroup per output image walks quadrant 0..3 and, inside a quadrant, the source's rows in chunks of the block size.  The
// kept rows of a chunk are compacted by ballot and prefix popcount (lane order inside a wave, wave order inside the chunk), and the running
// count carries over from chunk to chunk, so the output order is fixed whatever the schedule.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mosaic_desc.h"
#include "../../include/mdcv_aug.h"

#define MOSAIC_THREADS 256
#define MOSAIC_WAVES (MOSAIC_THREADS / 64)
#define MOSAIC_MAX_PIX_BLOCKS 2048               // 8 blocks per CU; the rows beyond are reached by the grid stride
#define MOSAIC_MAX_B 65535

namespace {

// Plain loads, not non-temporal ones: a source image is read by about four outputs of the launch and the first convolution reads the
// output next (measured, DESIGN §29: 26.5 us against 41.4 us with __builtin_nontemporal_load here)
__device__ __forceinline__ unsigned mosaic_ld(const unsigned* p) { return *p; }

// One candidate row r = (cls, cx, cy, w, h) of the source shown in quadrant (qx, qy) -> the row it becomes, or false.  Every operation
// rounds on its own; fmaxf / fminf return the other operand for a NaN, so a NaN collapses the box onto a clamp bound and w' or h' is 0.
__device__ __forceinline__ bool mosaic_label(const float* r, int qx, int qy, int xc, int yc, int H, int W, float min_px, float min_visible,
                                             float* o) {
  const float Wf = (float)W, Hf = (float)H;
  const float hw = r[3] * 0.5f, hh = r[4] * 0.5f;
  const float x1 = (r[1] - hw) * Wf, x2 = (r[1] + hw) * Wf;
  const float y1 = (r[2] - hh) * Hf, y2 = (r[2] + hh) * Hf;
  const float dx = (float)(qx ? xc : xc - W), dy = (float)(qy ? yc : yc - H);
  const float xlo = qx ? (float)xc : 0.0f, xhi = qx ? Wf : (float)xc;
  const float ylo = qy ? (float)yc : 0.0f, yhi = qy ? Hf : (float)yc;
  const float X1 = fminf(fmaxf(x1 + dx, xlo), xhi), X2 = fminf(fmaxf(x2 + dx, xlo), xhi);
  const float Y1 = fminf(fmaxf(y1 + dy, ylo), yhi), Y2 = fminf(fmaxf(y2 + dy, ylo), yhi);
  const float w = X2 - X1, h = Y2 - Y1;
  const float area = (x2 - x1) * (y2 - y1);
  if (!(w >= min_px && h >= min_px && w * h >= min_visible * area)) return false;
  o[0] = r[0];
  o[1] = ((X1 + X2) * 0.5f) / Wf;
  o[2] = ((Y1 + Y2) * 0.5f) / Hf;
  o[3] = w / Wf;
  o[4] = h / Hf;
  return true;
}

__device__ __forceinline__ bool mosaic_candidate(const float* r) { return (((r[0] + r[1]) + r[2]) + r[3]) + r[4] > 0.0f; }

__global__ __launch_bounds__(MOSAIC_THREADS) void mosaic_kernel(const int* __restrict__ desc, int B, int C, int H, int W, unsigned pix_blocks,
                                                                const unsigned* __restrict__ in, unsigned* __restrict__ out,
                                                                const float* __restrict__ tin, int T, float* __restrict__ tout, int T_out,
                                                                float min_px, float min_visible, int* __restrict__ stats) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  if (blockIdx.x < pix_blocks) {
    const unsigned rows = (unsigned)B * (unsigned)C * (unsigned)H;                 // <= 65535 * 4 * 4096 < 2^31
    const unsigned mis = (unsigned)(((uintptr_t)out >> 2) & 3u);                   // words from a 16-byte boundary to out[0]
    for (unsigned row = blockIdx.x * MOSAIC_WAVES + wave; row < rows; row += pix_blocks * MOSAIC_WAVES) {
      const int y = (int)(row % (unsigned)H);
      const unsigned bc = row / (unsigned)H;
      const int c = (int)(bc % (unsigned)C), b = (int)(bc / (unsigned)C);
      int d[MDCV_MOSAIC_DESC];
      for (int k = 0; k < MDCV_MOSAIC_DESC; ++k) d[k] = desc[(size_t)b * MDCV_MOSAIC_DESC + k];
      const bool apply = mosaic_row_ok(d, B, H, W) && d[M_APPLY] == 1;
      // pass-through is the mosaic with the centre at (0, 0) and every source b: quadrant 3 alone, unshifted
      const int xc = apply ? d[M_XC] : 0, yc = apply ? d[M_YC] : 0;
      const int qy = y >= yc ? 1 : 0;
      const int sy = y - yc + (qy ? 0 : H);                                        // in [0, H)
      const int sl = apply ? d[M_S0 + 2 * qy] : b, sr = apply ? d[M_S0 + 2 * qy + 1] : b;
      // word offsets such that source word = off + x: left run x in [0, xc) reads columns [W - xc, W), right run [xc, W) reads [0, W - xc)
      const long long off_l = (((long long)sl * C + c) * H + sy) * W + (W - xc);
      const long long off_r = (((long long)sr * C + c) * H + sy) * W - xc;
      const size_t o0 = (size_t)row * (size_t)W;
      unsigned* po = out + o0;
      const int a0 = (int)((o0 + mis) & 3u);                                       // the row starts a0 words into a 16-byte cell
      for (int x0 = lane * 4 - a0; x0 < W; x0 += 64 * 4) {
        if (x0 >= 0 && x0 + 4 <= W) {
          uint4 v;
          v.x = mosaic_ld(in + ((x0 + 0 < xc ? off_l : off_r) + x0 + 0));
          v.y = mosaic_ld(in + ((x0 + 1 < xc ? off_l : off_r) + x0 + 1));
          v.z = mosaic_ld(in + ((x0 + 2 < xc ? off_l : off_r) + x0 + 2));
          v.w = mosaic_ld(in + ((x0 + 3 < xc ? off_l : off_r) + x0 + 3));
          *reinterpret_cast<uint4*>(po + x0) = v;
        } else {
          for (int k = 0; k < 4; ++k) {
            const int x = x0 + k;
            if (x >= 0 && x < W) po[x] = mosaic_ld(in + ((x < xc ? off_l : off_r) + x));
          }
        }
      }
    }
    return;
  }

  // ---- labels of output image b
  __shared__ int s_wtot[2][MOSAIC_WAVES];
  __shared__ int s_cnt[3];
  const int b = (int)(blockIdx.x - pix_blocks);
  if (tid < 3) s_cnt[tid] = 0;
  int d[MDCV_MOSAIC_DESC];
  for (int k = 0; k < MDCV_MOSAIC_DESC; ++k) d[k] = desc[(size_t)b * MDCV_MOSAIC_DESC + k];
  const bool ok = mosaic_row_ok(d, B, H, W);
  const bool apply = ok && d[M_APPLY] == 1;
  if (!ok && tid == 0) atomicOr(stats + 3, 1);
  __syncthreads();
  float* to = tout + (size_t)b * T_out * 5;
  int kept = 0, dropped = 0, lost = 0;

  if (!apply) {                                                  // rows in place, padded rows included
    const float* ti = tin + (size_t)b * T * 5;
    const int n = T > T_out ? T : T_out;
    for (int t = tid; t < n; t += MOSAIC_THREADS) {
      float r[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (t < T) {
        for (int k = 0; k < 5; ++k) r[k] = ti[(size_t)t * 5 + k];
        if (mosaic_candidate(r)) {
          if (t < T_out) ++kept; else ++lost;
        }
      }
      if (t < T_out)
        for (int k = 0; k < 5; ++k) to[(size_t)t * 5 + k] = r[k];
    }
  } else {
    int base = 0, par = 0;                                       // kept rows of the chunks before this one
    for (int q = 0; q < 4; ++q) {
      const float* ti = tin + (size_t)d[M_S0 + q] * T * 5;
      for (int t0 = 0; t0 < T; t0 += MOSAIC_THREADS, par ^= 1) {
        const int t = t0 + tid;
        float o[5];
        bool keep = false;
        if (t < T) {
          float r[5];
          for (int k = 0; k < 5; ++k) r[k] = ti[(size_t)t * 5 + k];
          if (mosaic_candidate(r)) {
            keep = mosaic_label(r, q & 1, q >> 1, d[M_XC], d[M_YC], H, W, min_px, min_visible, o);
            if (!keep) ++dropped;
          }
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_wtot[par][wave] = __popcll(vote);
        __syncthreads();                                         // one barrier per chunk: the next chunk writes the other half of s_wtot
        int before = base, total = 0;
        for (int w = 0; w < MOSAIC_WAVES; ++w) {
          const int n = s_wtot[par][w];
          if (w < wave) before += n;
          total += n;
        }
        if (keep) {
          const int pos = before + __popcll(vote & ((1ull << lane) - 1ull));
          if (pos < T_out) {
            for (int k = 0; k < 5; ++k) to[(size_t)pos * 5 + k] = o[k];
            ++kept;
          } else {
            ++lost;
          }
        }
        base += total;
      }
    }
    const int first = base < T_out ? base : T_out;
    for (int i = first * 5 + tid; i < T_out * 5; i += MOSAIC_THREADS) to[i] = 0.0f;
  }

  if (kept) atomicAdd(&s_cnt[0], kept);
  if (dropped) atomicAdd(&s_cnt[1], dropped);
  if (lost) atomicAdd(&s_cnt[2], lost);
  __syncthreads();
  if (tid < 3 && s_cnt[tid]) atomicAdd(stats + tid, s_cnt[tid]);
}

bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
  const unsigned long long a0 = (unsigned long long)(size_t)a, b0 = (unsigned long long)(size_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" {

int mdcv_mosaic_batch(const int* desc_host, const int* desc, int B, int C, int H, int W, const float* in, float* out,
                      const float* targets_in, int T, float* targets_out, int T_out, float min_px, float min_visible, int* stats,
                      void* stream) {
  if (!desc_host || !desc || !in || !out || !targets_in || !targets_out || !stats) return MDCV_EARG;
  if (B < 1 || B > MOSAIC_MAX_B || C < 1 || C > 4) return MDCV_EARG;
  if (H < 1 || W < 1 || H > MDCV_MOSAIC_MAX_SIDE || W > MDCV_MOSAIC_MAX_SIDE) return MDCV_EARG;
  if (T < 1 || T_out < 1 || T > MDCV_MOSAIC_MAX_ROWS || T_out > MDCV_MOSAIC_MAX_ROWS) return MDCV_EARG;
  if (!(min_px >= 1.0f) || !(min_visible >= 0.0f && min_visible <= 1.0f)) return MDCV_EARG;
  const unsigned long long pix = (unsigned long long)B * (unsigned long long)C * (unsigned long long)H * (unsigned long long)W * 4ull;
  if (overlap(in, pix, out, pix)) return MDCV_EARG;
  if (overlap(targets_in, (unsigned long long)B * T * 20ull, targets_out, (unsigned long long)B * T_out * 20ull)) return MDCV_EARG;
  for (int b = 0; b < B; ++b)
    if (!mosaic_row_ok(desc_host + (size_t)b * MDCV_MOSAIC_DESC, B, H, W)) return MDCV_EARG;
  const unsigned rows = (unsigned)B * (unsigned)C * (unsigned)H;
  unsigned pix_blocks = (rows + MOSAIC_WAVES - 1) / MOSAIC_WAVES;
  if (pix_blocks > MOSAIC_MAX_PIX_BLOCKS) pix_blocks = MOSAIC_MAX_PIX_BLOCKS;
  hipLaunchKernelGGL(mosaic_kernel, dim3(pix_blocks + (unsigned)B), dim3(MOSAIC_THREADS), 0, (hipStream_t)stream, desc, B, C, H, W, pix_blocks,
                     reinterpret_cast<const unsigned*>(in), reinterpret_cast<unsigned*>(out), targets_in, T, targets_out, T_out, min_px,
                     min_visible, stats);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCV_OK : (int)e;
}

}  // extern "C"
