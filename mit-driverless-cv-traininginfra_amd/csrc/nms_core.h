// The pieces of the greedy NMS (utils/nms.py:4-61) that more than one kernel runs: csrc/postprocess.hip (mdcv_nms, mdcv_detect_post) and
// csrc/detect_tiles.hip (mdcv_detect_merge_tiles).  One definition each, so that the kernels cannot drift apart: the candidate key and its
// order, the radix select of the top_k keys, the LDS rank sort and the fp32 arithmetic of one pair (nms.py:44-59).  Every unit that
// includes this is built with -ffp-contract=off: each fp32 operation rounds on its own, as the reference's torch operations do.
// Workgroups are PB = 1024 threads (16 waves), one per image / frame.  The single-wave greedy scan over the suppression matrix is shared as
// text, nms_scan.inc (why: there).
#pragma once
#include "common.h"

#ifndef MDCV_NMS_MAX_TOPK
#define MDCV_NMS_MAX_TOPK 512
#endif

namespace {

constexpr int KMAX = MDCV_NMS_MAX_TOPK;
constexpr int KW = KMAX / 64;
constexpr int PB = 1024;  // threads per image workgroup
static_assert(PB == 2 * KMAX, "rank_sort_desc uses two threads per key");

__device__ __forceinline__ unsigned ord32(float f) {  // monotone float -> uint (NaN with sign 0 sorts highest)
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long make_key(float score, unsigned idx) { return ((unsigned long long)ord32(score) << 32) | idx; }

struct PostSmem {
  unsigned long long key[KMAX];
  float4 box[KMAX];
  float area[KMAX];
  unsigned long long mask[KMAX][KW];
  unsigned hist[256];
  int keep[KMAX];
  unsigned long long thresh;
  int need, sel, count, ngt, done;
  int wsum[PB / 64];
};

// top_k-th largest key of key_at(0..cnt) (all keys distinct): MSB-first radix select, 8 bits a pass.
// Returns a threshold t such that exactly `top_k` keys are >= t.
template <class KeyAt>
__device__ unsigned long long radix_select(KeyAt key_at, int cnt, int top_k, PostSmem& sm) {
  const int tid = threadIdx.x;
  if (tid == 0) { sm.thresh = 0; sm.need = top_k; sm.done = 0; }
  for (int p = 7; p >= 0; --p) {
    if (tid < 256) sm.hist[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = sm.thresh;
    const int sh = 8 * p;
    for (int i = tid; i < cnt; i += PB) {
      const unsigned long long k = key_at(i);
      const bool match = (p == 7) || ((k >> (sh + 8)) == (prefix >> (sh + 8)));
      if (match) atomicAdd(&sm.hist[(unsigned)(k >> sh) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: suffix scan over 256 bins, 4 per lane, highest bins in the highest lane
      const unsigned h0 = sm.hist[4 * tid], h1 = sm.hist[4 * tid + 1], h2 = sm.hist[4 * tid + 2], h3 = sm.hist[4 * tid + 3];
      const unsigned s = h0 + h1 + h2 + h3;
      unsigned incl = s;  // inclusive suffix sum over lanes >= tid
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_down(incl, o, 64);
        if (tid + o < 64) incl += v;
      }
      const unsigned above = incl - s;
      const unsigned need = (unsigned)sm.need;
      if (above < need && need <= incl) {
        unsigned a = above; int d; unsigned hd;
        if (a + h3 >= need) { d = 3; hd = h3; }
        else { a += h3; if (a + h2 >= need) { d = 2; hd = h2; } else { a += h2; if (a + h1 >= need) { d = 1; hd = h1; } else { a += h1; d = 0; hd = h0; } } }
        sm.thresh = prefix | ((unsigned long long)(4 * tid + d) << sh);
        sm.need = (int)(need - a);
        sm.done = (hd == need - a);  // the whole bin is taken: lower bits of the threshold stay 0
      }
    }
    __syncthreads();
    if (sm.done) break;
  }
  return sm.thresh;
}

// descending sort of the distinct keys sm.key[0..K), K <= KMAX: rank = number of larger keys.  Two threads per key,
// each counting over half of the others (the inner read is a wave-wide LDS broadcast).
__device__ void rank_sort_desc(PostSmem& sm, int K) {
  const int i = threadIdx.x & (KMAX - 1), h = threadIdx.x / KMAX;  // PB == 2 * KMAX
  const int half = (K + 1) >> 1;
  unsigned long long mine = 0;
  int rank = 0;
  if (i < K) {
    mine = sm.key[i];
    const int j0 = h * half, j1 = (j0 + half) < K ? (j0 + half) : K;
#pragma unroll 8
    for (int j = j0; j < j1; ++j) rank += sm.key[j] > mine ? 1 : 0;
  }
  if (h == 1 && i < K) sm.keep[i] = rank;
  __syncthreads();
  if (h == 0 && i < K) rank += sm.keep[i];
  __syncthreads();
  if (h == 0 && i < K) sm.key[rank] = mine;
  __syncthreads();
}

// one pair of the scan: the kept box bi (area ai) against a remaining box bj (area aj) -> IoU as nms.py:44-59 computes it in fp32,
// each operation rounded on its own; `inter` is the intersection area it divides
__device__ __forceinline__ float nms_pair_iou(const float4 bi, const float ai, const float4 bj, const float aj, float& inter) {
  const float xx1 = fmaxf(bj.x, bi.x), yy1 = fmaxf(bj.y, bi.y), xx2 = fminf(bj.z, bi.z), yy2 = fminf(bj.w, bi.w);
  const float ww = fmaxf(xx2 - xx1, 0.f), hh = fmaxf(yy2 - yy1, 0.f);
  inter = ww * hh;
  const float uni = (aj - inter) + ai;  // nms.py:56
  return inter / uni;
}

}  // namespace
