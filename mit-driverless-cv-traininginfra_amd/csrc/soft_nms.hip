// Soft-NMS detection post-processing on device (include/mdcv_softnms.h states the meaning rule by rule):
//   candidate filter (optionally with the class score) -> top_k keys -> rank sort -> the round loop: pick the largest CURRENT score, emit it,
//   decay (or, hard method, remove) the live boxes that overlap it -> IoU matching against the labels -> AP / R / P per image.
// In a library of its own (libmdcv_softnms.so), built with -ffp-contract=off like postprocess.o; csrc/nms_core.h supplies the key and its
// order, the radix select, the rank sort and the pair arithmetic, unchanged.  The pieces that live inside postprocess.hip and detect_mc.hip
// (the first-maximum class, the label matching, the AP integral) are restated here, each naming the rule it restates.
//
// Stage 1 (grid-wide).  (ceil(N/1024), B) workgroups of 256 threads, four rows a thread, the scheme of the existing filters: rows above
// the confidence threshold are compacted (ballot + prefix) into an LDS list, 16 lanes to a row find the first-maximum class, the template
// flag decides whether the class word enters the score and the second test applies; a second ballot compaction allocates the slots
// wave -> workgroup -> one global atomic per workgroup (counters 128 bytes apart).
//
// Stage 2 (one 1024-thread workgroup per image: radix_select and rank_sort_desc need PB).  After the sort, candidate rank r lives in lane
// r & 63 of wave r >> 6 -- K <= 512, at most 8 waves -- with its box, area, current score and class in registers for the whole loop; the
// sorted boxes and areas stay in LDS, so the winner's box is one broadcast read.  A round:
//   * each owning wave reduces ord32(s) over its lanes in registers (4 DPP steps inside the rows of 16, 4 v_readlane across them), the
//     ballot of the lanes that hold the maximum gives the smallest rank among them, and lane 0 writes the packed word
//     (ord32(s) << 32) | (KMAX - r) to slot[round & 1][wave]; a wave without a live lane writes 0 and skips the arithmetic;
//   * ONE __syncthreads();
//   * every wave reads the 8 slot words (broadcast) and takes their maximum: winner and stop decision are uniform over the workgroup
//     without a second barrier;
//   * the winner's lane notes its rank and current score in LDS (two words) and dies; every other live lane does one nms_pair_iou and one
//     product or death.  No atomics, no global memory traffic: __syncthreads() waits for a wave's outstanding global stores, so a row
//     stored straight from the loop put a memory round trip into every round (measured); the rows go out after the loop.
// All 16 waves run the loop's barrier: the hardware barrier counts every wave of the workgroup, so the 8 waves that own nothing cannot
// wait further down; they read the slots like the others, which costs them nothing the owners wait for.
#include "common.h"
#include "nms_core.h"
#include "../../include/mdcv_softnms.h"

namespace {

constexpr int CNT_STRIDE = 32;     // ints between per-image counters: one 128-byte line each
constexpr int FILTER_ROWS = 1024;  // prediction rows per stage-1 workgroup
constexpr int NO_CLASS = 0x7fffffff;
constexpr unsigned short FAILED = 0xffffu;   // list entry that missed the second test (classes are below MDCV_SNMS_MAX_CLASSES)

__global__ __launch_bounds__(256) void soft_clear_kernel(int* __restrict__ p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

// ---------------------------------------------------------------- stage 1
// exclusive prefix over wave_cnt[4][4] in (r, wave) order -> the total
__device__ __forceinline__ int prefix16(int (*wave_cnt)[4]) {
  int tot = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int c = wave_cnt[r][w]; wave_cnt[r][w] = tot; tot += c; }
  return tot;
}

// CLS = false: mdcv_detect_post's candidates (score = conf; the class is found here, once, for out_cls).
// CLS = true:  mdcv_detect_post_mc's rules 1-3 (score = conf * first-maximum class word, which must pass conf_thres too).
template <bool CLS>
__global__ __launch_bounds__(256) void soft_filter_kernel(const float* __restrict__ pred, int N, int C, float conf_thres,
                                                          unsigned long long* __restrict__ keys, unsigned short* __restrict__ cls16,
                                                          int* __restrict__ cnt) {
  __shared__ unsigned short lrow[FILTER_ROWS];   // the list: row within the workgroup's 1024,
  __shared__ float lval[FILTER_ROWS];            //   its confidence, then its score,
  __shared__ unsigned short lcls[FILTER_ROWS];   //   its class, FAILED when the score missed the second test
  __shared__ int wave_cnt[4][4];
  __shared__ int total, block_base;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_len = 5 + C;
  const int nb0 = blockIdx.x * FILTER_ROWS;
  const float* img = pred + (size_t)b * N * row_len;
  float s[4]; bool pass[4]; unsigned long long m[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = nb0 + tid + r * 256;
    s[r] = n < N ? img[(size_t)n * row_len + 4] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pass[r] = (nb0 + tid + r * 256 < N) && (s[r] > conf_thres);   // NaN does not pass
    m[r] = __ballot(pass[r]);
    if (lane == 0) wave_cnt[r][wave] = __popcll(m[r]);
  }
  __syncthreads();
  if (tid == 0) total = prefix16(wave_cnt);
  __syncthreads();
  const int L = total;
  if (L == 0) return;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (pass[r]) {
      const int e = wave_cnt[r][wave] + __popcll(m[r] & ((1ull << lane) - 1));
      lrow[e] = (unsigned short)(tid + r * 256);
      lval[e] = s[r];
    }
  __syncthreads();

  if (C <= 1) {  // k* = 0: no group walk
    for (int e = tid; e < L; e += 256) {
      unsigned short k = 0;
      if (CLS) {
        const float score = lval[e] * img[(size_t)(nb0 + lrow[e]) * row_len + 5];
        lval[e] = score;
        if (!(score > conf_thres)) k = FAILED;
      }
      lcls[e] = k;
    }
  } else {       // the first maximum as postprocess.hip finds it: 16 lanes to a row, lane q over classes q, q + 16, ..., then its tie rule
    const int q = lane & 15;
    for (int e0 = 0; e0 < L; e0 += 16) {  // 4 waves x 4 rows; uniform trip count, every lane takes part in the shuffles
      const int e = e0 + wave * 4 + (lane >> 4);
      const bool active = e < L;
      const float* r = img + (size_t)(nb0 + (active ? lrow[e] : 0)) * row_len;
      float bv = -__builtin_inff(); int bk = NO_CLASS;
      if (active)
        for (int k = q; k < C; k += 16) { const float v = r[5 + k]; if (v > bv || bk == NO_CLASS) { bv = v; bk = k; } }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int ok = __shfl_xor(bk, o, 64);
        if (ok != NO_CLASS && (bk == NO_CLASS || ov > bv || (ov == bv && ok < bk))) { bv = ov; bk = ok; }
      }
      if (active && q == 0) {
        unsigned short k = (unsigned short)bk;
        if (CLS) {
          const float score = lval[e] * bv;
          lval[e] = score;
          if (!(score > conf_thres)) k = FAILED;
        }
        lcls[e] = k;
      }
    }
  }
  __syncthreads();

  // second compaction: wave -> workgroup -> one global atomic
  bool cand[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = tid + r * 256;
    cand[r] = e < L && lcls[e] != FAILED;
    m[r] = __ballot(cand[r]);
    if (lane == 0) wave_cnt[r][wave] = __popcll(m[r]);
  }
  __syncthreads();
  if (tid == 0) {
    const int tot = prefix16(wave_cnt);
    block_base = tot ? atomicAdd(&cnt[b * CNT_STRIDE], tot) : 0;
  }
  __syncthreads();
  const int base = block_base;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (cand[r]) {
      const int e = tid + r * 256;
      const int n = nb0 + lrow[e];
      keys[(size_t)b * N + base + wave_cnt[r][wave] + __popcll(m[r] & ((1ull << lane) - 1))] = make_key(lval[e], (unsigned)n);
      cls16[(size_t)b * N + n] = lcls[e];
    }
}

// keys for the single-image entry: every box is a candidate.
__global__ __launch_bounds__(256) void soft_keys_kernel(const float* __restrict__ scores, int n, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = make_key(scores[i], (unsigned)i);
  if (i == 0) *cnt = n;
}

// ---------------------------------------------------------------- stage 2
struct SoftArgs {
  const unsigned long long* keys;  // [B][N]
  const int* cnt;                  // [B], CNT_STRIDE apart
  int N, top_k, method, use_cls;
  float nms_thres, sigma, score_thres;
  const float* pred; int row_len;             // batched source
  const unsigned short* cls16;                // [B][N], valid at candidate rows
  const float* boxes; const int* classes;     // single-image source
  const float* targets; int T; float iou_thres, width, height;
  float* out_boxes; float* out_prob; int* out_cls; long long* out_index; unsigned char* out_correct; int* out_count; float* out_stats;
};

__device__ __forceinline__ float ord_score(unsigned o) {  // ord32's inverse
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// maximum of an unsigned over the wave, in registers; every lane of the wave is active.  Inside a row of 16 lanes: quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror (each lane ends with its row's maximum); across the four rows: v_readlane.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  unsigned o;
  o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  v = o > v ? o : v;
  o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  v = o > v ? o : v;
  o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false); v = o > v ? o : v;
  o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false); v = o > v ? o : v;
  const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

// AP / recall / precision of `count` (1..KMAX) detections in emission order: postprocess.hip's ap_integral (utils.py:58-119), operation
// for operation.  Called by every thread of the workgroup; the result is valid on thread 0.
__device__ float4 soft_ap_integral(PostSmem& sm, const float* tp01, int count, int ngt, float* rec, float* pre, float* term) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool t = tid < count && tp01[tid] != 0.f;
  const unsigned long long m = __ballot(t);
  if (lane == 0) sm.wsum[wave] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < PB / 64; ++w) { const int v = sm.wsum[w]; total += v; before += w < wave ? v : 0; }
  const int tpi = before + __popcll(m & ((2ull << lane) - 1ull));
  const float fn = (float)ngt;
  if (tid < count) {
    const float tpc = (float)tpi, fpc = (float)(tid + 1 - tpi);
    rec[tid + 1] = tpc / fn;
    pre[tid + 1] = tpc / (tpc + fpc);
  }
  if (tid == 0) { rec[0] = 0.f; pre[0] = 0.f; rec[count + 1] = 1.f; pre[count + 1] = 0.f; }
  __syncthreads();
  if (tid < KMAX + 64) {
    float v = 0.f;
    if (tid <= count && rec[tid + 1] != rec[tid]) {
      float env = 0.f;
      for (int i = tid + 1; i <= count + 1; ++i) env = fmaxf(env, pre[i]);
      v = (rec[tid + 1] - rec[tid]) * env;
    }
    term[tid] = v;
  }
  __syncthreads();
  float ap = 0.f;
  if (wave == 0) {
    for (int ch = 0; ch * 64 <= count; ++ch) {
      const int v = __float_as_int(term[ch * 64 + lane]);
#pragma unroll
      for (int k = 0; k < 64; ++k) ap += __int_as_float(__builtin_amdgcn_readlane(v, k));
    }
  }
  const float tpc = (float)total, fpc = (float)(count - total);
  return make_float4(ap, tpc / fn, tpc / (tpc + fpc), 1.f);
}

static_assert(sizeof(PostSmem) + 2 * KMAX * 4 + 2 * KW * 8 + 64 <= 64 * 1024, "stage 2 keeps its static LDS under 64 KB");

template <bool BATCHED>
__global__ __launch_bounds__(PB) void soft_image_kernel(SoftArgs A) {
  __shared__ PostSmem sm;
  __shared__ int cl[KMAX];                       // class of sorted candidate t
  __shared__ unsigned long long slot[2][KW];     // the waves' maxima, double-buffered by round parity
  __shared__ float em_score[KMAX];               // current score of the e-th emitted candidate (its rank: sm.keep[e])
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long* keys = A.keys + (size_t)b * A.N;
  int cnt = A.cnt[b * CNT_STRIDE];
  cnt = cnt < 0 ? 0 : (cnt < A.N ? cnt : A.N);
  const int K = cnt < A.top_k ? cnt : A.top_k;

  // ---- candidates -> sm.key[0..K) sorted by descending key (rule 1)
  unsigned long long thresh = 0;
  if (cnt > A.top_k) thresh = radix_select([keys](int i) { return keys[i]; }, cnt, A.top_k, sm);
  if (tid == 0) sm.sel = 0;
  if (tid < 2 * KW) slot[tid / KW][tid % KW] = 0;      // the slots of the waves that own nothing stay 0
  __syncthreads();
  for (int i0 = 0; i0 < cnt; i0 += PB) {
    const int i = i0 + tid;
    unsigned long long k = 0;
    const bool take = i < cnt && (k = keys[i]) >= thresh;
    const unsigned long long m = __ballot(take);
    int base = 0;
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      if (lane == leader) base = atomicAdd(&sm.sel, __popcll(m));
      base = __shfl(base, leader, 64);
      if (take) sm.key[base + __popcll(m & ((1ull << lane) - 1))] = k;
    }
  }
  __syncthreads();
  rank_sort_desc(sm, K);

  // ---- rank tid's box, area, score and class: registers for the loop, box / area / class in LDS for the winner's broadcast
  bool live = tid < K;
  float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
  float ar = 0.f, s = 0.f;
  int c = 0;
  if (live) {
    const unsigned long long key = sm.key[tid];
    const unsigned idx = (unsigned)key;
    s = ord_score((unsigned)(key >> 32));
    if (BATCHED) {
      const float* r = A.pred + ((size_t)b * A.N + idx) * A.row_len;
      const float cx = r[0], cy = r[1], hw = r[2] / 2.f, hh = r[3] / 2.f;
      bx = make_float4(cx - hw, cy - hh, cx + hw, cy + hh);
      c = (int)A.cls16[(size_t)b * A.N + idx];
    } else {
      const float* r = A.boxes + (size_t)idx * 4;
      bx = make_float4(r[0], r[1], r[2], r[3]);
      c = A.classes ? A.classes[idx] : 0;
    }
    ar = (bx.z - bx.x) * (bx.w - bx.y);
    sm.box[tid] = bx; sm.area[tid] = ar; cl[tid] = c;
  }
  __syncthreads();

  // ---- the round loop (rules 2-5)
  const size_t ob = (size_t)b * A.top_k;
  const bool owner_wave = wave * 64 < K;
  const bool soft = A.method != MDCV_SNMS_HARD;
  const double dsigma = (double)A.sigma;
  int round = 0;
  for (;; ++round) {
    if (owner_wave) {
      const unsigned long long lv = __ballot(live);
      unsigned long long word = 0;
      if (lv) {
        const unsigned o = live ? ord32(s) : 0u;
        const unsigned mx = wave_max_u32(o);
        const unsigned long long at = __ballot(live && o == mx);              // never empty: the maximum is a live lane's
        word = ((unsigned long long)mx << 32) | (unsigned)(KMAX - (wave * 64 + (__ffsll((long long)at) - 1)));   // low part 1..KMAX: a live word is not 0
      }
      if (lane == 0) slot[round & 1][wave] = word;
    }
    // The one barrier of the round.  slot[p] written in round t is read by every wave right after this barrier, i.e. before the reader
    // arrives at barrier t + 1; slot[p] is next written in round t + 2, by a wave that has passed barrier t + 1, which opens only when
    // every reader has arrived there.  So no write can overtake a read, and the other parity keeps rounds t and t + 1 apart.
    __syncthreads();
    unsigned long long best = 0;
#pragma unroll
    for (int w = 0; w < KW; ++w) { const unsigned long long v = slot[round & 1][w]; best = v > best ? v : best; }
    if (best == 0) break;                                                     // rule 3: nobody is live
    const float sw = ord_score((unsigned)(best >> 32));
    if (soft && !(sw > A.score_thres)) break;                                 // rule 3
    const int mrank = KMAX - (int)(unsigned)best;
    if (tid == mrank) {                                                       // rule 4: its rank and score, two LDS words; rows go out after the loop
      sm.keep[round] = tid;
      em_score[round] = s;
      live = false;
    }
    if (owner_wave && __ballot(live)) {                                       // rule 5; a wave of dead lanes goes straight to the barrier
      const float4 bm = sm.box[mrank];
      const float am = sm.area[mrank];
      const int cm = cl[mrank];
      if (live && (!A.use_cls || c == cm)) {
        float inter;
        const float iou = nms_pair_iou(bm, am, bx, ar, inter);
        if (A.method == MDCV_SNMS_HARD) {
          live = iou <= A.nms_thres;                                          // survivors are IoU.le(overlap); NaN is removed
        } else if (A.method == MDCV_SNMS_LINEAR) {
          if (iou > A.nms_thres) s = s * (1.0f - iou);
        } else if (iou > 0.f) {
          const float w = (float)exp(-((double)iou * (double)iou) / dsigma);
          s = s * w;
        }
      }
    }
  }
  const int count = round;
  __syncthreads();

  // ---- rule 6: the emitted rows, in emission order; rows past them read as zeros
  if (!BATCHED) {
    const int lim = A.N < A.top_k ? A.N : A.top_k;
    if (tid < lim) {
      A.out_index[tid] = tid < count ? (long long)(unsigned)sm.key[sm.keep[tid]] : 0;
      A.out_prob[tid] = tid < count ? em_score[tid] : 0.f;
    }
    if (tid == 0) A.out_count[0] = count;
    return;
  }

  if (tid < count) {
    const int t = sm.keep[tid];
    *(float4*)(A.out_boxes + (ob + tid) * 4) = sm.box[t];
    A.out_prob[ob + tid] = em_score[tid];
    A.out_cls[ob + tid] = cl[t];
    A.out_index[ob + tid] = (long long)(unsigned)sm.key[t];
  }
  for (int e = count + tid; e < A.top_k; e += PB) {
    *(float4*)(A.out_boxes + (ob + e) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    A.out_prob[ob + e] = 0.f; A.out_cls[ob + e] = 0; A.out_index[ob + e] = 0; A.out_correct[ob + e] = 0;
  }
  if (tid == 0) A.out_count[b] = count;
  if (!A.targets) {
    for (int e = tid; e < count; e += PB) A.out_correct[ob + e] = 0;
    if (tid == 0) { float4 z = make_float4(0.f, 0.f, 0.f, 0.f); *(float4*)(A.out_stats + (size_t)b * 4) = z; }
    return;
  }

  // ---- labels: postprocess.hip's matching (validate.py:105-131), with use_cls detect_mc.hip's rule 8 (labels of the detection's class
  // only); rows with all of (cx,cy,w,h) > 0 are real
  float* best_iou = sm.area;             // reuse: [KMAX]
  int* best_t = (int*)&sm.mask[0][0];    // reuse: [KMAX] ints, then [KMAX] ok flags, recall, precision
  int* okf = best_t + KMAX;
  float* rec = (float*)(okf + KMAX);
  float* pre = rec + KMAX + 2;
  float* term = pre + KMAX + 2;
  const float* tg = A.targets + (size_t)b * A.T * 5;
  if (tid == 0) sm.ngt = 0;
  __syncthreads();
  {
    int local = 0;
    for (int t = tid; t < A.T; t += PB) {
      const float* l = tg + t * 5;
      local += (l[1] > 0.f && l[2] > 0.f && l[3] > 0.f && l[4] > 0.f) ? 1 : 0;
    }
    if (local) atomicAdd(&sm.ngt, local);
  }
  __syncthreads();
  const int ngt = sm.ngt;
  if (count == 0 || ngt == 0) {
    for (int e = tid; e < count; e += PB) A.out_correct[ob + e] = 0;
    if (tid == 0) { float4 z = make_float4(0.f, 0.f, 0.f, 0.f); *(float4*)(A.out_stats + (size_t)b * 4) = z; }
    return;
  }
  float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
  float fk = 0.f;
  if (tid < count) { const int t0 = sm.keep[tid]; d = sm.box[t0]; fk = (float)cl[t0]; }
  __syncthreads();                       // best_iou overlays sm.area, which the winners' reads are done with; sm.box stays
  if (tid < count) {
    const float da = (d.z - d.x + 1.f) * (d.w - d.y + 1.f);
    float bv = -1.f; int bt = -1;
    for (int t = 0; t < A.T; ++t) {
      const float* l = tg + t * 5;
      const float lx = l[1], ly = l[2], lw = l[3], lh = l[4];
      if (!(lx > 0.f && ly > 0.f && lw > 0.f && lh > 0.f) || (A.use_cls && !(l[0] == fk))) continue;
      const float tx1 = (lx - lw / 2.f) * A.width, ty1 = (ly - lh / 2.f) * A.height;
      const float tx2 = (lx + lw / 2.f) * A.width, ty2 = (ly + lh / 2.f) * A.height;
      const float ix1 = fmaxf(d.x, tx1), iy1 = fmaxf(d.y, ty1), ix2 = fminf(d.z, tx2), iy2 = fminf(d.w, ty2);
      const float inter = fmaxf(ix2 - ix1 + 1.f, 0.f) * fmaxf(iy2 - iy1 + 1.f, 0.f);
      const float ta = (tx2 - tx1 + 1.f) * (ty2 - ty1 + 1.f);
      const float iou = inter / (da + ta - inter + 1e-12f);
      if (bt < 0 || iou > bv) { bv = iou; bt = t; }                                       // first maximum
    }
    best_iou[tid] = bv; best_t[tid] = bt; okf[tid] = (bt >= 0 && bv > A.iou_thres) ? 1 : 0;
  }
  __syncthreads();
  if (tid < count) {                     // correct: above the threshold and no earlier such detection claimed the same label
    int ok = okf[tid];
    const int bt = best_t[tid];
    for (int e = 0; ok && e < tid; ++e) ok = !(okf[e] && best_t[e] == bt);
    A.out_correct[ob + tid] = (unsigned char)ok;
    best_iou[tid] = ok ? 1.f : 0.f;      // tp as float for the integral below
  }
  __syncthreads();
  const float4 o = soft_ap_integral(sm, best_iou, count, ngt, rec, pre, term);
  if (tid == 0) *(float4*)(A.out_stats + (size_t)b * 4) = o;
}

}  // namespace

#define SOFT_CHECK_LAUNCH()                                   \
  do {                                                        \
    hipError_t e__ = hipGetLastError();                       \
    if (e__ != hipSuccess) return (int)e__;                   \
  } while (0)

static bool soft_bad_method(int method, float sigma, float score_thres) {
  if (method != MDCV_SNMS_HARD && method != MDCV_SNMS_LINEAR && method != MDCV_SNMS_GAUSSIAN) return true;
  if (method == MDCV_SNMS_GAUSSIAN && !(sigma > 0.f && sigma <= 3.402823466e38f)) return true;   // NaN and +inf fail the comparisons
  return score_thres != score_thres;
}

extern "C" {

// workspace: keys u64[B*N] | cnt int[B * CNT_STRIDE] | cls u16[B*N]
long long mdcv_detect_post_soft_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0) return 0;
  return (long long)B * N * 8 + (long long)B * CNT_STRIDE * 4 + (((long long)B * N * 2 + 15) & ~15LL);
}

int mdcv_detect_post_soft(const float* pred, int B, int N, int C, const float* targets, int T, float conf_thres, float nms_thres,
                          float iou_thres, float width, float height, int top_k, int method, float sigma, float score_thres,
                          int class_aware, float* out_boxes, float* out_prob, int* out_cls, long long* out_index,
                          unsigned char* out_correct, int* out_count, float* out_stats, void* workspace, void* stream) {
  if (!pred || !out_boxes || !out_prob || !out_cls || !out_index || !out_correct || !out_count || !out_stats || !workspace)
    return MDCV_EARG;
  if (B <= 0 || B > 65535 || N <= 0 || C < 0 || C > MDCV_SNMS_MAX_CLASSES || T < 0 || top_k <= 0 || top_k > KMAX ||
      (targets == nullptr && T != 0) || (class_aware != 0 && class_aware != 1) || (class_aware && C < 1) ||
      soft_bad_method(method, sigma, score_thres))
    return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  int* cnt = (int*)(keys + (size_t)B * N);
  unsigned short* cls16 = (unsigned short*)(cnt + (size_t)B * CNT_STRIDE);
  hipLaunchKernelGGL(soft_clear_kernel, dim3((B * CNT_STRIDE + 255) / 256), dim3(256), 0, st, cnt, B * CNT_STRIDE);
  SOFT_CHECK_LAUNCH();
  const dim3 fgrid((N + FILTER_ROWS - 1) / FILTER_ROWS, B);
  if (class_aware) hipLaunchKernelGGL(soft_filter_kernel<true>, fgrid, dim3(256), 0, st, pred, N, C, conf_thres, keys, cls16, cnt);
  else hipLaunchKernelGGL(soft_filter_kernel<false>, fgrid, dim3(256), 0, st, pred, N, C, conf_thres, keys, cls16, cnt);
  SOFT_CHECK_LAUNCH();
  SoftArgs a{};
  a.keys = keys; a.cnt = cnt; a.N = N; a.top_k = top_k; a.method = method; a.use_cls = class_aware;
  a.nms_thres = nms_thres; a.sigma = sigma; a.score_thres = score_thres;
  a.pred = pred; a.row_len = 5 + C; a.cls16 = cls16;
  a.targets = T > 0 ? targets : nullptr; a.T = T; a.iou_thres = iou_thres; a.width = width; a.height = height;
  a.out_boxes = out_boxes; a.out_prob = out_prob; a.out_cls = out_cls; a.out_index = out_index; a.out_correct = out_correct;
  a.out_count = out_count; a.out_stats = out_stats;
  hipLaunchKernelGGL(soft_image_kernel<true>, dim3(B), dim3(PB), 0, st, a);
  SOFT_CHECK_LAUNCH();
  return MDCV_OK;
}

long long mdcv_soft_nms_workspace_bytes(int n) { return n <= 0 ? 128 : (long long)n * 8 + 128; }

int mdcv_soft_nms(const float* boxes, const float* scores, const int* classes, int n, int method, float nms_thres, float sigma,
                  float score_thres, int top_k, long long* keep, float* out_scores, int* count, void* workspace, void* stream) {
  if (n < 0 || top_k <= 0 || top_k > KMAX || !keep || !out_scores || !count || !workspace || (n > 0 && (!boxes || !scores)) ||
      soft_bad_method(method, sigma, score_thres))
    return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipLaunchKernelGGL(soft_clear_kernel, dim3(1), dim3(256), 0, st, count, 1);
    SOFT_CHECK_LAUNCH();
    return MDCV_OK;
  }
  unsigned long long* keys = (unsigned long long*)workspace;
  int* cnt = (int*)(keys + n);
  hipLaunchKernelGGL(soft_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, st, scores, n, keys, cnt);
  SOFT_CHECK_LAUNCH();
  SoftArgs a{};
  a.keys = keys; a.cnt = cnt; a.N = n; a.top_k = top_k; a.method = method; a.use_cls = classes != nullptr;
  a.nms_thres = nms_thres; a.sigma = sigma; a.score_thres = score_thres; a.boxes = boxes; a.classes = classes;
  a.out_index = keep; a.out_prob = out_scores; a.out_count = count;
  hipLaunchKernelGGL(soft_image_kernel<false>, dim3(1), dim3(PB), 0, st, a);
  SOFT_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
