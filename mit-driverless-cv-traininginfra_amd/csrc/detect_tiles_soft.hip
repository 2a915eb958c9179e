// Soft cross-tile merge (include/mdcv_softtiles.h states the meaning rule by rule): the detections of one frame arrive as
// T tiles x K boxes from the tiles' Soft-NMS scans (mdcv_detect_post_soft, one "image" per tile) and leave as one list per frame in
// scaled-frame coordinates.  A box that overlaps a pick of ANOTHER tile decays instead of leaving; the seam rule stays hard.  In a library
// of its own (libmdcv_softtiles.so).  One launch per batch of frames, grid (B), one 1024-thread workgroup per frame, no workspace, the
// counts read on the device only.  Built with -ffp-contract=off like detect_tiles_mc.o; csrc/nms_core.h supplies the key and its order,
// the radix select, the rank sort and the pair arithmetic, unchanged.  Per frame b:
//   0. tiles     detect_tiles.hip's step 0: the device copy of the tile table is searched for the tiles of b and checked again
//   1. keys      its step 1: never stored, recomputed over the n * K <= 32768 slots of the frame (a slot past its tile's count reads as 0)
//   2. select    its step 2: radix select of the top_k largest keys, ballot compaction into LDS, rank sort: rank r = 0..Ksel
//   3. ranks     thread r writes rank r's offset box (the fp64 add, one rounding), area and (local tile, class) to LDS; THE LAST BARRIER of
//                the main path follows: from here on these arrays are read-only
//   4. scan      ONE wave.  Wave 0 takes the up to 512 ranks into registers in the blocked layout -- rank r in lane r >> 3, slot r & 7 -- box,
//                area, current score, tile and class per slot, liveness as eight bits per lane; every loop over the slots is unrolled, no
//                register array is indexed by a variable.  A round:
//                  * lane-local maximum of ord32(s) over the live slots, first maximum = smallest slot (strict >);
//                  * wave maximum in registers: four DPP steps inside the rows of 16 lanes, four v_readlane across them;
//                  * ballot of the lanes that hold it: the first such lane and its slot are the smallest rank among equal maxima, because
//                    the layout is blocked; the rank becomes wave-uniform by one v_readlane;
//                  * the stop test on the uniform score; lane 0 notes (rank, score) in an LDS list; the winner's lane clears its bit;
//                  * the winner's box, area and (tile, class) as broadcast LDS reads;
//                  * the pair arithmetic over the lane's live slots of other tiles (and of the winner's class).
//                No barrier, no atomics and no global memory traffic inside the loop.  The hard method runs the same loop with a fixed
//                visiting order (the smallest live rank: a ballot and a find-first-set) and tests pairs of one tile too, which is the
//                greedy scan of detect_tiles.hip / detect_tiles_mc.hip pair for pair.
//   5. out       waves 1-15 wait at ONE closing barrier and then share the output rows and the zero tail with wave 0: boxes, prob (the
//                score at emission), src, count, cls with class_aware; slots past count: zeros, src (-1, -1), cls 0
// Plain C++, vector stores only.
#include "common.h"
#include "nms_core.h"
#include "../../include/mdcv_softtiles.h"

namespace {

constexpr int MAXT = MDCV_TILE_MAX_PER_FRAME;
constexpr int SLOTS = 8;                       // ranks per lane of the scanning wave
static_assert(KMAX == 64 * SLOTS, "one wave holds every selected candidate, eight to a lane");
enum { TD_FRAME = 0, TD_OFF_X = 1, TD_OFF_Y = 2, TD_ZERO = 3 };

// the same test on the host copy (MDCV_EARG) and on the device copy (count 0): detect_tiles.hip's
__host__ __device__ inline bool tile_offsets_ok(const int* d) {
  return d[TD_OFF_X] >= -MDCV_TILE_MAX_OFFSET && d[TD_OFF_X] <= MDCV_TILE_MAX_OFFSET && d[TD_OFF_Y] >= -MDCV_TILE_MAX_OFFSET &&
         d[TD_OFF_Y] <= MDCV_TILE_MAX_OFFSET && d[TD_ZERO] == 0;
}

// the candidate a selected key names: its low word is ~c.  Every selected key is a candidate's, so c < space; the bound keeps an index
// inside the frame's tiles whatever the key
__device__ __forceinline__ int cand_index(unsigned long long key, int space) {
  const unsigned c = ~(unsigned)key;
  return (int)(c < (unsigned)space ? c : (unsigned)space - 1u);
}

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

struct SoftMergeArgs {
  const float* tile_boxes;  // [T][K][4]
  const float* tile_prob;   // [T][K]
  const int* tile_cls;      // [T][K], read with use_cls only
  const int* tile_count;    // [T]
  const int* tiles;         // [T][MDCV_TILE_DESC], device copy
  int T, K, top_k, use_cls;
  float overlap, contain, sigma, score_thres;
  float* out_boxes; float* out_prob; int* out_cls; int* out_src; int* out_count;
};

// (local tile, class) per rank, the scores at emission (the emitted ranks go to sm.keep), the clamped counts, eight words of scalars
static_assert(sizeof(PostSmem) + KMAX * 8 + KMAX * 4 + MAXT * 4 + 64 <= 64 * 1024, "the merge keeps its static LDS under 64 KB");

template <int METHOD>
__global__ __launch_bounds__(PB) void merge_tiles_soft_kernel(SoftMergeArgs A) {
  __shared__ PostSmem sm;                        // sm.box / sm.area by rank; sm.keep[e] = rank of the e-th emitted candidate
  __shared__ int s_cnt[MAXT];
  __shared__ int2 s_meta[KMAX];                  // (tile within the frame, class) of rank r
  __shared__ float em_score[KMAX];               // score of the e-th emitted candidate at its emission (soft methods)
  __shared__ int s_lo, s_hi, s_n, s_bad, s_total, s_count;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.K;

  // ---- 0. the tiles of this frame
  if (tid == 0) { s_lo = 0x7fffffff; s_hi = -1; s_n = 0; s_bad = 0; s_total = 0; s_count = 0; sm.sel = 0; }
  __syncthreads();
  for (int t = tid; t < A.T; t += PB) {
    const int* d = A.tiles + (size_t)t * MDCV_TILE_DESC;
    if (d[TD_FRAME] == b) {
      atomicMin(&s_lo, t); atomicMax(&s_hi, t); atomicAdd(&s_n, 1);
      if (!tile_offsets_ok(d)) atomicOr(&s_bad, 1);
    }
  }
  __syncthreads();
  const int n = s_n, t0 = n > 0 ? s_lo : 0;
  const bool ok = n > 0 && n <= MAXT && !s_bad && s_hi - t0 + 1 == n;
  if (ok)
    for (int lt = tid; lt < n; lt += PB) {
      int c = A.tile_count[t0 + lt];
      c = c < 0 ? 0 : (c > K ? K : c);
      s_cnt[lt] = c;
      if (c) atomicAdd(&s_total, c);
    }
  __syncthreads();
  const int cnt = ok ? s_total : 0;            // candidates of the frame
  const int space = ok ? n * K : 0;            // their index space: <= MAXT * KMAX
  const int Ksel = cnt < A.top_k ? cnt : A.top_k;

  // ---- 1, 2. keys -> sm.key[0..Ksel) sorted by descending key
  const float* prob = A.tile_prob + (size_t)t0 * K;
  const int* cntp = s_cnt;
  auto key_at = [prob, cntp, K](int i) -> unsigned long long {
    const int lt = i / K, k = i - lt * K;
    return k < cntp[lt] ? make_key(prob[i], ~(unsigned)i) : 0ull;
  };
  unsigned long long thresh = 0;
  if (cnt > A.top_k) thresh = radix_select(key_at, space, A.top_k, sm);
  for (int i0 = 0; i0 < space; i0 += PB) {
    const int i = i0 + tid;
    unsigned long long k = 0;
    const bool take = i < space && (k = key_at(i)) != 0ull && k >= thresh;
    const unsigned long long m = __ballot(take);
    int base = 0;
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      if (lane == leader) base = atomicAdd(&sm.sel, __popcll(m));
      base = __shfl(base, leader, 64);
      const int at = base + __popcll(m & ((1ull << lane) - 1));
      if (take && at < KMAX) sm.key[at] = k;   // exactly Ksel keys pass (they are distinct); the bound is belt and braces
    }
  }
  __syncthreads();
  rank_sort_desc(sm, Ksel);

  // ---- 3. rank tid's merged box, area, tile and class
  if (tid < Ksel) {
    const int i = cand_index(sm.key[tid], space);
    const int lt = i / K;
    const int* d = A.tiles + (size_t)(t0 + lt) * MDCV_TILE_DESC;
    const double ox = (double)d[TD_OFF_X], oy = (double)d[TD_OFF_Y];
    const float* r = A.tile_boxes + ((size_t)t0 * K + i) * 4;
    const float4 bx = make_float4((float)((double)r[0] + ox), (float)((double)r[1] + oy), (float)((double)r[2] + ox), (float)((double)r[3] + oy));
    sm.box[tid] = bx;
    sm.area[tid] = (bx.z - bx.x) * (bx.w - bx.y);  // nms.py:24
    s_meta[tid] = make_int2(lt, A.use_cls ? A.tile_cls[(size_t)t0 * K + i] : 0);
  }
  __syncthreads();   // the last barrier of the main path: sm.key / box / area and s_meta are read-only from here on

  // ---- 4. the scan, wave 0 alone
  if (wave == 0) {
    float4 bx[SLOTS];
    float ar[SLOTS], sc[SLOTS];
    int tl[SLOTS], cs[SLOTS];
    unsigned livem = 0;                          // bit k: slot k (rank 8 * lane + k) is live
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int r = lane * SLOTS + k;
      const bool in = r < Ksel;
      const int rr = in ? r : 0;
      const int2 mt = s_meta[rr];
      bx[k] = sm.box[rr]; ar[k] = sm.area[rr]; sc[k] = ord_score((unsigned)(sm.key[rr] >> 32)); tl[k] = mt.x; cs[k] = mt.y;
      livem |= in ? (1u << k) : 0u;
    }
    const bool seam = A.contain >= 0.f;
    const bool use_cls = A.use_cls != 0;
    const double dsigma = (double)A.sigma;
    int round = 0;
    while (round < KMAX) {                       // a round emits one candidate, so at most Ksel rounds run; the bound is the lists'
      int wl, wk;
      float sw = 0.f;
      if (METHOD == MDCV_SNMS_HARD) {            // rule 4: the smallest live rank
        const unsigned long long at = __ballot(livem != 0u);
        if (!at) break;
        wl = __ffsll((long long)at) - 1;
        wk = __builtin_amdgcn_readlane(__ffs((int)livem) - 1, wl);
      } else {                                   // rule 2: the largest ord32(s), equal ones by rank
        unsigned lm = 0u;
        int lk = 0;
        bool have = false;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) {
          const unsigned o = ord32(sc[k]);
          const bool better = ((livem >> k) & 1u) && (!have || o > lm);
          lm = better ? o : lm; lk = better ? k : lk; have = have || better;
        }
        if (!__ballot(have)) break;              // nobody is live
        const unsigned mx = wave_max_u32(have ? lm : 0u);
        const unsigned long long at = __ballot(have && lm == mx);      // never empty: the maximum is a live slot's
        wl = __ffsll((long long)at) - 1;
        wk = __builtin_amdgcn_readlane(lk, wl);
        sw = ord_score(mx);
        if (!(sw > A.score_thres)) break;
      }
      const int m = wl * SLOTS + wk;             // wave-uniform
      if (lane == 0) { sm.keep[round] = m; em_score[round] = sw; }     // rows go out after the loop
      if (lane == wl) livem &= ~(1u << wk);
      ++round;
      const float4 bm = sm.box[m];
      const float am = sm.area[m];
      const int2 mm = s_meta[m];
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        bool pair = ((livem >> k) & 1u) && (!use_cls || cs[k] == mm.y);
        if (METHOD != MDCV_SNMS_HARD) pair = pair && tl[k] != mm.x;    // rule 3: a tile's own pairs are its own scan's
        if (!pair) continue;
        float inter;
        const float iou = nms_pair_iou(bm, am, bx[k], ar[k], inter);
        const float mn = ar[k] < am ? ar[k] : am;
        if (METHOD == MDCV_SNMS_HARD) {
          bool rem = !(iou <= A.overlap);                              // survivors are IoU.le(overlap); NaN is removed
          if (seam && tl[k] != mm.x) rem = rem || !(inter / mn <= A.contain);
          if (rem) livem &= ~(1u << k);
        } else if (!(inter == 0.f) || (seam && !(mn < 0.f || mn > 0.f))) {
          // (a zero intersection with a non-zero smaller area changes nothing: the ratio is +-0 <= contain_thres, the IoU +-0 or NaN, and
          // s * (1.0f - +-0) is s; the divisions are skipped where no lane of the wave needs them)
          if (seam && !(inter / mn <= A.contain)) {
            livem &= ~(1u << k);                                       // the seam rule, hard in every method; a NaN ratio leaves
          } else if (METHOD == MDCV_SNMS_LINEAR) {
            if (iou > A.overlap) sc[k] = sc[k] * (1.0f - iou);
          } else if (iou > 0.f) {
            const float w = (float)exp(-((double)iou * (double)iou) / dsigma);
            sc[k] = sc[k] * w;
          }
        }
      }
    }
    if (lane == 0) s_count = round;
  }
  __syncthreads();   // the closing barrier: waves 1-15 have waited here

  // ---- 5. out: every slot of the frame is written
  const int count = s_count;
  const size_t ob = (size_t)b * A.top_k;
  for (int c = tid; c < A.top_k; c += PB) {
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float p = 0.f;
    int st = -1, sk = -1, ck = 0;
    if (c < count) {
      const int t = sm.keep[c];
      const int i = cand_index(sm.key[t], space);
      const int lt = i / K;
      bx = sm.box[t]; p = METHOD == MDCV_SNMS_HARD ? prob[i] : em_score[c]; ck = s_meta[t].y; st = t0 + lt; sk = i - lt * K;
    }
    float* o = A.out_boxes + (ob + c) * 4;
    o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w;
    A.out_prob[ob + c] = p;
    if (A.use_cls) A.out_cls[ob + c] = ck;
    A.out_src[(ob + c) * 2] = st; A.out_src[(ob + c) * 2 + 1] = sk;
  }
  if (tid == 0) A.out_count[b] = count;
}

}  // namespace

extern "C" {

int mdcv_detect_merge_tiles_soft(const float* tile_boxes, const float* tile_prob, const int* tile_cls, const int* tile_count,
                                 const int* tiles_host, const int* tiles, int T, int K, int B, float overlap, float contain_thres,
                                 int top_k, float* out_boxes, float* out_prob, int* out_cls, int* out_src, int* out_count, int method,
                                 float sigma, float score_thres, int class_aware, void* stream) {
  if (B < 0 || T < 0 || K < 0 || B > 65535 || K > KMAX || top_k <= 0 || top_k > KMAX) return MDCV_EARG;
  if (method != MDCV_SNMS_HARD && method != MDCV_SNMS_LINEAR && method != MDCV_SNMS_GAUSSIAN) return MDCV_EARG;
  if (method == MDCV_SNMS_GAUSSIAN && !(sigma > 0.f && sigma <= 3.402823466e38f)) return MDCV_EARG;   // NaN and +inf fail the comparisons
  if (score_thres != score_thres || (class_aware != 0 && class_aware != 1)) return MDCV_EARG;
  if (T > 0 && !tiles_host) return MDCV_EARG;
  int prev = 0, run = 0;
  for (int t = 0; t < T; ++t) {                     // the host copy: frames in range and ascending, tiles of a frame contiguous, limits
    const int* d = tiles_host + (size_t)t * MDCV_TILE_DESC;
    const int f = d[TD_FRAME];
    if (f < 0 || f >= B || f < prev || !tile_offsets_ok(d)) return MDCV_EARG;
    run = (t > 0 && f == prev) ? run + 1 : 1;
    if (run > MAXT) return MDCV_EARG;
    prev = f;
  }
  if (B == 0 || T == 0 || K == 0) return MDCV_OK;   // nothing to merge: nothing is enqueued or written
  if (!tile_boxes || !tile_prob || !tile_count || !tiles || !out_boxes || !out_prob || !out_src || !out_count) return MDCV_EARG;
  if (class_aware && (!tile_cls || !out_cls)) return MDCV_EARG;
  SoftMergeArgs a{tile_boxes, tile_prob, tile_cls, tile_count, tiles, T, K, top_k, class_aware, overlap, contain_thres, sigma, score_thres,
                  out_boxes, out_prob, out_cls, out_src, out_count};
  const dim3 grid((unsigned)B), block(PB);
  if (method == MDCV_SNMS_HARD) hipLaunchKernelGGL(merge_tiles_soft_kernel<MDCV_SNMS_HARD>, grid, block, 0, (hipStream_t)stream, a);
  else if (method == MDCV_SNMS_LINEAR) hipLaunchKernelGGL(merge_tiles_soft_kernel<MDCV_SNMS_LINEAR>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(merge_tiles_soft_kernel<MDCV_SNMS_GAUSSIAN>, grid, block, 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCV_OK : (int)e;
}

}  // extern "C"
