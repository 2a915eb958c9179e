// Class-aware tile-and-scale inference, the join (include/mdcv_mctiles.h states the meaning rule by rule): the detections
// of one frame arrive as T tiles x K boxes WITH A CLASS EACH (mdcv_detect_post_mc's outputs, one "image" per tile) and leave as one list per
// frame in scaled-frame coordinates, the duplicates of overlapping tiles removed class by class.  The multi-class counterpart of
// csrc/detect_tiles.hip, in a library of its own (libmdcv_mctiles.so).  One launch per batch of frames, grid (B), one 1024-thread
// workgroup per frame, no workspace, the counts read on the device only.  Built with -ffp-contract=off like detect_tiles.o; csrc/nms_core.h
// supplies the key and its order, the radix select, the rank sort and the pair arithmetic, unchanged.  Per frame b:
//   0. tiles     detect_tiles.hip's step 0: the device copy of the tile table is searched for the tiles of b and checked again
//   1. keys      its step 1: never stored, recomputed over the n * K <= 32768 slots of the frame (a slot past its tile's count reads as 0)
//   2. select    its step 2: radix select of the top_k largest keys, ballot compaction into LDS, rank sort: the visiting order t = 0..Ksel
//   3. classes   cl[t] = tile_cls of the selected candidate; only those words are read
//   4. regroup   a second rank sort on (class, t): position p = pos[t] in SEGMENT order, one contiguous segment per class present, each in
//                visiting order; segment heads by comparing neighbours, numbered by ballot + prefix
//   5. boxes     detect_tiles.hip's step 3 (the fp64 offset add, one rounding; area as nms.py:24), but box, area and tile byte are WRITTEN at
//                p, not at t: the rows the matrix loop reads are then contiguous in LDS and nothing is gathered a second time
//   6. matrix    bit j of row p (j > p, same segment): j leaves once p is kept -- !(IoU <= overlap), or, for candidates of different tiles
//                and contain_thres >= 0, !(inter / min(area_j, area_p) <= contain_thres).  A block-diagonal matrix in the 32 KB `mask`:
//                pair work sum(L^2 / 2) over the segments instead of Ksel^2 / 2
//   7. scan      the segments are dealt to the 16 waves; each wave resolves its segments with the register-resident 64-candidate word walk
//                of nms_scan.inc -- a segment may start and end inside a word, so the bits in front of and past it are preset as removed;
//                a one-candidate segment is kept without a walk; kept bits are OR-ed into eight LDS words
//   8. out       kept bits back to visiting order through pos, compacted by ballot; boxes, prob, cls, src, count; slots past count:
//                zeros, src (-1, -1), cls 0
// Plain C++, vector stores only.
#include "common.h"
#include "nms_core.h"
#include "../../include/mdcv_mctiles.h"

namespace {

constexpr int MAXT = MDCV_TILE_MAX_PER_FRAME;
static_assert(MAXT <= 256, "the tile of a candidate is kept in one byte");
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

struct McMergeArgs {
  const float* tile_boxes;  // [T][K][4]
  const float* tile_prob;   // [T][K]
  const int* tile_cls;      // [T][K]
  const int* tile_count;    // [T]
  const int* tiles;         // [T][MDCV_TILE_DESC], device copy
  int T, K, top_k;
  float overlap, contain;
  float* out_boxes; float* out_prob; int* out_cls; int* out_src; int* out_count;
};

// the classes, the two permutations between visiting order and segment order, the segment table and the kept bits; the clamped counts
// and the tile bytes; eight words of scalars
constexpr int MC_EXTRA_LDS = KMAX * 4 + 3 * KMAX * 2 + (KMAX + 2) * 2 + KW * 8;
constexpr int TILE_EXTRA_LDS = MAXT * 4 + KMAX;
static_assert(sizeof(PostSmem) + MC_EXTRA_LDS + TILE_EXTRA_LDS + 64 <= 64 * 1024, "the merge keeps its static LDS under 64 KB");

__global__ __launch_bounds__(PB) void merge_tiles_mc_kernel(McMergeArgs A) {
  __shared__ PostSmem sm;                        // sm.box / sm.area are in SEGMENT order here (step 5)
  __shared__ int s_cnt[MAXT];
  __shared__ unsigned char s_tile[KMAX];         // tile (within the frame) of position p
  __shared__ int cl[KMAX];                       // class of sorted candidate t
  __shared__ unsigned short perm[KMAX];          // segment order -> visiting order
  __shared__ unsigned short pos[KMAX];           // visiting order -> segment order
  __shared__ unsigned short segid[KMAX];         // segment of position p
  __shared__ unsigned short segstart[KMAX + 2];  // first position of segment s; segstart[nseg] = Ksel
  __shared__ unsigned long long keptw[KW];       // kept bits in segment order
  __shared__ int s_lo, s_hi, s_n, s_bad, s_total;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.K;

  // ---- 0. the tiles of this frame
  if (tid == 0) { s_lo = 0x7fffffff; s_hi = -1; s_n = 0; s_bad = 0; s_total = 0; sm.sel = 0; }
  if (tid < KW) keptw[tid] = 0;
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

  // ---- 3. classes of the selected candidates
  for (int t = tid; t < Ksel; t += PB) cl[t] = A.tile_cls[(size_t)t0 * K + cand_index(sm.key[t], space)];
  __syncthreads();

  // ---- 4. rank sort on (class, t): one contiguous segment per class present, each in visiting order.  Two threads per candidate.
  {
    const int i = tid & (KMAX - 1), h = tid / KMAX;
    const int half = (Ksel + 1) >> 1;
    int rank = 0;
    if (i < Ksel) {
      const int ci = cl[i];
      const int j0 = h * half, j1 = (j0 + half) < Ksel ? (j0 + half) : Ksel;
#pragma unroll 8
      for (int j = j0; j < j1; ++j) { const int cj = cl[j]; rank += (cj < ci || (cj == ci && j < i)) ? 1 : 0; }
    }
    if (h == 1 && i < Ksel) sm.keep[i] = rank;
    __syncthreads();
    if (h == 0 && i < Ksel) { rank += sm.keep[i]; perm[rank] = (unsigned short)i; pos[i] = (unsigned short)rank; }
    __syncthreads();
  }
  int nseg;
  {
    const bool head = tid < Ksel && (tid == 0 || cl[perm[tid]] != cl[perm[tid - 1]]);
    const unsigned long long m = __ballot(head);
    if (lane == 0) sm.wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < PB / 64; ++w) { const int v = sm.wsum[w]; total += v; before += w < wave ? v : 0; }
    const int sid = before + __popcll(m & ((2ull << lane) - 1ull)) - 1;
    if (tid < Ksel) segid[tid] = (unsigned short)sid;
    if (head) segstart[sid] = (unsigned short)tid;
    if (tid == 0) segstart[total] = (unsigned short)Ksel;
    nseg = total;
  }

  // ---- 5. merged boxes, written in segment order
  for (int t = tid; t < Ksel; t += PB) {
    const int i = cand_index(sm.key[t], space);
    const int lt = i / K, p = pos[t];
    const int* d = A.tiles + (size_t)(t0 + lt) * MDCV_TILE_DESC;
    const double ox = (double)d[TD_OFF_X], oy = (double)d[TD_OFF_Y];
    const float* r = A.tile_boxes + ((size_t)t0 * K + i) * 4;
    const float4 bx = make_float4((float)((double)r[0] + ox), (float)((double)r[1] + oy), (float)((double)r[2] + ox), (float)((double)r[3] + oy));
    sm.box[p] = bx;
    sm.area[p] = (bx.z - bx.x) * (bx.w - bx.y);  // nms.py:24
    s_tile[p] = (unsigned char)lt;
  }
  __syncthreads();

  // ---- 6. suppression bits inside segments only (rule 4)
  const bool seam = A.contain >= 0.f;
  for (int p = wave; p < Ksel; p += PB / 64) {
    const int end = segstart[segid[p] + 1];
    const float4 bi = sm.box[p];
    const float ai = sm.area[p];
    const int ti = s_tile[p];
    for (int w = p >> 6; w * 64 < end; ++w) {
      const int j = w * 64 + lane;
      bool rem = false;
      if (j > p && j < end) {
        const float aj = sm.area[j];
        float inter;
        const float iou = nms_pair_iou(bi, ai, sm.box[j], aj, inter);
        rem = !(iou <= A.overlap);                  // survivors are IoU.le(overlap); NaN is removed
        if (seam && s_tile[j] != ti) rem = rem || !(inter / (aj < ai ? aj : ai) <= A.contain);
      }
      const unsigned long long m = __ballot(rem);
      if (lane == 0) sm.mask[p][w] = m;
    }
  }
  __syncthreads();

  // ---- 7. greedy scan, one wave per segment.  Lane w owns word w of the removed set; each 64-position word is resolved in registers: lane l
  // holds row (64w + l)'s bits for this word, the walk over the 64 bits is scalar (v_readlane).  Positions of the word outside the segment
  // are preset as removed, so they are neither kept nor do their (unwritten) rows contribute.
  for (int s = wave; s < nseg; s += PB / 64) {
    const int s0 = __builtin_amdgcn_readfirstlane((int)segstart[s]), s1 = __builtin_amdgcn_readfirstlane((int)segstart[s + 1]);
    if (s1 - s0 == 1) {                                 // a class with one candidate: kept
      if (lane == 0) atomicOr(&keptw[s0 >> 6], 1ull << (s0 & 63));
      continue;
    }
    const int w1 = (s1 - 1) >> 6;
    unsigned long long removed = 0;
    for (int w = s0 >> 6; w <= w1; ++w) {
      const int il = w * 64 + lane;
      const unsigned long long diag = (il >= s0 && il < s1) ? sm.mask[il][w] : 0ull;
      const int dlo = (int)(unsigned)diag, dhi = (int)(unsigned)(diag >> 32);
      unsigned long long cur = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(removed >> 32), w) << 32) |
                               (unsigned)__builtin_amdgcn_readlane((int)(unsigned)removed, w);
      const int lo = s0 - w * 64, nb = s1 - w * 64;
      if (lo > 0) cur |= (1ull << lo) - 1ull;           // before the segment (lo <= 63: w >= s0 / 64)
      if (nb < 64) cur |= ~0ull << nb;                  // past it
      unsigned long long kept = 0;
#pragma unroll
      for (int t = 0; t < 64; ++t) {
        const unsigned long long row = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, t) << 32) | (unsigned)__builtin_amdgcn_readlane(dlo, t);
        const unsigned long long alive = ((cur >> t) & 1ull) - 1ull;  // all ones while position t has not been removed
        kept |= (1ull << t) & alive;
        cur |= row & alive;
      }
      if (lane == 0) atomicOr(&keptw[w], kept);         // segments of other waves may share the word
      if (w < w1 && lane > w && lane <= w1) {           // rows of the kept positions -> later words of the segment
#pragma unroll
        for (int t = 0; t < 64; ++t) removed |= sm.mask[w * 64 + t][lane] & (0ull - ((kept >> t) & 1ull));
      }
    }
  }
  __syncthreads();

  // ---- 8. kept bits back to visiting order, compacted into sm.keep; every slot of the frame is written
  int count;
  {
    bool k = false;
    if (tid < Ksel) { const int p = pos[tid]; k = (keptw[p >> 6] >> (p & 63)) & 1ull; }
    const unsigned long long m = __ballot(k);
    if (lane == 0) sm.wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < PB / 64; ++w) { const int v = sm.wsum[w]; total += v; before += w < wave ? v : 0; }
    if (k) sm.keep[before + __popcll(m & ((1ull << lane) - 1))] = tid;
    count = total;
    __syncthreads();
  }
  const size_t ob = (size_t)b * A.top_k;
  for (int c = tid; c < A.top_k; c += PB) {
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float p = 0.f;
    int st = -1, sk = -1, ck = 0;
    if (c < count) {
      const int t = sm.keep[c];
      const int i = cand_index(sm.key[t], space);
      const int lt = i / K;
      bx = sm.box[pos[t]]; p = prob[i]; ck = cl[t]; st = t0 + lt; sk = i - lt * K;
    }
    float* o = A.out_boxes + (ob + c) * 4;
    o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w;
    A.out_prob[ob + c] = p;
    A.out_cls[ob + c] = ck;
    A.out_src[(ob + c) * 2] = st; A.out_src[(ob + c) * 2 + 1] = sk;
  }
  if (tid == 0) A.out_count[b] = count;
}

}  // namespace

extern "C" {

int mdcv_detect_merge_tiles_mc(const float* tile_boxes, const float* tile_prob, const int* tile_cls, const int* tile_count,
                               const int* tiles_host, const int* tiles, int T, int K, int B, float overlap, float contain_thres,
                               int top_k, float* out_boxes, float* out_prob, int* out_cls, int* out_src, int* out_count, void* stream) {
  if (B < 0 || T < 0 || K < 0 || B > 65535 || K > KMAX || top_k <= 0 || top_k > KMAX) return MDCV_EARG;
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
  if (!tile_boxes || !tile_prob || !tile_cls || !tile_count || !tiles || !out_boxes || !out_prob || !out_cls || !out_src || !out_count)
    return MDCV_EARG;
  McMergeArgs a{tile_boxes, tile_prob, tile_cls, tile_count, tiles, T, K, top_k, overlap, contain_thres,
                out_boxes, out_prob, out_cls, out_src, out_count};
  hipLaunchKernelGGL(merge_tiles_mc_kernel, dim3((unsigned)B), dim3(PB), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCV_OK : (int)e;
}

}  // extern "C"
