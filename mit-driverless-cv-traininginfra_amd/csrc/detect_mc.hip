// Class-aware detection post-processing on device (include/mdcv_mcdet.h states the meaning rule by rule):
//   objectness filter -> first-maximum class -> score = conf * class word -> second filter -> top_k keys -> greedy NMS class by class
//   -> IoU matching against the labels of the detection's own class -> AP / R / P per image.
// The multi-class counterpart of csrc/postprocess.hip, in a library of its own (libmdcv_mcdet.so).  Built with -ffp-contract=off like
// postprocess.o; csrc/nms_core.h supplies the key and its order, the radix select, the rank sort and the pair arithmetic, unchanged.
//
// Stage 1 (grid-wide).  (ceil(N/1024), B) workgroups of 256 threads, four rows a thread.  The confidence column is read for every row;
// the rows above the threshold are compacted (ballot + prefix) into an LDS list, and only those rows' class words are read: the four
// waves walk the list 16 lanes to a row, lane q reading classes q, q + 16, ... (coalesced 64-byte pieces of the row), the first maximum
// falls out of a 16-lane shuffle reduction with postprocess.hip's tie rule, lane 0 of the group forms the score and applies the second
// test.  Scores and classes go back into the LDS list; a second ballot compaction allocates the slots wave -> workgroup -> one global
// atomic per workgroup (counters 128 bytes apart) and writes the key list and the row's class (16 bits, at candidate rows only).
//
// Stage 2 (one 1024-thread workgroup per image).  Radix select, compaction, rank sort, boxes and areas as in postprocess.hip.  Then the
// class-segmented scan: a second rank sort on (class, position) regroups the K <= 512 sorted candidates into one contiguous segment
// per class present, each in score order.  The suppression bits are built inside segments only (a block-diagonal matrix in the same 32 KB
// `mask`), the segments are dealt to the 16 waves, and each wave resolves its segments with the register-resident 64-candidate word walk
// (v_readlane) -- a segment may start and end inside a word, so the bits outside it are preset as removed.  The kept bits are mapped back
// to score order and compacted by ballot into `keep`; output and label matching follow.
#include "common.h"
#include "nms_core.h"
#include "../../include/mdcv_mcdet.h"

namespace {

constexpr int CNT_STRIDE = 32;     // ints between per-image counters: one 128-byte line each
constexpr int FILTER_ROWS = 1024;  // prediction rows per stage-1 workgroup
constexpr int NO_CLASS = 0x7fffffff;
constexpr unsigned short FAILED = 0xffffu;   // list entry that missed the second test (classes are below MDCV_MCDET_MAX_CLASSES)

__global__ __launch_bounds__(256) void mc_clear_kernel(int* __restrict__ p, int n) {
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

__global__ __launch_bounds__(256) void mc_filter_kernel(const float* __restrict__ pred, int N, int C, float conf_thres,
                                                        unsigned long long* __restrict__ keys, unsigned short* __restrict__ cls16,
                                                        int* __restrict__ cnt) {
  __shared__ unsigned short lrow[FILTER_ROWS];   // the list: row within the workgroup's 1024,
  __shared__ float lval[FILTER_ROWS];            //   its confidence, then its score,
  __shared__ unsigned short lcls[FILTER_ROWS];   //   its class, FAILED when score <= conf_thres
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
    pass[r] = (nb0 + tid + r * 256 < N) && (s[r] > conf_thres);   // rule 3, first test (NaN does not pass)
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

  if (C == 1) {  // k* = 0: no group walk
    for (int e = tid; e < L; e += 256) {
      const float score = lval[e] * img[(size_t)(nb0 + lrow[e]) * row_len + 5];
      lval[e] = score;
      lcls[e] = score > conf_thres ? (unsigned short)0 : FAILED;
    }
  } else {
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
        const float score = lval[e] * bv;      // rule 2
        lval[e] = score;
        lcls[e] = score > conf_thres ? (unsigned short)bk : FAILED;
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
__global__ __launch_bounds__(256) void mc_nms_keys_kernel(const float* __restrict__ scores, int n, unsigned long long* __restrict__ keys,
                                                          int* __restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = make_key(scores[i], (unsigned)i);
  if (i == 0) *cnt = n;
}

// ---------------------------------------------------------------- stage 2
struct McArgs {
  const unsigned long long* keys;  // [B][N]
  const int* cnt;                  // [B], CNT_STRIDE apart
  int N, top_k;
  float nms_thres;
  const float* pred; int row_len;             // batched source
  const unsigned short* cls16;                // [B][N], valid at candidate rows
  const float* boxes; const int* classes;     // single-image source
  const float* targets; int T; float iou_thres, width, height;
  float* out_boxes; float* out_prob; int* out_cls; long long* out_index; unsigned char* out_correct; int* out_count; float* out_stats;
};

__device__ __forceinline__ float key_score(unsigned long long key) {  // ord32's inverse
  const unsigned o = (unsigned)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// AP / recall / precision (utils.py:58-119) of `count` (1..KMAX) detections in score order: postprocess.hip's integral, operation for
// operation.  Called by every thread of the workgroup; the result is valid on thread 0.
__device__ float4 mc_ap_integral(PostSmem& sm, const float* tp01, int count, int ngt, float* rec, float* pre, float* term) {
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

// the classes, the two permutations between score order and segment order, the segment table and the kept bits: beside PostSmem
constexpr int MC_EXTRA_LDS = KMAX * 4 + 3 * KMAX * 2 + (KMAX + 2) * 2 + KW * 8;
static_assert(sizeof(PostSmem) + MC_EXTRA_LDS + 64 <= 64 * 1024, "stage 2 keeps its static LDS under 64 KB");

template <bool BATCHED>
__global__ __launch_bounds__(PB) void mc_image_kernel(McArgs A) {
  __shared__ PostSmem sm;
  __shared__ int cl[KMAX];                       // class of sorted candidate t
  __shared__ unsigned short perm[KMAX];          // segment order -> score order
  __shared__ unsigned short pos[KMAX];           // score order -> segment order
  __shared__ unsigned short segid[KMAX];         // segment of position p
  __shared__ unsigned short segstart[KMAX + 2];  // first position of segment s; segstart[nseg] = K
  __shared__ unsigned long long keptw[KW];       // kept bits in segment order
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long* keys = A.keys + (size_t)b * A.N;
  int cnt = A.cnt[b * CNT_STRIDE];
  cnt = cnt < 0 ? 0 : (cnt < A.N ? cnt : A.N);
  const int K = cnt < A.top_k ? cnt : A.top_k;

  // ---- candidates -> sm.key[0..K) sorted by descending key (rule 4)
  unsigned long long thresh = 0;
  if (cnt > A.top_k) thresh = radix_select([keys](int i) { return keys[i]; }, cnt, A.top_k, sm);
  if (tid == 0) sm.sel = 0;
  if (tid < KW) keptw[tid] = 0;
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

  // ---- boxes, areas (rule 5) and classes
  for (int t = tid; t < K; t += PB) {
    const unsigned idx = (unsigned)sm.key[t];
    float4 bx;
    if (BATCHED) {
      const float* r = A.pred + ((size_t)b * A.N + idx) * A.row_len;
      const float cx = r[0], cy = r[1], hw = r[2] / 2.f, hh = r[3] / 2.f;
      bx = make_float4(cx - hw, cy - hh, cx + hw, cy + hh);
      cl[t] = (int)A.cls16[(size_t)b * A.N + idx];
    } else {
      const float* r = A.boxes + (size_t)idx * 4;
      bx = make_float4(r[0], r[1], r[2], r[3]);
      cl[t] = A.classes[idx];
    }
    sm.box[t] = bx;
    sm.area[t] = (bx.z - bx.x) * (bx.w - bx.y);
  }
  __syncthreads();

  // ---- rank sort on (class, position): one contiguous segment per class present, each in score order.  Two threads per candidate.
  {
    const int i = tid & (KMAX - 1), h = tid / KMAX;
    const int half = (K + 1) >> 1;
    int rank = 0;
    if (i < K) {
      const int ci = cl[i];
      const int j0 = h * half, j1 = (j0 + half) < K ? (j0 + half) : K;
#pragma unroll 8
      for (int j = j0; j < j1; ++j) { const int cj = cl[j]; rank += (cj < ci || (cj == ci && j < i)) ? 1 : 0; }
    }
    if (h == 1 && i < K) sm.keep[i] = rank;
    __syncthreads();
    if (h == 0 && i < K) { rank += sm.keep[i]; perm[rank] = (unsigned short)i; pos[i] = (unsigned short)rank; }
    __syncthreads();
  }
  // ---- segment table
  int nseg;
  {
    const bool head = tid < K && (tid == 0 || cl[perm[tid]] != cl[perm[tid - 1]]);
    const unsigned long long m = __ballot(head);
    if (lane == 0) sm.wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < PB / 64; ++w) { const int v = sm.wsum[w]; total += v; before += w < wave ? v : 0; }
    const int sid = before + __popcll(m & ((2ull << lane) - 1ull)) - 1;
    if (tid < K) segid[tid] = (unsigned short)sid;
    if (head) segstart[sid] = (unsigned short)tid;
    if (tid == 0) segstart[total] = (unsigned short)K;
    nseg = total;
    __syncthreads();
  }

  // ---- suppression bits inside segments only: bit j of mask[p] set when position j (> p, same segment) is removed once p is kept (rule 6)
  for (int p = wave; p < K; p += PB / 64) {
    const int i = perm[p], end = segstart[segid[p] + 1];
    const float4 bi = sm.box[i];
    const float ai = sm.area[i];
    for (int w = p >> 6; w * 64 < end; ++w) {
      const int j = w * 64 + lane;
      bool rem = false;
      if (j > p && j < end) {
        const int jj = perm[j];
        float inter;
        const float iou = nms_pair_iou(bi, ai, sm.box[jj], sm.area[jj], inter);
        rem = !(iou <= A.nms_thres);                    // survivors are IoU.le(overlap); NaN is removed
      }
      const unsigned long long m = __ballot(rem);
      if (lane == 0) sm.mask[p][w] = m;
    }
  }
  __syncthreads();

  // ---- greedy scan, one wave per segment.  Lane w owns word w of the removed set; each 64-position word is resolved in registers: lane l
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

  // ---- kept bits back to score order, compacted into sm.keep
  int count;
  {
    bool k = false;
    if (tid < K) { const int p = pos[tid]; k = (keptw[p >> 6] >> (p & 63)) & 1ull; }
    const unsigned long long m = __ballot(k);
    if (lane == 0) sm.wsum[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < PB / 64; ++w) { const int v = sm.wsum[w]; total += v; before += w < wave ? v : 0; }
    if (k) sm.keep[before + __popcll(m & ((1ull << lane) - 1))] = tid;
    count = total;
    __syncthreads();
  }

  if (!BATCHED) {
    for (int c = tid; c < count; c += PB) A.out_index[c] = (long long)(unsigned)sm.key[sm.keep[c]];
    if (tid == 0) A.out_count[0] = count;
    return;
  }

  // ---- kept detections out, in descending-key order (rule 7)
  const size_t ob = (size_t)b * A.top_k;
  for (int c = tid; c < count; c += PB) {
    const int t = sm.keep[c];
    const unsigned long long key = sm.key[t];
    *(float4*)(A.out_boxes + (ob + c) * 4) = sm.box[t];
    A.out_prob[ob + c] = key_score(key);
    A.out_cls[ob + c] = cl[t];
    A.out_index[ob + c] = (long long)(unsigned)key;
  }
  for (int c = count + tid; c < A.top_k; c += PB) {
    *(float4*)(A.out_boxes + (ob + c) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    A.out_prob[ob + c] = 0.f; A.out_cls[ob + c] = 0; A.out_index[ob + c] = 0; A.out_correct[ob + c] = 0;
  }
  if (tid == 0) A.out_count[b] = count;
  if (!A.targets) {
    for (int c = tid; c < count; c += PB) A.out_correct[ob + c] = 0;
    if (tid == 0) { float4 z = make_float4(0.f, 0.f, 0.f, 0.f); *(float4*)(A.out_stats + (size_t)b * 4) = z; }
    return;
  }

  // ---- labels (rule 8): rows with all of (cx,cy,w,h) > 0 are real
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
    for (int c = tid; c < count; c += PB) A.out_correct[ob + c] = 0;
    if (tid == 0) { float4 z = make_float4(0.f, 0.f, 0.f, 0.f); *(float4*)(A.out_stats + (size_t)b * 4) = z; }
    return;
  }
  for (int c = tid; c < count; c += PB) {
    const int t0 = sm.keep[c];
    const float4 d = sm.box[t0];
    const float fk = (float)cl[t0];
    const float da = (d.z - d.x + 1.f) * (d.w - d.y + 1.f);
    float bv = -1.f; int bt = -1;
    for (int t = 0; t < A.T; ++t) {
      const float* l = tg + t * 5;
      const float lx = l[1], ly = l[2], lw = l[3], lh = l[4];
      if (!(lx > 0.f && ly > 0.f && lw > 0.f && lh > 0.f) || !(l[0] == fk)) continue;   // real, and of the detection's class
      const float tx1 = (lx - lw / 2.f) * A.width, ty1 = (ly - lh / 2.f) * A.height;
      const float tx2 = (lx + lw / 2.f) * A.width, ty2 = (ly + lh / 2.f) * A.height;
      const float ix1 = fmaxf(d.x, tx1), iy1 = fmaxf(d.y, ty1), ix2 = fminf(d.z, tx2), iy2 = fminf(d.w, ty2);
      const float inter = fmaxf(ix2 - ix1 + 1.f, 0.f) * fmaxf(iy2 - iy1 + 1.f, 0.f);
      const float ta = (tx2 - tx1 + 1.f) * (ty2 - ty1 + 1.f);
      const float iou = inter / (da + ta - inter + 1e-12f);
      if (bt < 0 || iou > bv) { bv = iou; bt = t; }                                       // first maximum
    }
    best_iou[c] = bv; best_t[c] = bt; okf[c] = (bt >= 0 && bv > A.iou_thres) ? 1 : 0;
  }
  __syncthreads();
  for (int c = tid; c < count; c += PB) {
    int ok = okf[c];
    const int bt = best_t[c];
    for (int e = 0; ok && e < c; ++e) ok = !(okf[e] && best_t[e] == bt);
    A.out_correct[ob + c] = (unsigned char)ok;
    best_iou[c] = ok ? 1.f : 0.f;
  }
  __syncthreads();
  const float4 o = mc_ap_integral(sm, best_iou, count, ngt, rec, pre, term);
  if (tid == 0) *(float4*)(A.out_stats + (size_t)b * 4) = o;
}

}  // namespace

#define MC_CHECK_LAUNCH()                                     \
  do {                                                        \
    hipError_t e__ = hipGetLastError();                       \
    if (e__ != hipSuccess) return (int)e__;                   \
  } while (0)

extern "C" {

// workspace: keys u64[B*N] | cnt int[B * CNT_STRIDE] | cls u16[B*N]
long long mdcv_detect_post_mc_workspace_bytes(int B, int N) {
  if (B <= 0 || N <= 0) return 0;
  return (long long)B * N * 8 + (long long)B * CNT_STRIDE * 4 + (((long long)B * N * 2 + 15) & ~15LL);
}

int mdcv_detect_post_mc(const float* pred, int B, int N, int C, const float* targets, int T, float conf_thres, float nms_thres,
                        float iou_thres, float width, float height, int top_k, float* out_boxes, float* out_prob, int* out_cls,
                        long long* out_index, unsigned char* out_correct, int* out_count, float* out_stats, void* workspace,
                        void* stream) {
  if (!pred || !out_boxes || !out_prob || !out_cls || !out_index || !out_correct || !out_count || !out_stats || !workspace)
    return MDCV_EARG;
  if (B <= 0 || B > 65535 || N <= 0 || C < 1 || C > MDCV_MCDET_MAX_CLASSES || T < 0 || top_k <= 0 || top_k > KMAX ||
      (targets == nullptr && T != 0))
    return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  int* cnt = (int*)(keys + (size_t)B * N);
  unsigned short* cls16 = (unsigned short*)(cnt + (size_t)B * CNT_STRIDE);
  hipLaunchKernelGGL(mc_clear_kernel, dim3((B * CNT_STRIDE + 255) / 256), dim3(256), 0, st, cnt, B * CNT_STRIDE);
  MC_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_filter_kernel, dim3((N + FILTER_ROWS - 1) / FILTER_ROWS, B), dim3(256), 0, st, pred, N, C, conf_thres, keys, cls16, cnt);
  MC_CHECK_LAUNCH();
  McArgs a{};
  a.keys = keys; a.cnt = cnt; a.N = N; a.top_k = top_k; a.nms_thres = nms_thres;
  a.pred = pred; a.row_len = 5 + C; a.cls16 = cls16;
  a.targets = T > 0 ? targets : nullptr; a.T = T; a.iou_thres = iou_thres; a.width = width; a.height = height;
  a.out_boxes = out_boxes; a.out_prob = out_prob; a.out_cls = out_cls; a.out_index = out_index; a.out_correct = out_correct;
  a.out_count = out_count; a.out_stats = out_stats;
  hipLaunchKernelGGL(mc_image_kernel<true>, dim3(B), dim3(PB), 0, st, a);
  MC_CHECK_LAUNCH();
  return MDCV_OK;
}

long long mdcv_nms_mc_workspace_bytes(int n) { return n <= 0 ? 128 : (long long)n * 8 + 128; }

int mdcv_nms_mc(const float* boxes, const float* scores, const int* classes, int n, float overlap, int top_k, long long* keep, int* count,
                void* workspace, void* stream) {
  if (n < 0 || top_k <= 0 || top_k > KMAX || !keep || !count || !workspace || (n > 0 && (!boxes || !scores || !classes))) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    hipLaunchKernelGGL(mc_clear_kernel, dim3(1), dim3(256), 0, st, count, 1);
    MC_CHECK_LAUNCH();
    return MDCV_OK;
  }
  unsigned long long* keys = (unsigned long long*)workspace;
  int* cnt = (int*)(keys + n);
  hipLaunchKernelGGL(mc_nms_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, st, scores, n, keys, cnt);
  MC_CHECK_LAUNCH();
  McArgs a{};
  a.keys = keys; a.cnt = cnt; a.N = n; a.top_k = top_k; a.nms_thres = overlap; a.boxes = boxes; a.classes = classes;
  a.out_index = keep; a.out_count = count;
  hipLaunchKernelGGL(mc_image_kernel<false>, dim3(1), dim3(PB), 0, st, a);
  MC_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
