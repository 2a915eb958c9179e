// Tile-and-scale inference, the join: the detections of one frame arrive as T tiles x K boxes in tile coordinates (mdcv_detect_post's
// out_boxes / out_prob / out_count with one "image" per tile) and leave as ONE list per frame in scaled-frame coordinates, the duplicates of
// overlapping tiles removed by the reference's greedy NMS (utils/nms.py:4-61) run over the frame's candidates.  One launch per batch of
// frames, grid (B), one 1024-thread workgroup per frame, the counts read on the device only.  The reference has no tiled inference; what it
// fixes here is the scan itself and its fp32 arithmetic, which are nms_core.h's, shared with mdcv_nms / mdcv_detect_post.  Per frame b:
//   0. tiles     the device copy of the tile table is searched for the tiles of b and checked again (contiguous, at most
//                MDCV_TILE_MAX_PER_FRAME, offsets within +-MDCV_TILE_MAX_OFFSET, last word 0); a frame that fails, or has no tile, gets count 0
//   1. keys      candidate (t, k), k < min(tile_count[t], K) (a negative count is 0), has the key (ordered(tile_prob[t,k]) << 32) | ~c with
//                c = (t - first tile of b) * K + k: descending key = descending score, equal scores by ascending tile, then ascending slot.
//                The keys are never stored: c runs over the n * K <= 32768 slots of the frame and a slot past its tile's count reads as key 0,
//                which no candidate has and which is smaller than every candidate's
//   2. select    radix select of the top_k largest keys (only when there are more), compaction into LDS, rank sort: the visiting order
//   3. boxes     corner j of a selected candidate: (float)((double)tile_boxes[t,k,j] + (double)off), off_x for j = 0, 2 and off_y for 1, 3:
//                one rounding; area as nms.py:24
//   4. matrix    bit j of row i: j (> i) leaves once i is kept -- !(IoU <= overlap), or, for candidates of different tiles and
//                contain_thres >= 0, !(inter / min(area_j, area_i) <= contain_thres): the half cone a tile edge cut off, inside the whole cone
//                the neighbouring tile saw.  A NaN leaves in both tests
//   5. scan      wave 0, in registers; kept candidates in visiting order
//   6. out       boxes, prob, src = (tile index in the batch, slot in the tile), count; slots past count: zeros, src (-1, -1)
// Plain C++, vector stores only.  Built with -ffp-contract=off like postprocess.hip.
#include "../../include/mdcv_hip.h"
#include "common.h"
#include "nms_core.h"

namespace {

constexpr int MAXT = MDCV_TILE_MAX_PER_FRAME;
static_assert(MAXT <= 256, "the tile of a candidate is kept in one byte");
enum { TD_FRAME = 0, TD_OFF_X = 1, TD_OFF_Y = 2, TD_ZERO = 3 };

// the same test on the host copy (MDCV_EARG) and on the device copy (count 0)
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

struct MergeArgs {
  const float* tile_boxes;  // [T][K][4]
  const float* tile_prob;   // [T][K]
  const int* tile_count;    // [T]
  const int* tiles;         // [T][MDCV_TILE_DESC], device copy
  int T, K, top_k;
  float overlap, contain;
  float* out_boxes; float* out_prob; int* out_src; int* out_count;
};

__global__ __launch_bounds__(PB) void merge_tiles_kernel(MergeArgs A) {
  __shared__ PostSmem sm;
  __shared__ int s_cnt[MAXT];
  __shared__ unsigned char s_tile[KMAX];
  __shared__ int s_lo, s_hi, s_n, s_bad, s_total;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.K;

  // ---- 0. the tiles of this frame
  if (tid == 0) { s_lo = 0x7fffffff; s_hi = -1; s_n = 0; s_bad = 0; s_total = 0; sm.sel = 0; sm.count = 0; }
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

  // ---- 3. merged boxes
  for (int t = tid; t < Ksel; t += PB) {
    const int i = cand_index(sm.key[t], space);
    const int lt = i / K;
    const int* d = A.tiles + (size_t)(t0 + lt) * MDCV_TILE_DESC;
    const double ox = (double)d[TD_OFF_X], oy = (double)d[TD_OFF_Y];
    const float* r = A.tile_boxes + ((size_t)t0 * K + i) * 4;
    const float4 bx = make_float4((float)((double)r[0] + ox), (float)((double)r[1] + oy), (float)((double)r[2] + ox), (float)((double)r[3] + oy));
    sm.box[t] = bx;
    sm.area[t] = (bx.z - bx.x) * (bx.w - bx.y);  // nms.py:24
    s_tile[t] = (unsigned char)lt;
  }
  const int W = (Ksel + 63) >> 6;
  __syncthreads();

  // ---- 4. suppression matrix
  const bool seam = A.contain >= 0.f;
  for (int i = wave; i < Ksel; i += PB / 64) {
    const float4 bi = sm.box[i];
    const float ai = sm.area[i];
    const int ti = s_tile[i];
    for (int w = i >> 6; w < W; ++w) {
      const int j = w * 64 + lane;
      bool rem = false;
      if (j > i && j < Ksel) {
        const float aj = sm.area[j];
        float inter;
        const float iou = nms_pair_iou(bi, ai, sm.box[j], aj, inter);
        rem = !(iou <= A.overlap);                  // survivors are IoU.le(overlap); NaN is removed
        if (seam && s_tile[j] != ti) rem = rem || !(inter / (aj < ai ? aj : ai) <= A.contain);
      }
      const unsigned long long m = __ballot(rem);
      if (lane == 0) sm.mask[i][w] = m;
    }
  }
  __syncthreads();

  // ---- 5. greedy scan (nms_scan.inc)
  if (wave == 0) {
    const int K = Ksel;   // the scan's name for the number of sorted candidates
#include "nms_scan.inc"
  }
  __syncthreads();
  const int count = sm.count;

  // ---- 6. out: every slot of the frame is written
  const size_t ob = (size_t)b * A.top_k;
  for (int c = tid; c < A.top_k; c += PB) {
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float p = 0.f;
    int st = -1, sk = -1;
    if (c < count) {
      const int t = sm.keep[c];
      const int i = cand_index(sm.key[t], space);
      const int lt = i / K;
      bx = sm.box[t]; p = prob[i]; st = t0 + lt; sk = i - lt * K;
    }
    float* o = A.out_boxes + (ob + c) * 4;
    o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w;
    A.out_prob[ob + c] = p;
    A.out_src[(ob + c) * 2] = st; A.out_src[(ob + c) * 2 + 1] = sk;
  }
  if (tid == 0) A.out_count[b] = count;
}

}  // namespace

extern "C" {

int mdcv_detect_merge_tiles(const float* tile_boxes, const float* tile_prob, const int* tile_count, const int* tiles_host, const int* tiles,
                            int T, int K, int B, float overlap, float contain_thres, int top_k, float* out_boxes, float* out_prob,
                            int* out_src, int* out_count, void* stream) {
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
  if (!tile_boxes || !tile_prob || !tile_count || !tiles || !out_boxes || !out_prob || !out_src || !out_count) return MDCV_EARG;
  MergeArgs a{tile_boxes, tile_prob, tile_count, tiles, T, K, top_k, overlap, contain_thres, out_boxes, out_prob, out_src, out_count};
  MDCV_LAUNCH(merge_tiles_kernel, dim3((unsigned)B), dim3(PB), 0, (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
