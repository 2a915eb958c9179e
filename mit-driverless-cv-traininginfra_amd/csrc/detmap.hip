// Dataset-level detection evaluation: COCO-style average precision over a whole validation set, on the device, integer-exact.
// Two entry points.
//   mdcv_detmap_match     one launch per batch, grid (B, S, ceil(J / 4)), one 256-thread workgroup per (image, size range s, four thresholds).
//                         The image's detections and ground truth are staged in LDS; wave w takes the threshold j = 4 z + w; the workgroup
//                         owns one byte of each status word.  For its (j, s) a wave runs COCOeval.evaluateImg: detections in row order (most confident first, as mdcv_detect_post / mdcv_detect_merge_tiles
//                         leave them), lanes striding over the ground truth, one wave arg-max per detection over the key
//                         (not ignored, IoU bits, ground-truth index): the largest IoU >= thr_j among the unmatched ground truth of the
//                         detection's class, a non-ignored one before an ignored one, the HIGHER index on equal IoU (COCO's `<` test).
//                         The matched flags of a lane's ground truth are one 32-bit register (T <= 2048 = 64 lanes x 32).
//                         IoU is nms_core.h's nms_pair_iou(detection, ground truth), areas (x2-x1)*(y2-y1) in fp32: the arithmetic of NMS.
//                         Out: the image's rows of the dataset buffers (score, cls, count, two status bits per threshold) and the
//                         non-ignored ground truth per (range, class) added to n_gt with integer atomics (order-free, so deterministic).
//   mdcv_detmap_finalize  keys (cls << 32) | (0xFFFFFFFF - bits(score)), all ones for an invalid slot, value = slot; rocPRIM's stable radix
//                         sort; then one workgroup per (class, j, s): its segment of the sorted slots (two binary searches), one walk
//                         forward for the totals, one walk backward in chunks of MDCV_DETMAP_CHUNK with a block suffix scan carried from
//                         chunk to chunk: true positives and non-ignored detections behind a position, then the precision envelope, the
//                         suffix maximum of the rationals tp_i / nd_i compared by 64-bit cross-multiplication.  A non-ignored position
//                         writes the recall levels k it is the first to reach (100 * tp_i >= k * n_gt, integers).  Thread 0 sums the 101
//                         quotients in fp64 in the order k = 0..100.  Nothing but that last step is floating point.
// Plain C++, vector stores only.  Built with -ffp-contract=off like postprocess.hip: every fp32 / fp64 operation rounds on its own.
#include "../../include/mdcv_hip.h"
#include "common.h"
#include "nms_core.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int TMAX = MDCV_DETMAP_MAX_GT;
constexpr int JMAX = MDCV_DETMAP_MAX_THR;
constexpr int SMAX = MDCV_DETMAP_MAX_RANGES;
constexpr int CMAX = MDCV_DETMAP_MAX_CLASSES;
constexpr int CH = MDCV_DETMAP_CHUNK;
constexpr int NW = PB / 64;
constexpr int MB = 256, MW = MB / 64;            // the match kernel: 4 waves per workgroup, one threshold each: one byte of a status word
constexpr int GT_IGN = 1 << 30;                 // gmeta: class | GT_IGN, or -1 for a row that is no ground truth
constexpr int GT_CLS = GT_IGN - 1;
static_assert(TMAX == 64 * 32, "a lane keeps the matched flags of its ground truth in one 32-bit register");
static_assert(CMAX <= GT_CLS && TMAX < 4096, "class and ground-truth index fields of the match key");
static_assert(CH == PB, "the curve kernel scans one element per thread");
enum { ST_FP = MDCV_DETMAP_FP, ST_TP = MDCV_DETMAP_TP, ST_IGN = MDCV_DETMAP_IGNORED };

struct MatchArgs {
  const float* boxes; const float* prob; const int* cls; const int* count;
  const float* gt; const int* gt_cls; const unsigned char* gt_ignore; const int* gt_count;
  int K, T, mode, J, S, C, first;
  long long cap;
  float width, height;
  float thr[JMAX], lo[SMAX], hi[SMAX];
  float* score; int* ocls; int* ocount; unsigned* status; unsigned long long* n_gt;
};

struct MatchSmem {
  float4 gbox[TMAX];
  int gmeta[TMAX];
  float4 dbox[KMAX];
  int dcls[KMAX];
  unsigned stat[KMAX];
};

__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x) * (b.w - b.y); }   // nms.py:24
__device__ __forceinline__ bool in_range(float a, float lo, float hi) { return a >= lo && a < hi; }

__global__ __launch_bounds__(MB) void detmap_match_kernel(MatchArgs A) {
  __shared__ MatchSmem sm;
  const int b = blockIdx.x, s = blockIdx.y, jg = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.K, T = A.T;
  const bool first_wg = s == 0 && jg == 0;
  int cnt = A.count[b];
  cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
  const size_t row = (size_t)(A.first + b) * K;

  // ---- the image's detections: LDS, and (the workgroup of range 0, thresholds 0..3) its rows of the dataset buffers, every slot of them
  for (int k = tid; k < K; k += MB) {
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float p = 0.f;
    int c = 0;
    if (k < cnt) {
      const float* r = A.boxes + ((size_t)b * K + k) * 4;
      bx = make_float4(r[0], r[1], r[2], r[3]);
      p = A.prob[(size_t)b * K + k];
      c = A.cls ? A.cls[(size_t)b * K + k] : 0;
    }
    sm.dbox[k] = bx; sm.dcls[k] = c; sm.stat[k] = 0u;
    if (first_wg) { A.score[row + k] = p; A.ocls[row + k] = c; }
  }
  if (tid == 0 && first_wg) A.ocount[A.first + b] = cnt;

  // ---- the image's ground truth
  if (A.mode == MDCV_DETMAP_GT_PIXELS) {
    int ng = A.gt_count[b];
    ng = ng < 0 ? 0 : (ng > T ? T : ng);
    for (int t = tid; t < T; t += MB) {
      float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
      int meta = -1;
      if (t < ng) {
        const float* r = A.gt + ((size_t)b * T + t) * 4;
        bx = make_float4(r[0], r[1], r[2], r[3]);
        const int c = A.gt_cls ? A.gt_cls[(size_t)b * T + t] : 0;
        const bool ign = A.gt_ignore && A.gt_ignore[(size_t)b * T + t] != 0;
        if (c >= 0 && c < A.C) meta = c | (ign ? GT_IGN : 0);
      }
      sm.gbox[t] = bx; sm.gmeta[t] = meta;
    }
  } else {
    for (int t = tid; t < T; t += MB) {
      const float* l = A.gt + ((size_t)b * T + t) * 5;
      const float lc = l[0], lx = l[1], ly = l[2], lw = l[3], lh = l[4];
      float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
      int meta = -1;
      if (lx > 0.f && ly > 0.f && lw > 0.f && lh > 0.f) {                                 // validate.py:105, as mdcv_detect_post
        bx = make_float4((lx - lw / 2.f) * A.width, (ly - lh / 2.f) * A.height,          // utils.py:121-127, validate.py:107-109
                         (lx + lw / 2.f) * A.width, (ly + lh / 2.f) * A.height);
        if (lc >= 0.f && lc < (float)A.C) meta = (int)lc;
      }
      sm.gbox[t] = bx; sm.gmeta[t] = meta;
    }
  }
  __syncthreads();

  // ---- n_gt[s][c] += the image's non-ignored ground truth: wave 0, one atomic per class and 64 rows
  const float lo = A.lo[s], hi = A.hi[s];
  if (wave == 0 && jg == 0) {
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      const int meta = t < T ? sm.gmeta[t] : -1;
      const bool on = meta >= 0 && !(meta & GT_IGN) && in_range(box_area(sm.gbox[t < T ? t : 0]), lo, hi);
      const int c = meta & GT_CLS;
      unsigned long long m = __ballot(on);
      while (m) {
        const int leader = __ffsll((long long)m) - 1;
        const int lc = __shfl(c, leader, 64);
        const unsigned long long same = __ballot(on && c == lc);
        if (lane == leader) atomicAdd(&A.n_gt[(size_t)s * A.C + lc], (unsigned long long)__popcll(same));
        m &= ~same;
      }
    }
  }

  // ---- the matching: wave w of workgroup jg takes the threshold j = MW * jg + w
  const int j = MW * jg + wave;
  if (j < A.J) {                                                                           // wave-uniform
    const float th = A.thr[j];
    const int nI = (T + 63) >> 6;
    unsigned validm = 0u, ignm = 0u, matched = 0u;
    for (int i = 0; i < nI; ++i) {
      const int t = lane + 64 * i;
      if (t < T) {
        const int meta = sm.gmeta[t];
        if (meta >= 0) {
          validm |= 1u << i;
          if ((meta & GT_IGN) || !in_range(box_area(sm.gbox[t]), lo, hi)) ignm |= 1u << i;
        }
      }
    }
    // a lane's first ground truth stays in registers (T <= 64: its only one); the next detection is loaded under this one's work
    const bool v0 = (validm & 1u) != 0u;
    const float4 g0 = v0 ? sm.gbox[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int c0 = v0 ? (sm.gmeta[lane] & GT_CLS) : -1;
    const float a0 = box_area(g0);
    const unsigned long long nonign0 = (unsigned long long)((ignm & 1u) ^ 1u) << 62;
    float4 bn = sm.dbox[0];
    int cn = sm.dcls[0];
    for (int d = 0; d < cnt; ++d) {
      const float4 bi = bn;
      const int c = cn;
      const int dn = d + 1 < cnt ? d + 1 : d;
      bn = sm.dbox[dn]; cn = sm.dcls[dn];
      const float ai = box_area(bi);
      unsigned long long best = 0ull;
      if (v0 && !(matched & 1u) && c0 == c) {
        float inter;
        const float iou = nms_pair_iou(bi, ai, g0, a0, inter);
        if (iou >= th) best = nonign0 | ((unsigned long long)__float_as_uint(iou) << 12) | (unsigned long long)(lane + 1);   // th > 0: ordered bits
      }
      unsigned open = validm & ~matched & ~1u;
      while (open) {
        const int i = __ffs((int)open) - 1;
        open &= open - 1u;
        const int t = lane + 64 * i;
        if ((sm.gmeta[t] & GT_CLS) != c) continue;
        const float4 bj = sm.gbox[t];
        float inter;
        const float iou = nms_pair_iou(bi, ai, bj, box_area(bj), inter);
        if (iou >= th) {
          const unsigned long long key = ((unsigned long long)(((ignm >> i) & 1u) ^ 1u) << 62) |
                                         ((unsigned long long)__float_as_uint(iou) << 12) | (unsigned long long)(t + 1);
          best = key > best ? key : best;
        }
      }
      const unsigned long long has = __ballot(best != 0ull);                               // wave-uniform
      if (has != 0ull && (has & (has - 1ull)) == 0ull) {                                   // one lane has a candidate: its key is the maximum
        const int src = __ffsll((long long)has) - 1;
        const unsigned lo32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)best, src);
        const unsigned hi32 = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(best >> 32), src);
        best = ((unsigned long long)hi32 << 32) | lo32;
      } else if (has != 0ull) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long v = __shfl_xor(best, o, 64);
          best = v > best ? v : best;
        }
      }
      unsigned st;
      if (best) {
        const int t = (int)(best & 0xfffull) - 1;
        if ((t & 63) == lane) matched |= 1u << (t >> 6);
        st = ((best >> 62) & 1ull) ? ST_TP : ST_IGN;
      } else {
        st = in_range(ai, lo, hi) ? ST_FP : ST_IGN;
      }
      if (lane == 0 && st) atomicOr(&sm.stat[d], st << (2 * wave));
    }
  }
  __syncthreads();
  // the workgroup's four thresholds are bits 8 jg .. 8 jg + 7 of the status word: its own byte, stored as a byte (the last workgroup also
  // clears what lies above the thresholds), so the workgroups of one word need no atomics and the buffer no clearing
  static_assert(MW == 4, "four thresholds of two bits: one byte");
  unsigned char* sb = (unsigned char*)(A.status + ((size_t)s * A.cap) * K + row);
  const int last = (A.J - 1) / MW;
  for (int k = tid; k < K; k += MB) {
    sb[4 * (size_t)k + jg] = (unsigned char)sm.stat[k];
    if (jg == last)
      for (int z = last + 1; z < 4; ++z) sb[4 * (size_t)k + z] = 0;
  }
}

// ------------------------------------------------------------------------------------------------------------------------- finalize
__global__ void detmap_keys_kernel(const float* __restrict__ score, const int* __restrict__ cls, const int* __restrict__ count, int K, int C,
                                   unsigned N, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals, int* __restrict__ err) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const unsigned img = i / (unsigned)K, k = i - img * (unsigned)K;
  int cnt = count[img];
  cnt = cnt > K ? K : cnt;
  unsigned long long key = ~0ull;
  const int c = cls[i];
  if ((int)k < cnt && c >= 0 && c < C) {
    const float sc = score[i];
    if (sc > 0.f) key = ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xFFFFFFFFu - __float_as_uint(sc));
    else atomicOr(err, 1);                                                                // NaN or not positive: the bits are not ordered
  }
  keys[i] = key; vals[i] = i;
}

struct CurveArgs {
  const unsigned long long* keys;   // sorted
  const unsigned* vals;             // slot of each sorted key
  const unsigned* status;
  const long long* n_gt;
  unsigned N;
  int K, J, S, C;
  long long cap;
  long long* q; long long* tot; double* ap;
};

__device__ unsigned lower_bound_u64(const unsigned long long* a, unsigned n, unsigned long long v) {
  unsigned lo = 0, hi = n;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ long long gcd_ll(long long a, long long b) {
  while (b) { const long long r = a % b; a = b; b = r; }
  return a;
}

__global__ __launch_bounds__(PB) void detmap_curve_kernel(CurveArgs A) {
  __shared__ long long q_l[101][2];
  __shared__ int agg_tp[2][NW], agg_nd[2][NW], agg_n[2][NW], agg_d[2][NW];
  __shared__ int car_tp[2], car_nd[2], car_n[2], car_d[2];
  __shared__ unsigned s_lo, s_hi, s_tp, s_nd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = blockIdx.x;
  const int c = bid / (A.J * A.S), j = (bid / A.S) % A.J, s = bid % A.S;
  const unsigned* status = A.status + (size_t)s * A.cap * A.K;
  const int sh = 2 * j;

  if (tid < 101) { q_l[tid][0] = 0; q_l[tid][1] = 1; }                                    // an unreachable level is (0, 1)
  if (tid == 0) {
    s_lo = lower_bound_u64(A.keys, A.N, (unsigned long long)c << 32);
    s_hi = lower_bound_u64(A.keys, A.N, (unsigned long long)(c + 1) << 32);
    s_tp = 0u; s_nd = 0u;
    car_tp[0] = 0; car_nd[0] = 0; car_n[0] = 0; car_d[0] = 1;
  }
  __syncthreads();
  const unsigned lo = s_lo, hi = s_hi;

  // ---- forward: the totals
  {
    int ltp = 0, lnd = 0;
    for (unsigned p = lo + tid; p < hi; p += PB) {
      const unsigned st = (status[A.vals[p]] >> sh) & 3u;
      ltp += st == ST_TP; lnd += st != ST_IGN;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ltp += __shfl_xor(ltp, o, 64); lnd += __shfl_xor(lnd, o, 64); }
    if (lane == 0) { if (ltp) atomicAdd(&s_tp, (unsigned)ltp); if (lnd) atomicAdd(&s_nd, (unsigned)lnd); }
  }
  __syncthreads();
  const long long tot_tp = s_tp, tot_nd = s_nd;
  const long long ngt = A.n_gt[(size_t)s * A.C + c];

  // ---- backward: suffix counts, the precision envelope, the recall levels
  if (ngt > 0 && tot_nd > 0) {
    const int nch = (int)((hi - lo + CH - 1) / CH);
    int par = 0;
    for (int ch = nch - 1; ch >= 0; --ch, par ^= 1) {
      const unsigned p = lo + (unsigned)ch * CH + tid;
      const unsigned st = p < hi ? (status[A.vals[p]] >> sh) & 3u : (unsigned)ST_IGN;
      const int f_tp = st == ST_TP, f_nd = st != ST_IGN;
      int x_tp = f_tp, x_nd = f_nd;                                                       // inclusive suffix sums inside the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_down(x_tp, o, 64), b = __shfl_down(x_nd, o, 64);
        if (lane + o < 64) { x_tp += a; x_nd += b; }
      }
      if (lane == 0) { agg_tp[par][wave] = x_tp; agg_nd[par][wave] = x_nd; }
      __syncthreads();
      int a_tp = car_tp[par], a_nd = car_nd[par];                                         // behind this chunk
      for (int w = wave + 1; w < NW; ++w) { a_tp += agg_tp[par][w]; a_nd += agg_nd[par][w]; }
      const int S_tp = x_tp + a_tp, S_nd = x_nd + a_nd;                                   // at and behind this position
      if (tid == 0) { car_tp[par ^ 1] = S_tp; car_nd[par ^ 1] = S_nd; }
      const long long tp_i = tot_tp - S_tp + f_tp, nd_i = tot_nd - S_nd + 1;              // up to and including this position
      int rn = f_nd ? (int)tp_i : 0, rd = f_nd ? (int)nd_i : 1;                           // precision here; 0 / 1 where there is none
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int on = __shfl_down(rn, o, 64), od = __shfl_down(rd, o, 64);
        if (lane + o < 64 && (long long)on * rd > (long long)rn * od) { rn = on; rd = od; }
      }
      if (lane == 0) { agg_n[par][wave] = rn; agg_d[par][wave] = rd; }
      __syncthreads();
      int en = car_n[par], ed = car_d[par];
      for (int w = wave + 1; w < NW; ++w) {
        const int on = agg_n[par][w], od = agg_d[par][w];
        if ((long long)on * ed > (long long)en * od) { en = on; ed = od; }
      }
      if ((long long)en * rd > (long long)rn * ed) { rn = en; rd = ed; }                  // the envelope at this position
      if (tid == 0) { car_n[par ^ 1] = rn; car_d[par ^ 1] = rd; }
      if (f_nd) {
        long long khi = 100 * tp_i / ngt, klo = nd_i == 1 ? -1 : 100 * (tp_i - f_tp) / ngt;
        khi = khi > 100 ? 100 : khi; klo = klo > 100 ? 100 : klo;
        if (khi > klo) {
          const long long g = rn ? gcd_ll(rn, rd) : (long long)rd;                        // lowest terms; 0 is 0 / 1
          for (long long k = klo + 1; k <= khi; ++k) { q_l[k][0] = rn / g; q_l[k][1] = rd / g; }
        }
      }
    }
  }
  __syncthreads();
  if (tid < 101) {
    long long* o = A.q + ((size_t)bid * 101 + tid) * 2;
    o[0] = q_l[tid][0]; o[1] = q_l[tid][1];
  }
  if (tid == 0) {
    long long* t = A.tot + (size_t)bid * 3;
    t[0] = ngt; t[1] = tot_tp; t[2] = tot_nd;
    double ap = -1.0;
    if (ngt > 0) {
      double sum = 0.0;
      for (int k = 0; k <= 100; ++k) sum += (double)q_l[k][0] / (double)q_l[k][1];
      ap = sum / 101.0;
    }
    A.ap[bid] = ap;
  }
}

bool dims_ok(int K, int J, int S, int C, long long cap) {
  return K >= 1 && K <= KMAX && J >= 1 && J <= JMAX && S >= 1 && S <= SMAX && C >= 1 && C <= CMAX && cap >= 1 &&
         cap * K <= MDCV_DETMAP_MAX_SLOTS;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

hipError_t sort_pairs(void* temp, size_t& temp_bytes, unsigned long long* kin, unsigned long long* kout, unsigned* vin, unsigned* vout,
                      unsigned n, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, kin, kout, vin, vout, (size_t)n, 0u, 64u, st, false);
}

}  // namespace

extern "C" {

int mdcv_detmap_match(const float* boxes, const float* prob, const int* cls, const int* count, int B, int K, int gt_mode, const float* gt,
                      const int* gt_cls, const unsigned char* gt_ignore, const int* gt_count, int T, float width, float height,
                      const float* iou_thr, int J, const float* ranges, int S, int C, long long first, long long cap, float* ds_score,
                      int* ds_cls, int* ds_count, unsigned* ds_status, long long* ds_n_gt, void* stream) {
  if (!dims_ok(K, J, S, C, cap) || B < 0 || B > 65535 || T < 0 || T > TMAX || first < 0 || first + B > cap) return MDCV_EARG;
  if (gt_mode != MDCV_DETMAP_GT_PIXELS && gt_mode != MDCV_DETMAP_GT_LABELS) return MDCV_EARG;
  if (!iou_thr || !ranges) return MDCV_EARG;
  MatchArgs a{};
  for (int j = 0; j < J; ++j) {
    if (!(iou_thr[j] > 0.f && iou_thr[j] <= 1.f)) return MDCV_EARG;                       // also NaN
    a.thr[j] = iou_thr[j];
  }
  for (int s = 0; s < S; ++s) {
    const float lo = ranges[2 * s], hi = ranges[2 * s + 1];
    if (!(lo <= hi)) return MDCV_EARG;                                                    // lo > hi, or a NaN
    a.lo[s] = lo; a.hi[s] = hi;
  }
  if (gt_mode == MDCV_DETMAP_GT_LABELS && !(width > 0.f && height > 0.f)) return MDCV_EARG;
  if (!ds_score || !ds_cls || !ds_count || !ds_status || !ds_n_gt) return MDCV_EARG;
  if (B == 0) return MDCV_OK;
  if (!boxes || !prob || !count) return MDCV_EARG;
  if (T > 0 && (!gt || (gt_mode == MDCV_DETMAP_GT_PIXELS && !gt_count))) return MDCV_EARG;
  a.boxes = boxes; a.prob = prob; a.cls = cls; a.count = count;
  a.gt = gt; a.gt_cls = gt_cls; a.gt_ignore = gt_ignore; a.gt_count = gt_count;
  a.K = K; a.T = T; a.mode = T > 0 ? gt_mode : MDCV_DETMAP_GT_LABELS;                     // T == 0: no ground-truth pointer is read
  a.J = J; a.S = S; a.C = C; a.first = (int)first; a.cap = cap;
  a.width = width; a.height = height;
  a.score = ds_score; a.ocls = ds_cls; a.ocount = ds_count; a.status = ds_status; a.n_gt = (unsigned long long*)ds_n_gt;
  MDCV_LAUNCH(detmap_match_kernel, dim3((unsigned)B, (unsigned)S, (unsigned)((J + MW - 1) / MW)), dim3(MB), 0, (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

/* keys in | keys out (u64 [cap*K] each) | slots in | slots out (u32 [cap*K] each) | rocPRIM's temporary storage */
long long mdcv_detmap_finalize_workspace_bytes(long long cap, int K) {
  if (!dims_ok(K, 1, 1, 1, cap)) return MDCV_EARG;
  const size_t n = (size_t)cap * K;
  size_t temp = 0;
  if (sort_pairs(nullptr, temp, nullptr, nullptr, nullptr, nullptr, (unsigned)n, nullptr) != hipSuccess) return -2;
  return (long long)(2 * align256(n * 8) + 2 * align256(n * 4) + align256(temp) + 256);
}

int mdcv_detmap_finalize(const float* ds_score, const int* ds_cls, const int* ds_count, const unsigned* ds_status, const long long* ds_n_gt,
                         long long n_images, long long cap, int K, int J, int S, int C, long long* q, long long* tot, double* ap, int* err,
                         void* workspace, long long workspace_bytes, void* stream) {
  if (!dims_ok(K, J, S, C, cap) || n_images < 0 || n_images > cap) return MDCV_EARG;
  if (!ds_score || !ds_cls || !ds_count || !ds_status || !ds_n_gt || !q || !tot || !ap || !err || !workspace) return MDCV_EARG;
  const size_t ncap = (size_t)cap * K;
  const size_t fixed = 2 * align256(ncap * 8) + 2 * align256(ncap * 4);
  if (workspace_bytes < 0 || (size_t)workspace_bytes < fixed || ((uintptr_t)workspace & 7)) return MDCV_EARG;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)workspace;
  unsigned long long* kin = (unsigned long long*)w;
  unsigned long long* kout = (unsigned long long*)(w + align256(ncap * 8));
  unsigned* vin = (unsigned*)(w + 2 * align256(ncap * 8));
  unsigned* vout = (unsigned*)(w + 2 * align256(ncap * 8) + align256(ncap * 4));
  char* temp = w + fixed;
  temp = (char*)(((uintptr_t)temp + 255) & ~(uintptr_t)255);
  const unsigned N = (unsigned)((size_t)n_images * K);
  hipError_t e = hipMemsetAsync(err, 0, 4, st);
  if (e != hipSuccess) return (int)e;
  if (N > 0) {
    size_t need = 0;
    e = sort_pairs(nullptr, need, kin, kout, vin, vout, N, st);
    if (e != hipSuccess) return (int)e;
    if (temp + need > w + workspace_bytes) return MDCV_EARG;
    MDCV_LAUNCH(detmap_keys_kernel, dim3((N + 255) / 256), dim3(256), 0, st, ds_score, ds_cls, ds_count, K, C, N, kin, vin, err);
    MDCV_CHECK_LAUNCH();
    e = sort_pairs(temp, need, kin, kout, vin, vout, N, st);
    if (e != hipSuccess) return (int)e;
  }
  CurveArgs a{kout, vout, ds_status, ds_n_gt, N, K, J, S, C, cap, q, tot, ap};
  MDCV_LAUNCH(detmap_curve_kernel, dim3((unsigned)(C * J * S)), dim3(PB), 0, st, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
