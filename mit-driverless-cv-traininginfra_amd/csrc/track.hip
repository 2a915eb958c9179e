// Tracking of detections across frames (include/mdcv_track.h): per sequence a table of Kalman-filtered tracks, an optimal
// assignment of tracks to the frame's boxes by IoU, births and deaths -- all frames of a launch inside ONE kernel.
//
// Work split: one 256-thread workgroup per sequence, thread t = slot t = box t.  A slot's 17 filter words and its counters live in thread
// t's REGISTERS for the whole launch (loaded once, stored once); LDS holds what threads share: the frame's boxes, the 256 x 256 16-bit
// cost matrix (rows 129 dwords apart, so that thread t's writes to row t spread over the banks), the row list, the potentials of the rows,
// the column-to-row map and the small hand-over tables of matches and births.  The assignment runs on wave 0 alone: lane l owns columns
// l, l + 64, l + 128, l + 192 with minv, way, used and the column potential in registers, and the least (minv, column) is a DPP row
// rotation + readlane reduction of a 64-bit key -- no workgroup barrier inside an augmentation; the other waves wait at the frame's one
// barrier behind the solve.  Free slots, unmatched boxes and rows are numbered by ballot / popcount prefix counts: ids are deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdcv_track.h"

namespace {

constexpr int kT = MDCV_TRACK_SLOTS;         // threads = slots = boxes of a frame
constexpr int kRow = 2 * 129;                // uint16 per cost row
constexpr int kDummy = 65535;
constexpr int kInf = 0x7fffffff;
constexpr int kHdr = 16;

struct TrackArgs {
  const double* boxes; long long box_seq, box_frame;
  const int* count; long long count_seq, count_frame;
  const int* cls; long long cls_seq, cls_frame;
  int F, K;
  double iou_thres;
  int max_age, min_hits, max_tracks;
  unsigned char* state;
  int* track_id;
  unsigned char* flags;
};

struct Shared {
  uint16_t cost[kT * kRow];                  // 132096 B
  double box[kT][4];                         // the frame's boxes
  int u[kT];                                 // row potentials
  int slot_id[kT], slot_streak[kT];
  int dcls[kT];
  int16_t p[kT];                             // column -> row, -1 none
  int16_t rowslot[kT];                       // row -> slot
  int16_t slot_det[kT], det_slot[kT];        // the matches, -1 none
  int16_t freeslot[kT], birth[kT];           // k-th free slot; slot -> the box that opens a track in it, -1 none
  uint8_t good[kT];
  int wave[3][4];                            // per-wave totals of the three prefix counts
  int stat[2];                               // longest path, scan steps of this frame
};                                           // 145 KB of gfx950's 160 KB

__device__ inline int lane_prefix(unsigned long long mask) {                 // set bits below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

__device__ inline unsigned long long ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }

template <int CTRL>
__device__ inline unsigned long long key_step(unsigned long long k) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xf, 0xf, false);
  const unsigned long long o = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
  return o < k ? o : k;
}

__device__ inline unsigned long long key_lane(unsigned long long k, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// the least key of the wave, in every lane: four rotations inside each row of 16 lanes (row_ror 8, 4, 2, 1), then one lane of each row
__device__ inline unsigned long long wave_min_key(unsigned long long k) {
  k = key_step<0x128>(k);
  k = key_step<0x124>(k);
  k = key_step<0x122>(k);
  k = key_step<0x121>(k);
  const unsigned long long a = key_lane(k, 0), b = key_lane(k, 16), c = key_lane(k, 32), d = key_lane(k, 48);
  const unsigned long long ab = a < b ? a : b, cd = c < d ? c : d;
  return ab < cd ? ab : cd;
}

// The assignment of nr rows to m = max(n, nr) columns on one wave (include/mdcv_track.h, step 3).  Writes slot_det / det_slot.
// The lanes hand u and p to each other through LDS with no fence: a wave's LDS operations complete in order, and `volatile` keeps every
// access a real one in program order.  The stores of one lane (`lane == 0`, the owners of used columns) are read by all lanes in the
// next step -- keep these accesses volatile.
__device__ void solve(Shared& sh, int nr, int n, int lane) {
  volatile int* u = sh.u;
  volatile int16_t* p = sh.p;
  nr = __builtin_amdgcn_readfirstlane(nr);
  n = __builtin_amdgcn_readfirstlane(n);
  const int m = n > nr ? n : nr;
  int v[4], minv[4], way[4];
  bool used[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = 0;
    p[lane + 64 * k] = -1;
    u[lane + 64 * k] = 0;
  }
  int longest = 0, steps = 0;
  for (int r = 0; r < nr; ++r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { minv[k] = kInf; way[k] = -1; used[k] = false; }
    int j0 = -1;
    for (;;) {
      ++steps;
      const int i0 = j0 < 0 ? r : (int)p[j0];
      const int ui0 = u[i0];
      const uint16_t* row = sh.cost + (int)sh.rowslot[i0] * kRow;
      unsigned long long key = ~0ull;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = lane + 64 * k;
        if (col == j0) used[k] = true;
        if (col < m && !used[k]) {
          const int cur = (col < n ? (int)row[col] : kDummy) - ui0 - v[k];
          if (cur < minv[k]) { minv[k] = cur; way[k] = j0; }
          const unsigned long long mine = ((unsigned long long)(unsigned)minv[k] << 32) | (unsigned)col;
          if (mine < key) key = mine;
        }
      }
      key = wave_min_key(key);                                               // an unused column always exists: m >= nr
      const int delta = (int)(unsigned)(key >> 32), j1 = (int)(unsigned)key;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = lane + 64 * k;
        if (col < m) {
          if (used[k]) { u[p[col]] += delta; v[k] -= delta; }                // the rows of used columns are distinct: no two lanes meet
          else minv[k] -= delta;
        }
      }
      if (lane == 0) u[r] += delta;
      j0 = j1;
      if ((unsigned)j0 >= (unsigned)m) { j0 = -1; break; }                   // cannot happen (m >= nr); never index past the tables
      if (p[j0] < 0) break;
    }
    int len = 0;
    while (j0 >= 0 && len <= m) {                                            // the rows along `way` move one column each
      const int k = j0 >> 6;
      const int w = k == 0 ? way[0] : k == 1 ? way[1] : k == 2 ? way[2] : way[3];
      const int j1 = __builtin_amdgcn_readlane(w, __builtin_amdgcn_readfirstlane(j0 & 63));
      const int16_t from = j1 < 0 ? (int16_t)r : p[j1];
      if (lane == 0) p[j0] = from;
      j0 = j1;
      ++len;
    }
    longest = len > longest ? len : longest;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = lane + 64 * k;
    if (col < n) {
      const int r = p[col];
      if (r >= 0) {
        const int slot = sh.rowslot[r];
        if (sh.cost[slot * kRow + col] < kDummy) { sh.det_slot[col] = (int16_t)slot; sh.slot_det[slot] = (int16_t)col; }
      }
    }
  }
  if (lane == 0) { sh.stat[0] = longest; sh.stat[1] = steps; }
}

__global__ __launch_bounds__(kT) void track_frames_kernel(TrackArgs A) {
  __shared__ Shared sh;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const size_t seq = blockIdx.x;
  unsigned char* base = A.state + seq * MDCV_TRACK_STATE_BYTES;
  int* hdr = (int*)base;
  int* slots = hdr + kHdr;
  double* kf = (double*)(base + 4 * (kHdr + 6 * kT));

  // ---- the state, loaded once: uniform counters and thread t's slot
  int frames = hdr[0], next_id = hdr[1], dropped = hdr[2], longest = hdr[3], most_steps = hdr[4];
  int live = slots[t], id = slots[kT + t], cls = slots[2 * kT + t], tsu = slots[3 * kT + t], hits = slots[4 * kT + t],
      streak = slots[5 * kT + t];
  double x[7], pa[3], pb[3], pc[3], pr;
#pragma unroll
  for (int i = 0; i < 7; ++i) x[i] = kf[i * kT + t];
#pragma unroll
  for (int i = 0; i < 3; ++i) { pa[i] = kf[(7 + 3 * i) * kT + t]; pb[i] = kf[(8 + 3 * i) * kT + t]; pc[i] = kf[(9 + 3 * i) * kT + t]; }
  pr = kf[16 * kT + t];
  const double qv[3] = {1e-2, 1e-2, 1e-4}, rv[3] = {1.0, 1.0, 10.0};
  const size_t out0 = seq * (size_t)A.F * (size_t)A.K;

  for (int f = 0; f < A.F; ++f) {
    int n = A.count[seq * A.count_seq + f * A.count_frame];
    n = n < 0 ? 0 : n;
    n = n > A.K ? A.K : n;
    n = n > kT ? kT : n;
    // ---- A: the frame's boxes into LDS; predict
    bool good = false;
    int mycls = 0;
    if (t < n) {
      const double* b = A.boxes + seq * A.box_seq + f * A.box_frame + 4 * (size_t)t;
      const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
      sh.box[t][0] = b0; sh.box[t][1] = b1; sh.box[t][2] = b2; sh.box[t][3] = b3;
      good = __builtin_isfinite(b0) && __builtin_isfinite(b1) && __builtin_isfinite(b2) && __builtin_isfinite(b3) && b2 - b0 > 0.0 &&
             b3 - b1 > 0.0;
      if (A.cls) mycls = A.cls[seq * A.cls_seq + f * A.cls_frame + t];
    }
    sh.good[t] = good;
    sh.dcls[t] = mycls;
    sh.det_slot[t] = -1; sh.slot_det[t] = -1; sh.birth[t] = -1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (live) {
      if (x[2] + x[6] <= 0.0) x[6] = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        x[i] = x[i] + x[4 + i];
        const double na = ((pa[i] + pb[i]) + (pb[i] + pc[i])) + 1.0, nb = pb[i] + pc[i], nc = pc[i] + qv[i];
        pa[i] = na; pb[i] = nb; pc[i] = nc;
      }
      pr = pr + 1.0;
      ++tsu;
      const double w = sqrt(x[2] * x[3]), h = x[2] / w;
      a0 = x[0] - w / 2.0; a1 = x[1] - h / 2.0; a2 = x[0] + w / 2.0; a3 = x[1] + h / 2.0;
    }
    __syncthreads();

    // ---- B: thread t fills row t; the rows with an admissible box are numbered in slot order
    bool has = false;
    if (live) {
      const double ta = (a2 - a0) * (a3 - a1);
      uint16_t* row = sh.cost + t * kRow;
      for (int j = 0; j < n; ++j) {
        int c = kDummy;
        if (sh.good[j] && (!A.cls || sh.dcls[j] == cls)) {
          const double b0 = sh.box[j][0], b1 = sh.box[j][1], b2 = sh.box[j][2], b3 = sh.box[j][3];
          const double xx1 = a0 > b0 ? a0 : b0, yy1 = a1 > b1 ? a1 : b1, xx2 = a2 < b2 ? a2 : b2, yy2 = a3 < b3 ? a3 : b3;
          double iw = xx2 - xx1, ih = yy2 - yy1;
          iw = iw > 0.0 ? iw : 0.0;
          ih = ih > 0.0 ? ih : 0.0;
          const double wh = iw * ih;
          if (wh > 0.0) {
            const double iou = wh / ((ta + (b2 - b0) * (b3 - b1)) - wh);
            if (iou >= A.iou_thres) {
              const double g = iou * 65536.0;
              c = kDummy - (g >= 65535.0 ? 65535 : (int)g);
              has = true;
            }
          }
        }
        row[j] = (uint16_t)c;
      }
    }
    const unsigned long long rows = ballot(has);
    if (lane == 0) sh.wave[0][wv] = __popcll(rows);
    __syncthreads();
    int before = 0, nr = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int c = sh.wave[0][k]; before += k < wv ? c : 0; nr += c; }
    if (has) sh.rowslot[before + lane_prefix(rows)] = (int16_t)t;
    __syncthreads();

    // ---- C: the assignment, wave 0; the others wait here
    if (wv == 0) solve(sh, nr, n, lane);
    __syncthreads();
    longest = sh.stat[0] > longest ? sh.stat[0] : longest;
    most_steps = sh.stat[1] > most_steps ? sh.stat[1] : most_steps;

    // ---- D: update or age every live slot; free slots and unmatched boxes are numbered
    if (live) {
      const int j = sh.slot_det[t];
      if (j >= 0) {
        const double b0 = sh.box[j][0], b1 = sh.box[j][1], b2 = sh.box[j][2], b3 = sh.box[j][3];
        const double w = b2 - b0, h = b3 - b1;
        const double z[4] = {b0 + w / 2.0, b1 + h / 2.0, w * h, w / h};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double y = z[i] - x[i], S = pa[i] + rv[i], k0 = pa[i] / S, k1 = pb[i] / S;
          x[i] = x[i] + k0 * y;
          x[4 + i] = x[4 + i] + k1 * y;
          pc[i] = pc[i] - k1 * pb[i];
          pb[i] = pb[i] - k0 * pb[i];
          pa[i] = pa[i] - k0 * pa[i];
        }
        const double k = pr / (pr + 10.0);
        x[3] = x[3] + k * (z[3] - x[3]);
        pr = pr - k * pr;
        tsu = 0; ++hits; ++streak;
      } else {
        streak = 0;
        if (tsu > A.max_age) live = 0;
      }
    }
    const bool is_free = !live && t < A.max_tracks;
    const bool wants = good && sh.det_slot[t] < 0;
    const unsigned long long fm = ballot(is_free), wm = ballot(wants);
    if (lane == 0) { sh.wave[1][wv] = __popcll(fm); sh.wave[2][wv] = __popcll(wm); }
    __syncthreads();
    int fbefore = 0, nfree = 0, wbefore = 0, nwant = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = sh.wave[1][k], d = sh.wave[2][k];
      fbefore += k < wv ? c : 0; nfree += c;
      wbefore += k < wv ? d : 0; nwant += d;
    }
    const int frank = fbefore + lane_prefix(fm), wrank = wbefore + lane_prefix(wm);
    if (is_free) sh.freeslot[frank] = (int16_t)t;
    __syncthreads();
    if (wants && wrank < nfree) {
      const int slot = sh.freeslot[wrank];
      sh.birth[slot] = (int16_t)t;
      sh.det_slot[t] = (int16_t)slot;
    }
    __syncthreads();
    // ---- births: the k-th free slot takes the k-th unmatched box and id next_id + k
    if (is_free && sh.birth[t] >= 0) {
      const int j = sh.birth[t];
      const double b0 = sh.box[j][0], b1 = sh.box[j][1], b2 = sh.box[j][2], b3 = sh.box[j][3];
      const double w = b2 - b0, h = b3 - b1;
      x[0] = b0 + w / 2.0; x[1] = b1 + h / 2.0; x[2] = w * h; x[3] = w / h; x[4] = 0.0; x[5] = 0.0; x[6] = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) { pa[i] = 10.0; pb[i] = 0.0; pc[i] = 1e4; }
      pr = 10.0;
      live = 1; id = next_id + frank; cls = sh.dcls[j]; tsu = 0; hits = 0; streak = 0;
    }
    sh.slot_id[t] = live ? id : -1;
    sh.slot_streak[t] = streak;
    __syncthreads();
    // ---- the frame's outputs: every entry of the K
    int* oid = A.track_id + out0 + (size_t)f * A.K;
    unsigned char* ofl = A.flags + out0 + (size_t)f * A.K;
    {
      int tid = -1, fl = 0;
      if (t < n) {
        const int s = sh.det_slot[t];
        if (s >= 0) {
          tid = sh.slot_id[s];
          fl = (sh.slot_streak[s] >= A.min_hits || frames < A.min_hits) ? MDCV_TRACK_CONFIRMED : 0;
        } else {
          fl = good ? MDCV_TRACK_DROPPED : MDCV_TRACK_BAD_BOX;
        }
      }
      if (t < A.K) { oid[t] = tid; ofl[t] = (unsigned char)fl; }
      for (int j = t + kT; j < A.K; j += kT) { oid[j] = -1; ofl[j] = 0; }
    }
    const int born = nwant < nfree ? nwant : nfree;
    next_id += born;
    dropped += nwant - born;
    ++frames;
  }

  // ---- the state, stored once
  if (t == 0) { hdr[0] = frames; hdr[1] = next_id; hdr[2] = dropped; hdr[3] = longest; hdr[4] = most_steps; }
  slots[t] = live; slots[kT + t] = id; slots[2 * kT + t] = cls; slots[3 * kT + t] = tsu; slots[4 * kT + t] = hits; slots[5 * kT + t] = streak;
#pragma unroll
  for (int i = 0; i < 7; ++i) kf[i * kT + t] = x[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { kf[(7 + 3 * i) * kT + t] = pa[i]; kf[(8 + 3 * i) * kT + t] = pb[i]; kf[(9 + 3 * i) * kT + t] = pc[i]; }
  kf[16 * kT + t] = pr;
}

}  // namespace

extern "C" {

long long mdcv_track_state_bytes(void) { return MDCV_TRACK_STATE_BYTES; }

int mdcv_track_frames(const double* boxes, long long box_seq, long long box_frame, const int* count, long long count_seq,
                      long long count_frame, const int* cls, long long cls_seq, long long cls_frame, int S, int F, int K, double iou_thres,
                      int max_age, int min_hits, int max_tracks, void* state, int* track_id, unsigned char* flags, void* stream) {
  if (S < 0 || F < 0 || K < 1 || K > MDCV_TRACK_MAX_K || !(iou_thres > 0.0 && iou_thres <= 1.0) || max_age < 0 || min_hits < 0) return MDCV_EARG;
  if (max_tracks < 1 || max_tracks > MDCV_TRACK_SLOTS) return MDCV_EARG;
  if (box_seq < 0 || box_frame < 0 || count_seq < 0 || count_frame < 0 || cls_seq < 0 || cls_frame < 0) return MDCV_EARG;
  if (!boxes || !count || !state || !track_id || !flags) return MDCV_EARG;
  if (S == 0 || F == 0) return MDCV_OK;
  TrackArgs a{boxes, box_seq, box_frame, count, count_seq, count_frame, cls, cls_seq, cls_frame, F, K, iou_thres, max_age, min_hits,
              max_tracks, (unsigned char*)state, track_id, flags};
  hipLaunchKernelGGL(track_frames_kernel, dim3((unsigned)S), dim3(kT), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCV_OK : (int)e;
}

}  // extern "C"
