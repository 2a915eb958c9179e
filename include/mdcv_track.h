/* libmdcv_track.so — C ABI of the opt-in tracker (csrc/track.hip): a SORT-style association of every frame's boxes with the
 * tracks of its sequence -- a constant-velocity Kalman filter per track, an optimal one-to-one assignment by IoU, track birth, confirmation
 * and death -- for whole sequences in one launch.  It is the consumer of the box tables behind `FrameDetector(..., track=)` and its
 * subclasses, and of `mdcv.yolo.track.track_boxes`.
 *
 * The conventions are those of include/mdcv_hip.h and of the other opt-in libraries: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success,
 * MDCV_EARG for an argument error (checked on the host before any GPU call), a positive hipError_t otherwise.  A header and a library of
 * its own for the reason include/mdcv_cls.h gives.
 *
 * The rule (tests/helpers/track_numpy.py restates it in float64 and exact integers).  Every floating-point operation below is one IEEE
 * double operation, rounded on its own, in the order written (csrc/track.hip is compiled without contraction); max(a, b) is
 * `a > b ? a : b` and min(a, b) is `a < b ? a : b`, so a NaN on the left gives way to the right.
 *
 * A sequence owns MDCV_TRACK_SLOTS slots, of which the first max_tracks are used, a frame counter, a next-id counter and a `dropped`
 * counter, all 0 in a fresh (all-zero) state block.  Frames are processed in order.  Frame f has n = min(max(count, 0), K,
 * MDCV_TRACK_SLOTS) boxes (x0, y0, x1, y1) and, with `cls`, a class per box.  A box is GOOD when its four words are finite and
 * x1 - x0 > 0 and y1 - y0 > 0; its measurement is w = x1 - x0, h = y1 - y0, z = (x0 + w / 2, y0 + h / 2, w * h, w / h).
 *
 *   1. Predict, every live slot.  State (cx, cy, s, r, vx, vy, vs); covariance in block form: (a, b, c) = (var position, covariance,
 *      var velocity) for each of (cx, vx), (cy, vy), (s, vs), and the variance pr of r.  If s + vs <= 0 then vs = 0.  Then for each pair:
 *      position = position + velocity; a' = ((a + b) + (b + c)) + 1; b' = b + c; c' = c + qv (from the old a, b, c), qv = 1e-2, 1e-2,
 *      1e-4; pr = pr + 1.  time_since_update rises by 1.  The predicted box: w = sqrt(s * r), h = s / w,
 *      (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2).
 *   2. IoU of predicted box A and good box B: iw = max(min(A.x1, B.x1) - max(A.x0, B.x0), 0), ih likewise, wh = iw * ih; unless wh > 0
 *      the pair is not admissible; IoU = wh / (((A.x1 - A.x0) * (A.y1 - A.y0) + (B.x1 - B.x0) * (B.y1 - B.y0)) - wh).  Admissible:
 *      IoU >= iou_thres and, with `cls`, the track's class (that of the box that opened it) equals the box's.  Gain q = 65535 when
 *      IoU * 65536 >= 65535, else (int)(IoU * 65536).  Cost: 65535 - q for an admissible pair, 65535 for every other.
 *   3. Assignment.  Rows: the live slots with at least one admissible box, in slot order (nr of them).  Columns: the n boxes, and
 *      dummy columns of cost 65535 up to m = max(n, nr).  Row by row, the shortest augmenting path with integer potentials u (rows) and
 *      v (columns), all 0 at the start: from the new row, repeat { mark the current column used (none at first); with i0 the row of the
 *      current column (the new row at first), minv[j] = min(minv[j], cost[i0][j] - u[i0] - v[j]) for every unused column j, remembering
 *      the current column as way[j] where it lowered minv[j]; delta = the least minv over unused columns, j1 its LOWEST column
 *      (strict <); u += delta for the new row and the rows of used columns, v -= delta for used columns, minv -= delta for unused
 *      ones; the current column = j1 } until j1 has no row; then the rows along `way` move one column each.  A pair assigned at cost
 *      65535 is unmatched on both sides.
 *   4. A matched slot is updated with its box's z: for each pair with measurement noise rv = 1, 1, 10: y = z - position; S = a + rv;
 *      k0 = a / S; k1 = b / S; position = position + k0 * y; velocity = velocity + k1 * y; c' = c - k1 * b; b' = b - k0 * b;
 *      a' = a - k0 * a; and k = pr / (pr + 10); r = r + k * (z.r - r); pr = pr - k * pr.  time_since_update = 0; hits and hit_streak
 *      rise by 1.  An unmatched live slot keeps its prediction, its hit_streak becomes 0, and it is freed when time_since_update >
 *      max_age.  Slots freed in a frame are free for that frame's births.
 *   5. Births.  The good boxes left unmatched, in box order, take the free slots below max_tracks in slot order, the k-th box the k-th
 *      slot with id next_id + k: state (z, 0, 0, 0), (a, b, c) = (10, 0, 1e4), pr = 10, hits = hit_streak = time_since_update = 0, the
 *      box's class.  A box without a slot gets id -1 and `dropped` rises; next_id rises by the number of births.
 *   6. Output per box j < n: track_id (-1 for a box that is not good or was dropped) and flags: MDCV_TRACK_CONFIRMED when the box has
 *      a track and (hit_streak >= min_hits or f < min_hits), f the sequence's frame counter before this frame; MDCV_TRACK_BAD_BOX;
 *      MDCV_TRACK_DROPPED.  Entries j >= n are -1 and 0.  The frame counter rises.
 *
 * State block of one sequence, MDCV_TRACK_STATE_BYTES: int32 header [16] = frames, next_id, dropped, the longest augmenting path so far
 * (columns on it), the most scan steps of one frame's assignment so far, 11 zeros; int32 [6][256] = live, id, cls, time_since_update,
 * hits, hit_streak per slot; double [17][256] = cx, cy, s, r, vx, vy, vs, then (a, b, c) of cx, of cy, of s, then pr.
 * One 256-thread workgroup per sequence, the frames in a loop inside it; no workspace, no host read: it can be captured into a graph. */
#ifndef MDCV_TRACK_H
#define MDCV_TRACK_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif
#define MDCV_TRACK_SLOTS 256
#define MDCV_TRACK_STATE_BYTES 41024          /* 64 + 6 * 256 * 4 + 17 * 256 * 8 */
#define MDCV_TRACK_CONFIRMED 1
#define MDCV_TRACK_BAD_BOX 2
#define MDCV_TRACK_DROPPED 4
#define MDCV_TRACK_MAX_K 65536

/* bytes of one sequence's state block (MDCV_TRACK_STATE_BYTES) */
long long mdcv_track_state_bytes(void);

/* boxes f64: box j of frame f of sequence s at boxes[s * box_seq + f * box_frame + 4 * j]; count i32 at count[s * count_seq + f *
 * count_frame]; cls i32 or NULL at cls[s * cls_seq + f * cls_frame + j] (strides in elements, >= 0); state [S] blocks of
 * MDCV_TRACK_STATE_BYTES, 8-byte aligned, read and written; track_id i32 [S,F,K] and flags u8 [S,F,K], every entry written -- all device
 * pointers.  MDCV_EARG: S < 0, F < 0, K < 1 or > MDCV_TRACK_MAX_K, iou_thres outside (0, 1], max_age < 0, min_hits < 0, max_tracks
 * outside 1..MDCV_TRACK_SLOTS, a negative stride, a NULL boxes, count, state, track_id or flags.  S == 0 or F == 0: MDCV_OK, nothing is
 * enqueued. */
int mdcv_track_frames(const double* boxes, long long box_seq, long long box_frame, const int* count, long long count_seq,
                      long long count_frame, const int* cls, long long cls_seq, long long cls_frame, int S, int F, int K, double iou_thres,
                      int max_age, int min_hits, int max_tracks, void* state, int* track_id, unsigned char* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
