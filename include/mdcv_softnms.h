/* libmdcv_softnms.so — C ABI of the opt-in Soft-NMS (Bodla et al. 2017) detection post-processing (csrc/soft_nms.hip).
 * An overlapping box is not deleted: its score decays by a function of the IoU, and the box with the highest CURRENT score is picked next.
 * The visiting order therefore changes after every pick, which the suppression matrix and the one-wave scan of mdcv_detect_post cannot
 * express; the scan here is a round loop of its own.
 *
 * The conventions are those of include/mdcv_hip.h and of the other opt-in libraries: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success,
 * MDCV_EARG for an argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a positive
 * hipError_t otherwise.  A header and a library of its own for the reason include/mdcv_cls.h gives.  The candidate key and its order, the
 * radix select, the rank sort and the fp32 arithmetic of one NMS pair are shared as source with mdcv_detect_post (csrc/nms_core.h).
 *
 * Meaning.  Every fp32 operation below is ONE operation rounding on its own (the unit is built without fma contraction).
 *   1. Candidates.  mdcv_detect_post_soft with class_aware = 0: mdcv_detect_post's rules -- a row of pred [B,N,5+C] is a candidate iff
 *      r[4] > conf_thres, its score is r[4], its class the first maximum of r[5 .. 5+C) (0 when C = 0), its box
 *      (cx - w/2, cy - h/2, cx + w/2, cy + h/2), area = (x2 - x1) * (y2 - y1).  With class_aware = 1: rules 1-5 of include/mdcv_mcdet.h --
 *      score = r[4] * the first-maximum class word, and both r[4] and the score must pass conf_thres.  In mdcv_soft_nms every box
 *      [n,4] (corners) is a candidate with scores[i] and classes[i].  key = (ord32(score) << 32) | index; the top_k largest keys enter
 *      the scan, and `rank` is a candidate's position in descending key order.
 *   2. One round.  Every live candidate has a current score s, at first its own score.  The round picks the live candidate with the
 *      largest ord32(s); equal s go to the smaller rank.  This is the existing visiting order, so without overlaps the output is the
 *      hard NMS's.
 *   3. Stopping.  With a soft method the scan ends when the pick has !(s > score_thres); the hard method ignores score_thres.  It also
 *      ends when no live candidate is left.
 *   4. Emitting.  The pick m is emitted with its current score and becomes dead.
 *   5. Decaying.  For every live j (with classes: only those with cls_j == cls_m), iou = inter / ((area_j - inter) + area_m) as in
 *      mdcv_nms (csrc/nms_core.h nms_pair_iou).
 *        MDCV_SNMS_HARD:     j dies iff !(iou <= nms_thres) -- the existing rule, NaN included.
 *        MDCV_SNMS_LINEAR:   iff iou > nms_thres, s_j = s_j * (1.0f - iou).
 *        MDCV_SNMS_GAUSSIAN: iff iou > 0, w = (float)exp(-((double)iou * (double)iou) / (double)sigma), s_j = s_j * w.
 *      A NaN iou (two degenerate boxes) changes nothing in the soft methods.
 *   6. Outputs in emission order (descending current score): out_prob / out_scores = the current score at emission, out_index / keep =
 *      the row index, out_boxes, out_cls, out_count / count; rows past the count are zeros (keep and out_scores: up to min(n, top_k)).
 *      With targets [B,T,5]: the label matching, out_correct and out_stats = (AP, recall, precision, valid) of mdcv_detect_post
 *      (class_aware = 0) or of rule 8 of include/mdcv_mcdet.h (class_aware = 1), applied to the emitted list in its order.
 * Consequence: with MDCV_SNMS_HARD every output equals mdcv_detect_post's / mdcv_detect_post_mc's, and keep / count equal mdcv_nms's /
 * mdcv_nms_mc's, bit for bit. */
#ifndef MDCV_SOFTNMS_H
#define MDCV_SOFTNMS_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif
#ifndef MDCV_NMS_MAX_TOPK
#define MDCV_NMS_MAX_TOPK 512
#endif
#define MDCV_SNMS_HARD 0
#define MDCV_SNMS_LINEAR 1
#define MDCV_SNMS_GAUSSIAN 2
#define MDCV_SNMS_MAX_CLASSES 65535 /* the per-row class travels between the two stages as 16 bits */

/* keys u64[n] | one 128-byte counter line */
long long mdcv_soft_nms_workspace_bytes(int n);

/* classes NULL: class-agnostic (every live box decays).  keep and out_scores: min(n, top_k) entries at least.  n == 0 writes *count = 0.
 * Two launches.  MDCV_EARG: n < 0, top_k outside 1..MDCV_NMS_MAX_TOPK, a NULL keep / out_scores / count / workspace, a NULL boxes /
 * scores with n > 0, an unknown method, sigma <= 0 or not finite with MDCV_SNMS_GAUSSIAN, a NaN score_thres. */
int mdcv_soft_nms(const float* boxes, const float* scores, const int* classes, int n, int method, float nms_thres, float sigma,
                  float score_thres, int top_k, long long* keep, float* out_scores, int* count, void* workspace, void* stream);

/* keys u64[B*N] | one counter per image, 128 bytes apart | class u16[B*N]; 0 for B or N < 1 */
long long mdcv_detect_post_soft_workspace_bytes(int B, int N);

/* The arguments of mdcv_detect_post, then method, sigma, score_thres and class_aware, then its seven outputs.  Three launches (counters,
 * candidates, one workgroup per image).  MDCV_EARG: a NULL pred / output / workspace, B or N < 1, B > 65535, C < 0 or
 * > MDCV_SNMS_MAX_CLASSES, C < 1 with class_aware, class_aware outside 0..1, T < 0, targets NULL with T != 0, top_k outside
 * 1..MDCV_NMS_MAX_TOPK, an unknown method, sigma <= 0 or not finite with MDCV_SNMS_GAUSSIAN, a NaN score_thres. */
int mdcv_detect_post_soft(const float* pred, int B, int N, int C, const float* targets, int T, float conf_thres, float nms_thres,
                          float iou_thres, float width, float height, int top_k, int method, float sigma, float score_thres,
                          int class_aware, float* out_boxes, float* out_prob, int* out_cls, long long* out_index,
                          unsigned char* out_correct, int* out_count, float* out_stats, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
