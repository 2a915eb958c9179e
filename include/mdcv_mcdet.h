/* libmdcv_mcdet.so — C ABI of the opt-in class-aware detection post-processing (csrc/detect_mc.hip): the multi-class
 * counterpart of mdcv_detect_post / mdcv_nms of include/mdcv_hip.h.  The class probability enters the score, the greedy NMS runs class by
 * class, and a detection matches labels of its own class only.
 *
 * The conventions are those of include/mdcv_hip.h and of the other opt-in libraries: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success,
 * MDCV_EARG for an argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a positive
 * hipError_t otherwise.  A header and a library of its own for the reason include/mdcv_cls.h gives.  The candidate key and its order, the
 * radix select, the rank sort and the fp32 arithmetic of one NMS pair are shared as source with mdcv_detect_post (csrc/nms_core.h).
 *
 * Meaning.  The result is compared with `==`, so every fp32 operation below is ONE operation rounding on its own (the unit is built
 * without fma contraction).  pred is [B,N,5+C], row r = (cx, cy, w, h, conf, class words...).  For image b and row n:
 *   1. k* is the class mdcv_detect_post reports in `cls`: the first maximum of r[5 .. 5+C), by its comparisons in its order.
 *   2. score = r[4] * r[5 + k*], one fp32 product.
 *   3. the row is a candidate iff r[4] > conf_thres and score > conf_thres (NaN fails either test).  One candidate per row at most.
 *   4. key = (ord32(score) << 32) | n; candidates are visited by descending key, and the top_k largest keys enter the NMS.
 *   5. box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2), area = (x2 - x1) * (y2 - y1): mdcv_detect_post's.
 *   6. a kept candidate i removes a later candidate j iff cls_i == cls_j and !(iou <= nms_thres), iou = inter / ((area_j - inter) + area_i)
 *      as in mdcv_nms.  Class by class this is the greedy NMS over that class's candidates among the selected top_k.
 *   7. outputs in descending-key order: out_boxes [B,top_k,4], out_prob = score, out_cls = k*, out_index = n, out_count [B]; rows past
 *      out_count[b] are zeros.
 *   8. with targets [B,T,5] (class, cx, cy, w, h; a row is real when cx, cy, w, h are all > 0): for a detection of class k the best label
 *      is the first maximum of mdcv_detect_post's fp32 "+1" IoU over the real rows with l[0] == (float)k; without such a row the
 *      detection is not correct; out_correct iff that IoU > iou_thres and no earlier detection with the flag claimed the same row.
 *      out_stats [B,4] = (AP, recall, precision, valid) over all kept detections as mdcv_detect_post computes them, the label count
 *      being ALL real rows; valid = 0 (and zeros) when nothing is kept or no row is real.  targets NULL / T 0: correct and stats zeros.
 *   9. mdcv_nms_mc applies rule 6 to boxes [n,4] (corners), scores [n] and classes [n] (int32, any values), every box a candidate, and
 *      writes the kept indices in visiting order and their number. */
#ifndef MDCV_MCDET_H
#define MDCV_MCDET_H
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
#define MDCV_MCDET_MAX_CLASSES 65535 /* the per-row class travels between the two stages as 16 bits */

/* keys u64[B*N] | one counter per image, 128 bytes apart | class u16[B*N]; 0 for B or N < 1 */
long long mdcv_detect_post_mc_workspace_bytes(int B, int N);

/* The arguments of mdcv_detect_post, and its seven outputs.  Three launches (counters, candidates, one workgroup per image).
 * MDCV_EARG: a NULL pred / output / workspace, B or N < 1, B > 65535, C < 1 or > MDCV_MCDET_MAX_CLASSES, T < 0, targets NULL with T != 0,
 * top_k outside 1..MDCV_NMS_MAX_TOPK. */
int mdcv_detect_post_mc(const float* pred, int B, int N, int C, const float* targets, int T, float conf_thres, float nms_thres,
                        float iou_thres, float width, float height, int top_k, float* out_boxes, float* out_prob, int* out_cls,
                        long long* out_index, unsigned char* out_correct, int* out_count, float* out_stats, void* workspace,
                        void* stream);

long long mdcv_nms_mc_workspace_bytes(int n);

/* keep: min(n, top_k) entries at least.  n == 0 writes *count = 0.  MDCV_EARG: n < 0, top_k outside 1..MDCV_NMS_MAX_TOPK, a NULL keep /
 * count / workspace, a NULL boxes / scores / classes with n > 0. */
int mdcv_nms_mc(const float* boxes, const float* scores, const int* classes, int n, float overlap, int top_k, long long* keep, int* count,
                void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
