/* libmdcv_softtiles.so — C ABI of the opt-in soft cross-tile merge (csrc/detect_tiles_soft.hip): Soft-NMS (Bodla et al. 2017)
 * carried across tile borders.  The tiles' detections of a frame become one list per frame as in mdcv_detect_merge_tiles /
 * mdcv_detect_merge_tiles_mc, but a box that overlaps a pick of ANOTHER tile is not deleted: its score decays, and the box with the highest
 * CURRENT score is picked next, as in mdcv_detect_post_soft (include/mdcv_softnms.h).  It is the join behind
 * `TiledFrameDetector(..., nms="linear" | "gaussian", tile_merge="soft" | "soft_per_class")`: the far cone inside the near cone's box that
 * the tiles' soft scans kept is not deleted at the join.
 *
 * The conventions are those of include/mdcv_hip.h and of the other opt-in libraries: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success,
 * MDCV_EARG for an argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a positive
 * hipError_t otherwise.  A header and a library of its own for the reason include/mdcv_cls.h gives.  The candidate key and its order, the
 * radix select, the rank sort and the fp32 arithmetic of one NMS pair are shared as source with mdcv_detect_merge_tiles (csrc/nms_core.h).
 *
 * Meaning.  Every fp32 operation below is ONE operation rounding on its own (the unit is built without fma contraction).  The inputs are
 * mdcv_detect_merge_tiles_mc's: tile_boxes [T,K,4], tile_prob [T,K], tile_cls [T,K] int32, tile_count [T], the tile table on the host and
 * its device copy -- as mdcv_detect_post_soft writes its outputs for T tiles (tile_prob then holds the tiles' decayed scores).  For frame b:
 *   1. Candidates and order: rules 1-2 of mdcv_detect_merge_tiles, unchanged.  The tiles of b, their validation on the device copy (a
 *      frame whose tiles fail, or that has none, gets count 0), the candidates (t, k) with k < min(max(tile_count[t], 0), K), the key
 *      (ord32(tile_prob[t,k]) << 32) | ~c with c = (t - first tile of b) * K + k, the global cut to the top_k largest keys; `rank` is a
 *      candidate's position in descending key order (descending score, equal scores by ascending tile, then ascending slot).  Corner j =
 *      (float)((double)tile_boxes[t,k,j] + (double)off), off_x for j = 0, 2 and off_y for j = 1, 3 (one rounding); area = (x2 - x1) *
 *      (y2 - y1).  With class_aware = 1 the class of (t, k) is tile_cls[t*K + k], int32, ANY value; only the selected candidates' words are
 *      read.  With class_aware = 0, tile_cls and out_cls may be NULL and are not touched.
 *   2. Rounds (MDCV_SNMS_LINEAR, MDCV_SNMS_GAUSSIAN), as rules 2-4 of include/mdcv_softnms.h.  Every live candidate has a current score
 *      s, at first tile_prob.  A round picks the live candidate with the largest ord32(s); equal s go to the smaller rank.  The scan ends
 *      when the pick has !(s > score_thres), or when nobody is live.  The pick m is emitted with its current score and dies.
 *   3. Decay.  For every live j with tile_j != tile_m (with class_aware = 1: and cls_j == cls_m), iou = inter / ((area_j - inter) + area_m)
 *      as in mdcv_nms (csrc/nms_core.h nms_pair_iou).  Then, in this order:
 *        the seam rule, hard in every method: if contain_thres >= 0 and !(inter / min(area_j, area_m) <= contain_thres), j dies (a NaN
 *          ratio removes j too, as in the existing merges).  The half of a cone that a tile edge cut off is not a second cone; decaying it
 *          would keep it;
 *        otherwise MDCV_SNMS_LINEAR:   iff iou > overlap, s_j = s_j * (1.0f - iou);
 *                  MDCV_SNMS_GAUSSIAN: iff iou > 0, s_j = s_j * (float)exp(-((double)iou * (double)iou) / (double)sigma).
 *        A NaN iou changes nothing.
 *      Pairs of the SAME tile are never touched: the tile's own soft scan (mdcv_detect_post_soft) has already decayed them against each
 *      other, and a second decay would punish a cone twice for one neighbour.
 *   4. MDCV_SNMS_HARD.  The scan visits the ranks in order and tests ALL pairs, those of one tile included, with rule 4 of
 *      include/mdcv_mctiles.h: a kept i removes a later j iff (class_aware = 0 or cls_i == cls_j) and at least one of !(iou <= overlap);
 *      contain_thres >= 0 and tile_i != tile_j and !(inter / min(area_j, area_i) <= contain_thres).  score_thres is ignored.  Consequence:
 *      with class_aware = 0 every output equals mdcv_detect_merge_tiles's, with class_aware = 1 mdcv_detect_merge_tiles_mc's, bit for bit.
 *      The method is there to pin this entry to those two; it runs the round loop and is 9-13 times slower than they are: a
 *      caller who wants a hard merge calls them.
 *   5. Outputs in emission order: out_boxes [B,top_k,4], out_prob [B,top_k] = the score at emission, out_src [B,top_k,2] = (tile index in
 *      the batch, slot in the tile), out_count [B], and with class_aware = 1 out_cls [B,top_k] int32.  Every slot of a frame is written:
 *      past out_count[b] zeros, out_src (-1, -1), out_cls 0.
 * One launch, grid (B), one 1024-thread workgroup per frame, no workspace, no host read: it can be captured into a graph. */
#ifndef MDCV_SOFTTILES_H
#define MDCV_SOFTTILES_H
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
#ifndef MDCV_TILE_DESC
#define MDCV_TILE_DESC 4
#define MDCV_TILE_MAX_PER_FRAME 64
#define MDCV_TILE_MAX_OFFSET 16777216
#endif
#ifndef MDCV_SNMS_HARD
#define MDCV_SNMS_HARD 0
#define MDCV_SNMS_LINEAR 1
#define MDCV_SNMS_GAUSSIAN 2
#endif

/* The arguments of mdcv_detect_merge_tiles_mc, then method, sigma, score_thres and class_aware, then the
 * stream.  MDCV_EARG: everything mdcv_detect_merge_tiles_mc lists (B, T or K < 0, B > 65535, K or top_k > MDCV_NMS_MAX_TOPK, top_k < 1, a
 * NULL tiles_host with T > 0, a host tile table with a frame outside 0..B-1 or descending, more than MDCV_TILE_MAX_PER_FRAME tiles of one
 * frame, an offset beyond +-MDCV_TILE_MAX_OFFSET or a last word that is not 0), an unknown method, sigma <= 0 or not finite with
 * MDCV_SNMS_GAUSSIAN, a NaN score_thres, class_aware outside 0..1.  B == 0, T == 0 or K == 0: MDCV_OK, nothing is enqueued or written.
 * Otherwise a NULL device pointer is MDCV_EARG -- tile_cls and out_cls with class_aware = 1 only. */
int mdcv_detect_merge_tiles_soft(const float* tile_boxes, const float* tile_prob, const int* tile_cls, const int* tile_count,
                                 const int* tiles_host, const int* tiles, int T, int K, int B, float overlap, float contain_thres,
                                 int top_k, float* out_boxes, float* out_prob, int* out_cls, int* out_src, int* out_count, int method,
                                 float sigma, float score_thres, int class_aware, void* stream);

#ifdef __cplusplus
}
#endif
#endif
