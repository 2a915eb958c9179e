/* libmdcv_mctiles.so — C ABI of the opt-in class-aware cross-tile merge (csrc/detect_tiles_mc.hip): the multi-class
 * counterpart of mdcv_detect_merge_tiles of include/mdcv_hip.h.  The tiles' detections of a frame become one list per frame as there, but
 * a kept box removes later boxes of its OWN class only, as mdcv_detect_post_mc / mdcv_nms_mc (include/mdcv_mcdet.h) remove them inside a
 * tile.  It is the join behind `TiledFrameDetector(..., class_aware=True, tile_merge="per_class")`.
 *
 * The conventions are those of include/mdcv_hip.h and of the other opt-in libraries: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success,
 * MDCV_EARG for an argument error (checked on the host before any GPU call, so reachable on a machine without a GPU), a positive
 * hipError_t otherwise.  A header and a library of its own for the reason include/mdcv_cls.h gives.  The candidate key and its order, the
 * radix select, the rank sort and the fp32 arithmetic of one NMS pair are shared as source with mdcv_detect_merge_tiles (csrc/nms_core.h).
 *
 * Meaning.  The result is compared with `==`, so every fp32 operation below is ONE operation rounding on its own (the unit is built
 * without fma contraction).  The inputs are mdcv_detect_merge_tiles's -- tile_boxes [T,K,4], tile_prob [T,K], tile_count [T], the tile
 * table on the host and its device copy -- and tile_cls [T,K] int32, as mdcv_detect_post_mc writes out_cls for T tiles.  For frame b:
 *   1. the tiles of b, their validation on the device copy (a frame whose tiles fail, or that has none, gets count 0), the candidates
 *      (t, k) with k < min(max(tile_count[t], 0), K), their keys, the visiting order (descending score, equal scores by ascending tile,
 *      then ascending slot) and the cut to the top_k largest keys: mdcv_detect_merge_tiles's, unchanged.  The cut is global: it is made
 *      before any class is looked at.
 *   2. corner j of a selected candidate = (float)((double)tile_boxes[t,k,j] + (double)off), off_x for j = 0, 2 and off_y for j = 1, 3 (one
 *      rounding); area = (x2 - x1) * (y2 - y1): mdcv_detect_merge_tiles's.
 *   3. the class of candidate (t, k) is tile_cls[t*K + k]: int32, ANY value (negative ones included), as in mdcv_nms_mc.  Only the selected
 *      candidates' words are read.
 *   4. a kept candidate i removes a later candidate j iff cls_i == cls_j and at least one of
 *        !(iou <= overlap), iou = inter / ((area_j - inter) + area_i) as in mdcv_nms (a NaN leaves);
 *        contain_thres >= 0 and tile_i != tile_j and !(inter / min(area_j, area_i) <= contain_thres)   (the seam rule; a NaN leaves).
 *      So the seam rule acts within a class only, too: class by class the result is what mdcv_detect_merge_tiles would keep from that
 *      class's candidates among the selected top_k.  A cut-off half cone that a tile gave ANOTHER class than the neighbouring tile gave the
 *      whole cone therefore survives; a seam rule across classes is not part of this entry.
 *   5. outputs in descending-key order of the kept candidates: out_boxes [B,top_k,4], out_prob [B,top_k], out_src [B,top_k,2] = (tile
 *      index in the batch, slot in the tile) and out_count [B] as mdcv_detect_merge_tiles writes them, and out_cls [B,top_k] int32.  Every
 *      slot of a frame is written: past out_count[b] zeros, out_src (-1, -1), out_cls 0.
 * One launch, grid (B), one 1024-thread workgroup per frame, no workspace, no host read: it can be captured into a graph. */
#ifndef MDCV_MCTILES_H
#define MDCV_MCTILES_H
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

/* MDCV_EARG, as mdcv_detect_merge_tiles: B, T or K < 0, B > 65535, K or top_k > MDCV_NMS_MAX_TOPK, top_k < 1, a NULL tiles_host with
 * T > 0, a host tile table with a frame outside 0..B-1 or descending, more than MDCV_TILE_MAX_PER_FRAME tiles of one frame, an offset
 * beyond +-MDCV_TILE_MAX_OFFSET or a last word that is not 0.  B == 0, T == 0 or K == 0: MDCV_OK, nothing is enqueued or written.
 * Otherwise a NULL device pointer is MDCV_EARG, tile_cls and out_cls included. */
int mdcv_detect_merge_tiles_mc(const float* tile_boxes, const float* tile_prob, const int* tile_cls, const int* tile_count,
                               const int* tiles_host, const int* tiles, int T, int K, int B, float overlap, float contain_thres,
                               int top_k, float* out_boxes, float* out_prob, int* out_cls, int* out_src, int* out_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
