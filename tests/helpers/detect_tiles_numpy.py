"""NumPy restatement of csrc/detect_tiles.hip (mdcv_detect_merge_tiles): the detections of a frame's tiles become one list per frame.

Per frame b, over its tiles t (contiguous rows of the tile table, words: frame, off_x, off_y, 0):
  1. candidates (t, k), k < min(tile_count[t], K); corner j = float32(float64(tile_boxes[t,k,j]) + float64(off)), off_x for j = 0, 2 and
     off_y for j = 1, 3 (one rounding); score tile_prob[t,k];
  2. visiting order: descending score, equal scores by ascending tile, then ascending slot; only the first top_k are considered
     (utils/nms.py:26 `idx[-top_k:]`);
  3. the greedy scan of utils/nms.py:31-61 in float32, every operation rounded on its own: area (x2 - x1) * (y2 - y1), the clamps,
     inter = w * h, union = (rem_area - inter) + area_i, IoU = inter / union; a remaining j stays behind a kept i iff IoU <= overlap (a NaN
     leaves) and, when contain_thres >= 0 and tile(j) != tile(i), also inter / min(area_j, area_i) <= contain_thres (the seam rule);
  4. kept boxes in visiting order; slots past the count hold zeros, their src (-1, -1).
The clamps are C's fmaxf / fminf (np.fmax / np.fmin: a NaN operand loses), as the kernels compute them.
"""
import numpy as np

F = np.float32
MAX_TILES_PER_FRAME = 64         # MDCV_TILE_MAX_PER_FRAME
MAX_TOPK = 512                   # MDCV_NMS_MAX_TOPK
MAX_OFFSET = 1 << 24             # MDCV_TILE_MAX_OFFSET


def ord32(scores):
    """float32 -> uint32 whose unsigned order is the kernels' score order (NaN with sign 0 highest, -0 below +0)"""
    u = np.ascontiguousarray(scores, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def offset_boxes(boxes, off_x, off_y):
    """float32 [n,4] tile corners -> float32 [n,4] scaled-frame corners: one rounding of the float64 sum"""
    b = np.asarray(boxes, F).reshape(-1, 4).astype(np.float64)
    b[:, 0::2] += np.float64(off_x)
    b[:, 1::2] += np.float64(off_y)
    with np.errstate(all="ignore"):
        return b.astype(F)


def visiting_order(scores, tile, slot, top_k):
    """indices of the candidates in visiting order, cut to the first top_k"""
    order = np.lexsort((slot, tile, -ord32(scores).astype(np.int64)))        # last key first: score desc, tile asc, slot asc
    return order[:top_k]


def greedy_scan(boxes, tile, overlap, contain_thres):
    """boxes float32 [n,4] already in visiting order, tile [n] -> kept positions, in order"""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    n = len(boxes)
    overlap, seam = F(overlap), F(contain_thres) >= F(0)
    with np.errstate(all="ignore"):
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        alive = np.ones(n, bool)
        keep = []
        for i in range(n):
            if not alive[i]:
                continue
            keep.append(i)
            j = np.nonzero(alive[i + 1:])[0] + i + 1
            if not len(j):
                continue
            xx1, yy1 = np.fmax(boxes[j, 0], boxes[i, 0]), np.fmax(boxes[j, 1], boxes[i, 1])
            xx2, yy2 = np.fmin(boxes[j, 2], boxes[i, 2]), np.fmin(boxes[j, 3], boxes[i, 3])
            w, h = np.fmax(xx2 - xx1, F(0)), np.fmax(yy2 - yy1, F(0))
            inter = w * h
            union = (area[j] - inter) + area[i]
            stay = (inter / union) <= overlap                                # False for NaN
            if seam:
                small = np.where(area[j] < area[i], area[j], area[i])
                stay &= (tile[j] == tile[i]) | ((inter / small) <= F(contain_thres))
            alive[j[~stay]] = False
    assert area.dtype == F
    return np.array(keep, np.int64)


def merge_tiles(tile_boxes, tile_prob, tile_count, tiles, B, overlap, contain_thres, top_k):
    """-> out_boxes float32 [B,top_k,4], out_prob float32 [B,top_k], out_src int32 [B,top_k,2], out_count int32 [B]"""
    tile_boxes = np.asarray(tile_boxes, F)
    T, K = tile_boxes.shape[0], tile_boxes.shape[1]
    tile_prob = np.asarray(tile_prob, F).reshape(T, K)
    tiles = np.asarray(tiles, np.int32).reshape(T, 4)
    out_boxes = np.zeros((B, top_k, 4), F)
    out_prob = np.zeros((B, top_k), F)
    out_src = np.full((B, top_k, 2), -1, np.int32)
    out_count = np.zeros(B, np.int32)
    for b in range(B):
        boxes, prob, tile, slot = [], [], [], []
        for t in np.nonzero(tiles[:, 0] == b)[0]:
            n = min(max(int(tile_count[t]), 0), K)
            boxes.append(offset_boxes(tile_boxes[t, :n], tiles[t, 1], tiles[t, 2]))
            prob.append(tile_prob[t, :n])
            tile.append(np.full(n, t, np.int64))
            slot.append(np.arange(n, dtype=np.int64))
        if not boxes:
            continue
        boxes, prob, tile, slot = np.concatenate(boxes), np.concatenate(prob), np.concatenate(tile), np.concatenate(slot)
        order = visiting_order(prob, tile, slot, top_k)
        keep = order[greedy_scan(boxes[order], tile[order], overlap, contain_thres)]
        n = len(keep)
        out_boxes[b, :n], out_prob[b, :n], out_count[b] = boxes[keep], prob[keep], n
        out_src[b, :n, 0], out_src[b, :n, 1] = tile[keep], slot[keep]
    return out_boxes, out_prob, out_src, out_count


def table_ok(tiles, B):
    """the host validation of the tile table (MDCV_EARG when False)"""
    tiles = np.asarray(tiles, np.int64).reshape(-1, 4)
    f = tiles[:, 0]
    if len(f) == 0:
        return True
    if (f < 0).any() or (f >= B).any() or (np.diff(f) < 0).any() or (np.abs(tiles[:, 1:3]) > MAX_OFFSET).any() or tiles[:, 3].any():
        return False
    return int(np.bincount(f).max()) <= MAX_TILES_PER_FRAME
