"""NumPy restatement of csrc/detmap.hip (mdcv_detmap_match, mdcv_detmap_finalize): COCOeval.evaluateImg per image, class, IoU threshold
and size range, then one precision / recall curve per (class, threshold, range) over the whole dataset.  Plain loops: the IoU by np.float32
operations in the order of csrc/nms_core.h's nms_pair_iou (detection = the kept box), the curve in Python integers and
fractions.Fraction, the final sum a float64 loop.  Nothing here is tuned for speed."""
from fractions import Fraction

import numpy as np

F = np.float32
FP, TP, IGNORED = 0, 1, 2
MAX_TOPK, MAX_GT, MAX_THR, MAX_RANGES, MAX_CLASSES, CHUNK = 512, 2048, 10, 4, 1024, 1024
COCO_THRESHOLDS = tuple(F(0.5) + F(0.05) * F(i) for i in range(10))


def area32(b):
    b = np.asarray(b, F)
    return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def iou32(det, gt):
    """nms_pair_iou(bi = det, ai, bj = gt, aj): every operation rounds to float32 on its own"""
    bi, bj = np.asarray(det, F), np.asarray(gt, F)
    ai, aj = area32(bi), area32(bj)
    xx1, yy1 = np.maximum(bj[..., 0], bi[..., 0]), np.maximum(bj[..., 1], bi[..., 1])
    xx2, yy2 = np.minimum(bj[..., 2], bi[..., 2]), np.minimum(bj[..., 3], bi[..., 3])
    ww, hh = np.maximum(xx2 - xx1, F(0)), np.maximum(yy2 - yy1, F(0))
    inter = ww * hh
    uni = (aj - inter) + ai
    with np.errstate(divide="ignore", invalid="ignore"):
        out = inter / uni
    assert out.dtype == F
    return out


def in_range(a, lo, hi):
    return bool(a >= F(lo) and a < F(hi))


def labels_to_pixels(rows, width, height, C):
    """the loader's zero-padded (class, cx, cy, w, h) rows -> corner boxes [T,4] float32 and classes [T] (-1: padding, or a class outside
    0..C-1), with the float32 operations of mdcv_detect_post (validate.py:105-110)"""
    rows = np.asarray(rows, F).reshape(-1, 5)
    W, H, two = F(width), F(height), F(2)
    boxes, cls = np.zeros((len(rows), 4), F), np.full(len(rows), -1, np.int64)
    for t, (lc, lx, ly, lw, lh) in enumerate(rows):
        if lx > 0 and ly > 0 and lw > 0 and lh > 0:
            boxes[t] = [F(F(lx - F(lw / two)) * W), F(F(ly - F(lh / two)) * H), F(F(lx + F(lw / two)) * W), F(F(ly + F(lh / two)) * H)]
            if lc >= 0 and lc < F(C):
                cls[t] = int(lc)
    return boxes, cls


def match_image(boxes, cls, count, gt_boxes, gt_cls, gt_ignore, thresholds, ranges, C, stats=None):
    """one image -> status [S,K] uint32 (two bits per threshold), n_gt [S,C].  boxes [K,4], cls [K] or None, count; gt_boxes [T,4],
    gt_cls [T] (an entry outside 0..C-1 is no ground truth) or None, gt_ignore [T] or None.  stats: a dict counting 'tp', 'fp', 'ignored',
    'fallback' (a detection that took an ignored ground truth) and 'ties' (a choice between equal IoUs)."""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    K = len(boxes)
    count = max(0, min(int(count), K))
    gt_boxes = np.asarray(gt_boxes, F).reshape(-1, 4)
    T = len(gt_boxes)
    cls = np.zeros(K, np.int64) if cls is None else np.asarray(cls).astype(np.int64)
    gt_cls = np.zeros(T, np.int64) if gt_cls is None else np.asarray(gt_cls).astype(np.int64)
    gt_ignore = np.zeros(T, bool) if gt_ignore is None else np.asarray(gt_ignore).astype(bool)
    J, S = len(thresholds), len(ranges)
    status, n_gt = np.zeros((S, K), np.uint32), np.zeros((S, C), np.int64)
    real = (gt_cls >= 0) & (gt_cls < C)
    g_area = area32(gt_boxes)
    with np.errstate(all="ignore"):
        iou = iou32(boxes[:count, None, :], gt_boxes[None, :, :]) if count and T else np.zeros((count, T), F)
    for s, (lo, hi) in enumerate(ranges):
        ign = np.array([bool(gt_ignore[t]) or not in_range(g_area[t], lo, hi) for t in range(T)], bool)
        for t in np.nonzero(real & ~ign)[0]:
            n_gt[s, gt_cls[t]] += 1
        for j, thr in enumerate(thresholds):
            taken = np.zeros(T, bool)
            for d in range(count):
                cand = real & ~taken & (gt_cls == cls[d]) & (iou[d] >= F(thr))
                if cand.any():
                    pool = cand & ~ign                                     # a non-ignored ground truth first
                    fallback = not pool.any()
                    if fallback:
                        pool = cand
                    best = iou[d][pool].max()
                    at = np.nonzero(pool & (iou[d] == best))[0]           # equal IoU: the higher index (COCO's `<` test)
                    taken[at[-1]] = True
                    st = IGNORED if fallback else TP
                    if stats is not None:
                        stats["ties"] = stats.get("ties", 0) + len(at) - 1
                        stats["fallback"] = stats.get("fallback", 0) + fallback
                else:
                    st = FP if in_range(area32(boxes[d]), lo, hi) else IGNORED
                if stats is not None:
                    name = ("fp", "tp", "ignored")[st]
                    stats[name] = stats.get(name, 0) + 1
                status[s, d] |= np.uint32(st << (2 * j))
    return status, n_gt


class Dataset:
    """the dataset buffers of mdcv_detmap_match, grown image by image"""

    def __init__(self, K, thresholds, ranges, C):
        self.K, self.C = int(K), int(C)
        self.thresholds = [F(t) for t in thresholds]
        self.ranges = [(F(lo), F(hi)) for lo, hi in ranges]
        self.stats = {}
        self.reset()

    def reset(self):
        self.score, self.cls, self.count, self.status = [], [], [], []
        self.n_gt = np.zeros((len(self.ranges), self.C), np.int64)

    def add_pixels(self, boxes, prob, cls, count, gt_boxes, gt_cls, gt_count, gt_ignore=None):
        boxes = np.asarray(boxes, F)
        B, K = boxes.shape[0], self.K
        assert boxes.shape[1] == K
        gt_boxes = np.asarray(gt_boxes, F).reshape(B, -1, 4)
        for b in range(B):
            n = max(0, min(int(count[b]), K))
            ng = max(0, min(int(gt_count[b]), gt_boxes.shape[1]))
            c = np.zeros(K, np.int64) if cls is None else np.asarray(cls[b]).astype(np.int64)
            st, ng_sc = match_image(boxes[b], c, n, gt_boxes[b, :ng], None if gt_cls is None else np.asarray(gt_cls[b])[:ng],
                                    None if gt_ignore is None else np.asarray(gt_ignore[b])[:ng], self.thresholds, self.ranges, self.C, self.stats)
            self._push(np.asarray(prob[b], F), c, n, st, ng_sc)

    def add_labels(self, boxes, prob, cls, count, targets, width, height):
        boxes = np.asarray(boxes, F)
        B, K = boxes.shape[0], self.K
        targets = np.asarray(targets, F).reshape(B, -1, 5)
        for b in range(B):
            n = max(0, min(int(count[b]), K))
            c = np.zeros(K, np.int64) if cls is None else np.asarray(cls[b]).astype(np.int64)
            gb, gc = labels_to_pixels(targets[b], width, height, self.C)
            st, ng_sc = match_image(boxes[b], c, n, gb, gc, None, self.thresholds, self.ranges, self.C, self.stats)
            self._push(np.asarray(prob[b], F), c, n, st, ng_sc)

    def _push(self, prob, c, n, st, ng_sc):
        score, cl = np.zeros(self.K, F), np.zeros(self.K, np.int32)
        score[:n], cl[:n] = prob[:n], c[:n]
        self.score.append(score), self.cls.append(cl), self.count.append(n), self.status.append(st)
        self.n_gt += ng_sc

    def buffers(self):
        """score [n,K], cls [n,K], count [n], status [S,n,K], n_gt [S,C]"""
        n, S = len(self.count), len(self.ranges)
        if n == 0:
            return np.zeros((0, self.K), F), np.zeros((0, self.K), np.int32), np.zeros(0, np.int32), np.zeros((S, 0, self.K), np.uint32), self.n_gt
        return (np.stack(self.score), np.stack(self.cls), np.array(self.count, np.int32),
                np.stack(self.status, axis=1).astype(np.uint32), self.n_gt)

    def finalize(self):
        return finalize(*self.buffers(), len(self.thresholds))


def sorted_slots(score, cls, count, C):
    """-> (slots in evaluation order, their classes, err): by class, then descending score; equal scores by image, then row (a stable
    sort over slot order).  A valid row whose score is NaN or not positive sets err and is left out."""
    score, cls = np.asarray(score, F), np.asarray(cls)
    n, K = score.shape
    keys, err = [], 0
    for i in range(n):
        for k in range(min(int(count[i]), K)):
            c = int(cls[i, k])
            if not 0 <= c < C:
                continue
            if not score[i, k] > 0:
                err |= 1
                continue
            keys.append(((c << 32) | (0xFFFFFFFF - int(score[i, k].view(np.uint32))), i * K + k))
    keys.sort()                                                           # the slot breaks ties: what a stable sort over slot order gives
    return [s for _, s in keys], [k >> 32 for k, _ in keys], err


def curve(statuses, n_gt):
    """the statuses of one (class, threshold, range) in evaluation order -> (q: 101 Fractions, total TP, non-ignored detections)"""
    pts, tp = [], 0
    for st in statuses:
        if st == IGNORED:
            continue
        tp += st == TP
        pts.append((tp, len(pts) + 1))
    env, best = [None] * len(pts), (0, 1)
    for i in range(len(pts) - 1, -1, -1):                                 # the suffix maximum of tp / nd, by cross-multiplication
        if pts[i][0] * best[1] > best[0] * pts[i][1]:
            best = pts[i]
        env[i] = best
    q = [Fraction(0, 1)] * 101
    if n_gt > 0:
        i = 0
        for k in range(101):
            while i < len(pts) and 100 * pts[i][0] < k * n_gt:
                i += 1
            if i < len(pts):
                q[k] = Fraction(env[i][0], env[i][1])
    return q, tp, len(pts)


def ap_of(q, n_gt):
    if n_gt <= 0:
        return np.float64(-1.0)
    total = np.float64(0.0)
    for f in q:                                                           # k = 0..100, in that order
        total = total + np.float64(f.numerator) / np.float64(f.denominator)
    return total / np.float64(101.0)


def finalize(score, cls, count, status, n_gt, J):
    """-> q [C,J,S,101,2] int64, tot [C,J,S,3] int64, ap [C,J,S] float64, err"""
    status = np.asarray(status, np.uint32)
    S, C = n_gt.shape
    slots, classes, err = sorted_slots(score, cls, count, C)
    flat = status.reshape(S, -1)
    q = np.zeros((C, J, S, 101, 2), np.int64)
    tot, ap = np.zeros((C, J, S, 3), np.int64), np.zeros((C, J, S), np.float64)
    for c in range(C):
        seg = [s for s, k in zip(slots, classes) if k == c]
        for j in range(J):
            for s in range(S):
                sts = [int(flat[s, slot] >> (2 * j)) & 3 for slot in seg]
                qs, tp, nd = curve(sts, int(n_gt[s, c]))
                q[c, j, s] = [(f.numerator, f.denominator) for f in qs]
                tot[c, j, s] = (n_gt[s, c], tp, nd)
                ap[c, j, s] = ap_of(qs, int(n_gt[s, c]))
    return q, tot, ap, err


# ------------------------------------------------------------------------------------------------------------------- test data
def random_batch(rng, B, K, T, C, ignore=True, empty_images=True):
    """B images on a coarse integer grid, so that equal IoUs and equal scores actually occur -> dict of boxes [B,K,4], prob [B,K]
    (descending inside an image, multiples of 1/256), cls [B,K], count [B], gt_boxes [B,T,4], gt_cls [B,T], gt_ignore [B,T], gt_count [B].
    Detections are copies of ground truth shifted by multiples of 4 px, or boxes of their own; some ground truth is duplicated (an exact
    IoU tie for whatever matches it); class C-1 never occurs when C > 1 (an empty class)."""
    nc = max(C - 1, 1)
    boxes, prob = np.zeros((B, K, 4), F), np.zeros((B, K), F)
    cls, count = np.zeros((B, K), np.int32), np.zeros(B, np.int32)
    gt, gcls = np.zeros((B, T, 4), F), np.zeros((B, T), np.int32)
    gign, gcount = np.zeros((B, T), np.uint8), np.zeros(B, np.int32)
    for b in range(B):
        ng = int(rng.integers(0, T + 1))
        n = int(rng.integers(0, K + 1))
        if b == 0:
            n, ng = K, T                                                  # the first image is full: every row, every ground truth
        if empty_images and b % 4 == 1:
            n = 0
        if empty_images and b % 4 == 2:
            ng = 0
        for t in range(ng):
            if t and rng.random() < 0.2:
                gt[b, t], gcls[b, t] = gt[b, t - 1], gcls[b, t - 1]                      # the same box again
            else:
                x0, y0 = 8 * rng.integers(0, 8, 2)
                w, h = 8 * rng.integers(1, 4, 2)
                gt[b, t], gcls[b, t] = (x0, y0, x0 + w, y0 + h), rng.integers(0, nc)
            gign[b, t] = ignore and rng.random() < 0.2
        for k in range(n):
            if ng and rng.random() < 0.7:
                t = int(rng.integers(0, ng))
                dx, dy = 4 * rng.integers(-1, 2, 2)
                boxes[b, k] = gt[b, t] + np.array([dx, dy, dx, dy], F)
                cls[b, k] = gcls[b, t] if rng.random() < 0.9 else rng.integers(0, nc)
            else:
                x0, y0 = 4 * rng.integers(0, 16, 2)
                w, h = 4 * rng.integers(1, 8, 2)
                boxes[b, k], cls[b, k] = (x0, y0, x0 + w, y0 + h), rng.integers(0, nc)
        prob[b, :n] = -np.sort(-rng.integers(1, 256, n)) / F(256)
        count[b], gcount[b] = n, ng
    return dict(boxes=boxes, prob=prob, cls=cls, count=count, gt_boxes=gt, gt_cls=gcls, gt_ignore=gign, gt_count=gcount)


def labels_of(batch, side=64):
    """the pixel ground truth of `random_batch` as the loader's zero-padded rows [B,T,5] for a side x side input (exact: the grid is in
    multiples of 4 px and side is a power of two); rows past gt_count, and every ignored row, become padding"""
    g, n = batch["gt_boxes"], batch["gt_count"]
    B, T = g.shape[:2]
    rows = np.zeros((B, T, 5), F)
    for b in range(B):
        for t in range(int(n[b])):
            if batch["gt_ignore"][b, t]:
                continue                                                  # a zero row in the middle: padding, not a ground truth
            x0, y0, x1, y1 = g[b, t]
            rows[b, t] = (batch["gt_cls"][b, t], (x0 + x1) / 2 / side, (y0 + y1) / 2 / side, (x1 - x0) / side, (y1 - y0) / side)
    return rows
