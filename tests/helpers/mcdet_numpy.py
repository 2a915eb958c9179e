"""Class-aware detection post-processing restated in float32 NumPy, rule by rule as include/mdcv_mcdet.h numbers them; the greedy NMS of
each class is the oracle's (oracle/postprocess_oracle.py `nms`, pinned to the reference), the matching is restated from its loop."""
import numpy as np

from oracle import postprocess_oracle as PO

F = np.float32


def build(B, N, C, T, conf, quant, seed, span=416.0):
    """the small input builder: label clusters, mostly of the label's class, over a random background; class 0 the most frequent"""
    rng = np.random.default_rng(seed)
    tg, out = np.zeros((B, T, 5), F), np.zeros((B, N, 5 + C), F)
    for b in range(B):
        n = T if b != 1 else max(T - 2, 1)
        tg[b, :n, 0] = np.minimum(rng.integers(0, C, n), rng.integers(0, C, n))
        tg[b, :n, 1:3], tg[b, :n, 3:5] = rng.random((n, 2)) * 0.8 + 0.1, rng.random((n, 2)) * 0.25 + 0.05
        out[b, :, 0:2], out[b, :, 2:4] = rng.random((N, 2)) * span, rng.random((N, 2)) * 80 + 4
        out[b, :, 4] = rng.random(N) * (0.6 if b != 1 else conf * 0.9)          # image 1: few candidates
        out[b, :, 5:] = rng.random((N, C))
        rows, r = rng.permutation(N), 0
        for lab in tg[b, :n]:
            for _ in range(int(rng.integers(3, 9))):
                i, r = rows[r], r + 1
                k = int(lab[0]) if rng.random() < 0.7 else int(rng.integers(0, C))
                out[b, i, 0:4] = lab[1:5] * span * (1 + 0.06 * rng.standard_normal(4))
                out[b, i, 4], out[b, i, 5:] = 0.7 + 0.3 * rng.random(), out[b, i, 5:] * 0.5
                out[b, i, 5 + k] = 0.9 + 0.1 * rng.random()
        out[b, ::97, 2:4] = 0                                  # zero-area boxes: 0/0 IoU among themselves
        out[b, 0:194:97, 0:2], out[b, 0:194:97, 4], out[b, 0:194:97, 5:] = 100.0, 0.95, out[b, 0, 5:]
        if B >= 3 and b == B - 1:
            out[b, :, 4] = conf * 0.5                          # nothing passes
    if quant:
        out[..., 4:] = np.round(out[..., 4:] / quant) * quant
    out[0, 7, 4] = np.nan
    return out.astype(F), tg


def _keys(score, n):
    u = score.view(np.uint32).astype(np.uint64)
    o = np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000)
    return (o << np.uint64(32)) | n.astype(np.uint64)


def select(boxes, score, cls, rows, overlap, top_k):
    """rules 4 and 6 -> (kept, selected) as positions into `rows`, most confident first; the oracle visits ties by descending index"""
    sel = np.argsort(_keys(score, rows))[::-1][:top_k]
    kept = []
    for c in np.unique(cls[sel]):
        m = np.sort(sel[cls[sel] == c])
        kept.extend(m[PO.nms(boxes[m], score[m], overlap, len(m))])
    kept = np.asarray(kept, np.int64)
    return kept[np.argsort(_keys(score[kept], rows[kept]))[::-1]], sel


def restate(det, labels, conf_thres, nms_thres, iou_thres, width, height, top_k):
    """one image -> the fields of `Detections`, and what the test asserts about its own inputs (segments, the two class situations)"""
    det, labels = np.asarray(det, F), np.asarray(labels, F)
    k = np.argmax(det[:, 5:], axis=1)                                                       # rule 1: first maximum
    with np.errstate(invalid="ignore"):
        score = (det[:, 4] * det[np.arange(len(det)), 5 + k]).astype(F)                     # rule 2
        obj = det[:, 4] > F(conf_thres)
        rows = np.nonzero(obj & (score > F(conf_thres)))[0]                                 # rule 3
    d = det[rows]
    half = (d[:, 2:4] / F(2)).astype(F)
    corner = np.concatenate([d[:, 0:2] - half, d[:, 0:2] + half], axis=1).astype(F)         # rule 5
    kept, sel = select(corner, score[rows], k[rows], rows, nms_thres, top_k)
    n = len(kept)
    out = dict(count=n, index=rows[kept], boxes=corner[kept], prob=score[rows][kept], cls=k[rows][kept].astype(np.int32),
               correct=np.zeros(n, np.uint8), stats=np.zeros(4, F), n_cand=len(rows), conf_only=int(obj.sum()) - len(rows),
               seg_len=np.unique(k[rows][sel], return_counts=True)[1], cross_keep=False, wrong_class=False)
    out["seg_start"] = np.cumsum(out["seg_len"]) - out["seg_len"]
    b, c = out["boxes"], out["cls"]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F)
    for i in range(n):                                                                      # kept pairs of different classes above nms_thres
        w = np.maximum(np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]), F(0))
        h = np.maximum(np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]), F(0))
        with np.errstate(invalid="ignore", divide="ignore"):
            out["cross_keep"] |= bool(((w * h / ((area[i + 1:] - w * h) + area[i]) > F(nms_thres)) & (c[i + 1:] != c[i])).any())
    lab = labels[(labels[:, 1:5] <= 0).sum(axis=1) == 0]
    if n == 0 or len(lab) == 0:
        return out
    tb = PO.xywh2xyxy(lab[:, 1:5])                                                          # rule 8, from postprocess_image's loop
    tb *= np.array([width, height, width, height], F)
    ious = PO.corner_iou_plus1(b[:, None, :], tb[None, :, :])
    detected = np.zeros(len(lab), bool)
    for i in range(n):
        own = np.nonzero(lab[:, 0] == F(c[i]))[0]
        if len(own):
            best = own[np.argmax(ious[i, own])]
            if ious[i, best] > F(iou_thres) and not detected[best]:
                out["correct"][i], detected[best] = 1, True
        out["wrong_class"] |= bool(not out["correct"][i] and (ious[i, lab[:, 0] != F(c[i])] > F(iou_thres)).any())
    out["stats"] = np.array([*PO.average_precision(out["correct"], out["prob"], len(lab)), 1], F)
    return out
