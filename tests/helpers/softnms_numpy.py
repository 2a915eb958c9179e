"""Soft-NMS restated in plain NumPy, rule by rule as include/mdcv_softnms.h numbers them.  `dt` is the type of the scores, the weights and
the thresholds; the IoU is rule 5's: csrc/nms_core.h's float32 arithmetic, which the Gaussian rule then converts."""
import numpy as np

F, EPS = np.float32, 2.0 ** -23


def scene(n, seed, centres=12):
    """clustered boxes (centres, sigma 14 px, sides 18..60 px), scores uniform in [0.05, 0.99]"""
    rng = np.random.default_rng(seed)
    c = (rng.random((centres, 2)) * 380 + 18)[rng.integers(0, centres, n)] + rng.standard_normal((n, 2)) * 14
    half = rng.uniform(18, 60, (n, 2)) / 2
    return np.concatenate([c - half, c + half], 1).astype(F), rng.uniform(0.05, 0.99, n).astype(F)


def keys(score, index):
    u = score.view(np.uint32).astype(np.uint64)
    return (np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000) << np.uint64(32)) | index.astype(np.uint64)


def pair_iou(bm, am, b, a):
    with np.errstate(invalid="ignore", divide="ignore"):
        ww = np.maximum(np.minimum(b[:, 2], bm[2]) - np.maximum(b[:, 0], bm[0]), F(0))
        hh = np.maximum(np.minimum(b[:, 3], bm[3]) - np.maximum(b[:, 1], bm[1]), F(0))
        inter = ww * hh
        return inter / ((a - inter) + am)


def soft_nms(boxes, scores, classes, method, nms_thres, sigma, score_thres, top_k, dt=F):
    """rules 1-6 -> keep, the scores at emission, each emitted candidate's number of decays, and `margin`: the smallest ratio of a
    decision's gap (a pick to its runner-up and to score_thres, a linear IoU to nms_thres) to the error bound 2 d 2^-23 (one ulp at least)"""
    order = np.argsort(keys(scores, np.arange(len(scores))))[::-1][:top_k]                   # rule 1: rank order
    b, s = boxes[order], scores[order].astype(dt)
    cls = np.zeros(len(order), np.int64) if classes is None else classes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    live, d, margin = np.ones(len(order), bool), np.zeros(len(order), np.int64), np.inf
    err = lambda i: max(2 * d[i], 1) * EPS * abs(float(s[i])) + 1e-300  # noqa: E731
    keep, out, dec = [], [], []
    while live.any():
        cand = np.nonzero(live)[0]
        m = cand[np.argmax(s[cand])]                                                         # rule 2: first maximum = smaller rank
        rest = cand[cand != m]
        if method != "hard":
            margin = min(margin, abs(float(s[m]) - score_thres) / err(m))
            if len(rest) and (d[m] or d[rest[np.argmax(s[rest])]]):                          # two undecayed scores compare exactly
                r = rest[np.argmax(s[rest])]
                margin = min(margin, (float(s[m]) - float(s[r])) / (err(m) + err(r)))
        if method != "hard" and not s[m] > dt(score_thres):                                  # rule 3
            break
        keep.append(order[m]), out.append(s[m]), dec.append(d[m]), live.__setitem__(m, False)   # rule 4
        j = np.nonzero(live & (cls == cls[m]))[0]                                            # rule 5
        iou = pair_iou(b[m], area[m], b[j], area[j])
        with np.errstate(invalid="ignore"):
            if method == "hard":
                live[j[~(iou <= F(nms_thres))]] = False
                continue
            if method == "linear":
                hit, w = iou.astype(dt) > dt(nms_thres), dt(1) - iou.astype(dt)
                margin = min([margin, *(np.abs(iou[~np.isnan(iou)].astype(np.float64) - nms_thres) / EPS)])
            else:
                hit, w = iou > 0, np.exp(-(iou.astype(np.float64) * iou.astype(np.float64)) / np.float64(sigma)).astype(dt)
        s[j[hit]] = s[j[hit]] * w[hit]
        d[j[hit]] += 1
    return np.asarray(keep, np.int64), np.asarray(out, dt), np.asarray(dec, np.int64), margin


def postprocess(det, labels, conf_thres, nms_thres, iou_thres, width, height, top_k, method, sigma, score_thres, class_aware):
    """one image of detect_postprocess in float32 -> the fields of `Detections`; the matching is the oracle's loop (rule 6)"""
    from oracle import postprocess_oracle as PO
    det, labels = np.asarray(det, F), np.asarray(labels, F)
    k = np.argmax(det[:, 5:], axis=1)
    with np.errstate(invalid="ignore"):
        score = (det[:, 4] * det[np.arange(len(det)), 5 + k]).astype(F) if class_aware else det[:, 4]
        rows = np.nonzero((det[:, 4] > F(conf_thres)) & (score > F(conf_thres)))[0]
    half = (det[rows, 2:4] / F(2)).astype(F)
    corner = np.concatenate([det[rows, 0:2] - half, det[rows, 0:2] + half], axis=1).astype(F)
    keep, prob, _, _ = soft_nms(corner, score[rows], k[rows] if class_aware else None, method, nms_thres, sigma, score_thres, top_k)
    n, lab = len(keep), labels[(labels[:, 1:5] <= 0).sum(axis=1) == 0]
    out = dict(count=n, index=rows[keep], boxes=corner[keep], prob=prob, cls=k[rows][keep].astype(np.int32), correct=np.zeros(n, np.uint8),
               stats=np.zeros(4, F))
    if n == 0 or len(lab) == 0:
        return out
    tb = PO.xywh2xyxy(lab[:, 1:5]) * np.array([width, height, width, height], F)
    ious, detected = PO.corner_iou_plus1(out["boxes"][:, None, :], tb[None, :, :]), np.zeros(len(lab), bool)
    for i in range(n):
        own = np.nonzero(lab[:, 0] == F(out["cls"][i]))[0] if class_aware else np.arange(len(lab))
        if len(own):
            best = own[np.argmax(ious[i, own])]
            if ious[i, best] > F(iou_thres) and not detected[best]:
                out["correct"][i], detected[best] = 1, True
    out["stats"] = np.array([*PO.average_precision(out["correct"], out["prob"], len(lab)), 1], F)
    return out
