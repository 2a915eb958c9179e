"""mdcv_detect_merge_tiles_soft restated in NumPy, rule by rule as include/mdcv_softtiles.h numbers them.  `dt` types the scores, weights and
thresholds; the IoU and the seam ratio are csrc/nms_core.h's float32 arithmetic, converted as in tests/helpers/softnms_numpy.py."""
import numpy as np

import detect_tiles_numpy as TN
import softnms_numpy as S

F, I32, EPS = np.float32, np.int32, S.EPS
CLASSES = np.array([-3, 0, 70000], I32)


def merge(boxes, prob, cls, count, tiles, B, overlap, contain, top_k, method, sigma, score_thres, dt=F):
    """rules 1-5 (cls None: class-agnostic) -> the outputs, `decays` [B,top_k] of the emitted scores, and `margin`: the smallest ratio of a
    decision's gap (a pick to its runner-up and to score_thres, a linear IoU to overlap) to the bound 2 d 2^-23 (an ulp at least)"""
    assert TN.table_ok(tiles, B)
    K, seam = boxes.shape[1], F(contain) >= F(0)
    out = dict(boxes=np.zeros((B, top_k, 4), F), prob=np.zeros((B, top_k), dt), cls=np.zeros((B, top_k), I32),
               src=np.full((B, top_k, 2), -1, I32), count=np.zeros(B, I32))
    decays, margin = np.zeros((B, top_k), np.int64), np.inf
    for b in range(B):
        ts = np.nonzero(tiles[:, 0] == b)[0]
        ns = [min(max(int(count[t]), 0), K) for t in ts]                                      # rule 1
        if not sum(ns):
            continue
        bx = np.concatenate([TN.offset_boxes(boxes[t, :n], tiles[t, 1], tiles[t, 2]) for t, n in zip(ts, ns)])
        pr = np.concatenate([prob[t, :n] for t, n in zip(ts, ns)])
        tile, slot = np.repeat(ts, ns), np.concatenate([np.arange(n) for n in ns])
        cl = np.zeros(len(pr), I32) if cls is None else np.concatenate([cls[t, :n] for t, n in zip(ts, ns)])
        o = TN.visiting_order(pr, tile, slot, top_k)
        bx, s, tile, slot, cl = bx[o], pr[o].astype(dt), tile[o], slot[o], cl[o]
        with np.errstate(all="ignore"):
            area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            live, d, em = np.ones(len(s), bool), np.zeros(len(s), np.int64), []
            err = lambda i: max(2 * d[i], 1) * EPS * abs(float(s[i])) + 1e-300  # noqa: E731
            while live.any():
                cand = np.nonzero(live)[0]
                m = cand[0] if method == "hard" else cand[np.argmax(s[cand])]                 # rules 4 / 2: first maximum = smaller rank
                rest = cand[cand != m]
                if method != "hard":
                    margin = min(margin, abs(float(s[m]) - score_thres) / err(m))
                    r = rest[np.argmax(s[rest])] if len(rest) else m
                    if r != m and (d[m] or d[r]):                                             # two undecayed scores compare exactly
                        margin = min(margin, (float(s[m]) - float(s[r])) / (err(m) + err(r)))
                    if not s[m] > dt(score_thres):
                        break
                em.append(m), live.__setitem__(m, False)
                decays[b, len(em) - 1], out["prob"][b, len(em) - 1] = d[m], s[m]
                j = np.nonzero(live & (cl == cl[m]) & ((tile != tile[m]) | (method == "hard")))[0]      # rule 3 (hard: every pair)
                iou = S.pair_iou(bx[m], area[m], bx[j], area[j])
                inter = (np.fmax(np.fmin(bx[j, 2], bx[m, 2]) - np.fmax(bx[j, 0], bx[m, 0]), F(0)) *
                         np.fmax(np.fmin(bx[j, 3], bx[m, 3]) - np.fmax(bx[j, 1], bx[m, 1]), F(0)))
                cut = seam & (tile[j] != tile[m]) & ~(inter / np.where(area[j] < area[m], area[j], area[m]) <= F(contain))   # the seam rule
                if method == "hard":
                    live[j[cut | ~(iou <= F(overlap))]] = False
                    continue
                live[j[cut]] = False
                j, iou = j[~cut], iou[~cut]
                if method == "linear":
                    hit, w = iou.astype(dt) > dt(overlap), dt(1) - iou.astype(dt)
                    margin = min([margin, *(np.abs(iou[~np.isnan(iou)].astype(np.float64) - overlap) / EPS)])
                else:
                    hit, w = iou > 0, np.exp(-(iou.astype(np.float64) * iou.astype(np.float64)) / np.float64(sigma)).astype(dt)
                s[j[hit]] = s[j[hit]] * w[hit]
                d[j[hit]] += 1
        n = out["count"][b] = len(em)
        out["boxes"][b, :n], out["cls"][b, :n], out["src"][b, :n] = bx[em], cl[em] if cls is not None else 0, np.stack([tile[em], slot[em]], 1)
    return out, decays, margin


def tiled_scene(n, seed, grids, K, nms=0.3, sthres=0.05, size=230, step=100, centres=12):
    """one S.scene per frame cut into grids[f] = (columns, rows) tiles of `size` px every `step` px, S.soft_nms per tile over the boxes whose
    centre it holds, each tile with its own view of a cone's score -> tile_boxes [T,K,4], tile_prob, tile_cls, tile_count, the tile table"""
    T = sum(gx * gy for gx, gy in grids)
    tb, tp, tc, cnt, table = np.zeros((T, K, 4), F), np.zeros((T, K), F), np.zeros((T, K), I32), np.zeros(T, I32), np.zeros((T, 4), I32)
    t = 0
    for f, (gx, gy) in enumerate(grids):
        (b, s), rng = S.scene(n, seed + f, centres), np.random.default_rng(seed + f)
        c, cls = (b[:, :2] + b[:, 2:]) / 2, CLASSES[np.arange(n) % 3]
        for ox, oy in ((step * x, step * y) for y in range(gy) for x in range(gx)):
            own = np.nonzero((c[:, 0] >= ox) & (c[:, 0] < ox + size) & (c[:, 1] >= oy) & (c[:, 1] < oy + size))[0]
            bt = b[own] - np.array([ox, oy, ox, oy], F)
            keep, out, _, _ = S.soft_nms(bt, s[own] * rng.uniform(0.8, 1.0, len(own)).astype(F), None, "linear", nms, 0.5, sthres, K)
            cnt[t], table[t], tb[t, :len(keep)], tp[t, :len(keep)], tc[t, :len(keep)] = len(keep), (f, ox, oy, 0), bt[keep], out, cls[own][keep]
            t += 1
    return tb, tp, tc, cnt, table
