"""NumPy restatement of csrc/mosaic.hip (include/mdcv_aug.h), operation for operation: pixels as a gather of fp32 words, labels
as single np.float32 operations in the kernel's order (np.fmax / np.fmin return the other operand for a NaN, as fmaxf / fminf do)."""
import numpy as np

F = np.float32
DESC = 8


def row_ok(d, B, H, W):
    d = [int(v) for v in d]
    if d[0] == 0:
        return True
    if d[0] != 1:
        return False
    if not (1 <= d[1] <= W - 1 and 1 <= d[2] <= H - 1):
        return False
    return all(0 <= s < B for s in d[3:7]) and d[7] == 0


def candidate(r):
    return bool((((r[0] + r[1]) + r[2]) + r[3]) + r[4] > F(0))


def label(r, qx, qy, xc, yc, H, W, min_px, min_visible):
    """one candidate row of the source shown in quadrant (qx, qy) -> the row it becomes (5 float32), or None"""
    r = np.asarray(r, F)
    min_px, min_visible = F(min_px), F(min_visible)
    Wf, Hf, half = F(W), F(H), F(0.5)
    with np.errstate(all="ignore"):
        hw, hh = r[3] * half, r[4] * half
        x1, x2 = (r[1] - hw) * Wf, (r[1] + hw) * Wf
        y1, y2 = (r[2] - hh) * Hf, (r[2] + hh) * Hf
        dx, dy = F(xc if qx else xc - W), F(yc if qy else yc - H)
        xlo, xhi = (F(xc), Wf) if qx else (F(0), F(xc))
        ylo, yhi = (F(yc), Hf) if qy else (F(0), F(yc))
        X1, X2 = np.fmin(np.fmax(x1 + dx, xlo), xhi), np.fmin(np.fmax(x2 + dx, xlo), xhi)
        Y1, Y2 = np.fmin(np.fmax(y1 + dy, ylo), yhi), np.fmin(np.fmax(y2 + dy, ylo), yhi)
        w, h = X2 - X1, Y2 - Y1
        area = (x2 - x1) * (y2 - y1)
        if not (w >= min_px and h >= min_px and w * h >= min_visible * area):
            return None
        return np.array([r[0], ((X1 + X2) * half) / Wf, ((Y1 + Y2) * half) / Hf, w / Wf, h / Hf], F)


def source_of(d, b, y, x, H, W):
    """(source image, source y, source x) of output pixel (y, x) of image b under descriptor row d"""
    if int(d[0]) != 1:
        return b, y, x
    xc, yc = int(d[1]), int(d[2])
    qx, qy = int(x >= xc), int(y >= yc)
    return int(d[3 + 2 * qy + qx]), y - yc + (0 if qy else H), x - xc + (0 if qx else W)


def pixels(desc, imgs):
    """imgs [B,C,H,W] float32 -> the mosaic batch; a bad row passes through"""
    B, C, H, W = imgs.shape
    out = np.empty_like(imgs)
    for b in range(B):
        d = desc[b]
        if not (row_ok(d, B, H, W) and int(d[0]) == 1):
            out[b] = imgs[b]
            continue
        xc, yc, s = int(d[1]), int(d[2]), [int(v) for v in d[3:7]]
        out[b, :, :yc, :xc] = imgs[s[0], :, H - yc:, W - xc:]
        out[b, :, :yc, xc:] = imgs[s[1], :, H - yc:, :W - xc]
        out[b, :, yc:, :xc] = imgs[s[2], :, :H - yc, W - xc:]
        out[b, :, yc:, xc:] = imgs[s[3], :, :H - yc, :W - xc]
    return out


def labels(desc, targets, T_out, min_px, min_visible, H, W):
    """targets [B,T,5] float32 -> (targets_out [B,T_out,5], stats int32[4] = kept, dropped by the rule, lost beyond T_out, error bits)"""
    B, T, _ = targets.shape
    out = np.zeros((B, T_out, 5), F)
    stats = np.zeros(4, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            d = desc[b]
            ok = row_ok(d, B, H, W)
            if not ok:
                stats[3] |= 1
            if not (ok and int(d[0]) == 1):
                n = min(T, T_out)
                out[b, :n] = targets[b, :n]
                for t in range(T):
                    if candidate(targets[b, t]):
                        stats[0 if t < T_out else 2] += 1
                continue
            n = 0
            for q in range(4):
                for t in range(T):
                    r = targets[int(d[3 + q]), t]
                    if not candidate(r):
                        continue
                    o = label(r, q & 1, q >> 1, int(d[1]), int(d[2]), H, W, min_px, min_visible)
                    if o is None:
                        stats[1] += 1
                    elif n < T_out:
                        out[b, n] = o
                        n += 1
                        stats[0] += 1
                    else:
                        n += 1
                        stats[2] += 1
    return out, stats


def mosaic(desc, imgs, targets, T_out, min_px, min_visible):
    desc = np.asarray(desc, np.int32).reshape(-1, DESC)
    _, _, H, W = imgs.shape
    t, s = labels(desc, targets, T_out, min_px, min_visible, H, W)
    return pixels(desc, imgs), t, s
