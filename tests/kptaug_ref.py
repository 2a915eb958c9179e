"""NumPy restatement of csrc/kptaug.hip (include/mdcv_kptaug.h), operation for operation: every step a single np.float32
operation in the kernel's order (np.fmax / np.fmin return the other operand for a NaN, as fmaxf / fminf do), the heat-maps through the two
functions of oracle/synth_oracle.py that restate csrc/kpt_heatmap.h in float64."""
import numpy as np

from oracle.synth_oracle import _blur_reflect101, _resize_onehot_axis

F = np.float32
DESC = 24
K = 7
PERM = (0, 2, 1, 4, 3, 6, 5)
APPLY, SWAP = 1, 2


def row(apply=1, swap=0, I=(1, 0, 0, 0, 1, 0), Fw=(1, 0, 0, 0, 1, 0), gain=(1, 1, 1), bias=(0, 0, 0), flags=None):
    """a descriptor row int32[24] from plain numbers (each rounded once to fp32)"""
    d = np.zeros(DESC, np.int32)
    d[0] = (APPLY * int(bool(apply)) | SWAP * int(bool(swap))) if flags is None else flags
    d[1:19] = np.array([*I, *Fw, *gain, *bias], np.float64).astype(F).view(np.int32)
    return d


def row_ok(d):
    d = np.asarray(d, np.int32)
    if int(d[0]) & ~3:
        return False
    if not np.isfinite(d[1:19].view(F)).all():
        return False
    return not d[19:].any()


def forward(d, pts, S):
    """the seven points of one image through the forward map -> (X [7], Y [7]) in pixels, float32"""
    Fw, Sf = np.asarray(d, np.int32)[7:13].view(F), F(S)
    with np.errstate(all="ignore"):
        px, py = pts[:, 0] * Sf, pts[:, 1] * Sf
        X = (Fw[0] * px + Fw[1] * py) + Fw[2]
        Y = (Fw[3] * px + Fw[4] * py) + Fw[5]
    return X.astype(F), Y.astype(F)


def valid(X, Y, S):
    v = np.concatenate([X, Y])
    return bool(((v >= F(0)) & (v <= F(S))).all())                # a NaN compares false


def pixels(d, img):
    """img [C,S,S] float32 -> the warped, colour-adjusted image"""
    d = np.asarray(d, np.int32)
    C, S, _ = img.shape
    I, gain, bias, Sf = d[1:7].view(F), d[13:16].view(F), d[16:19].view(F), F(S)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    xf, yf = xx.astype(F), yy.astype(F)
    with np.errstate(all="ignore"):
        sx = np.fmin(np.fmax((I[0] * xf + I[1] * yf) + I[2], F(-1)), Sf)
        sy = np.fmin(np.fmax((I[3] * xf + I[4] * yf) + I[5], F(-1)), Sf)
        x0f, y0f = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0f, sy - y0f
        xi, yi = x0f.astype(np.int64), y0f.astype(np.int64)
        x0, x1 = np.clip(xi, 0, S - 1), np.clip(xi + 1, 0, S - 1)
        y0, y1 = np.clip(yi, 0, S - 1), np.clip(yi + 1, 0, S - 1)
        out = np.empty_like(img)
        for c in range(C):
            p = img[c]
            v00, v01, v10, v11 = p[y0, x0], p[y0, x1], p[y1, x0], p[y1, x1]
            top = v00 + fx * (v01 - v00)
            bot = v10 + fx * (v11 - v10)
            v = top + fy * (bot - top)
            out[c] = np.fmin(np.fmax(v * gain[c] + bias[c], F(0)), F(1))
    assert out.dtype == F and sx.dtype == F and fx.dtype == F
    return out


def heatmap(hx, hy, S):
    """prep_label's map of a one-hot at row hy, column hx of an S x S crop, at S x S"""
    vy = _blur_reflect101(_resize_onehot_axis(hy, S, S))
    vx = _blur_reflect101(_resize_onehot_axis(hx, S, S))
    tot = sum(vy.tolist()) * sum(vx.tolist())
    return (np.outer(vy, vx) / tot).astype(F)


def kptaug(desc, imgs, hm, pts):
    """-> (imgs_out, hm_out, pts_out, stats int32[4] = augmented, rejected, passed through, error bits)"""
    desc = np.asarray(desc, np.int32).reshape(-1, DESC)
    B, C, S, _ = imgs.shape
    oi, oh, op = imgs.copy(), hm.copy(), pts.copy()
    stats = np.zeros(4, np.int32)
    for b in range(B):
        d = desc[b]
        ok = row_ok(d)
        if not ok:
            stats[3] |= 1
        wanted = ok and bool(int(d[0]) & APPLY)
        X, Y = forward(d, pts[b], S)
        if not (wanted and valid(X, Y, S)):
            stats[1 if wanted else 2] += 1
            continue
        stats[0] += 1
        oi[b] = pixels(d, imgs[b])
        for k in range(K):
            j = PERM[k] if int(d[0]) & SWAP else k
            op[b, k, 0], op[b, k, 1] = X[j] / F(S), Y[j] / F(S)
            oh[b, k] = heatmap(min(int(X[j]), S - 1), min(int(Y[j]), S - 1), S)
    return oi, oh, op, stats
