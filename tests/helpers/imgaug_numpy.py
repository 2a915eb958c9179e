"""NumPy restatement of the four image operations of the augmented real-image loader (csrc/imgaug.hip), byte for byte what Pillow 12.2
computes: `Image.blend` under ImageEnhance.Brightness / Contrast / Color, `convert('HSV')` / `convert('RGB')` around the hue shift, and
`Image.transform(AFFINE, BILINEAR, fillcolor=127)`.  tests/test_imgaug_host.py pins it against Pillow itself and the golden images; the
GPU tests then use it where golden files would be too large.  Test infrastructure only: the product never imports it."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def luma(rgb):
    """Pillow convert('L') of (..., 3) uint8 -> int64"""
    a = rgb.astype(np.int64)
    return (a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16


def blend(degenerate, image, factor):
    """Image.blend(degenerate, image, factor): float32 `d + alpha * (i - d)`, truncated; clipped first when alpha is outside [0, 1]"""
    alpha = F32(factor)
    d, i = degenerate.astype(np.int32), image.astype(np.int32)
    t = d.astype(F32) + alpha * (i - d).astype(F32)
    assert t.dtype == F32
    if 0 <= alpha <= 1:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def contrast_mean(rgb):
    """ImageEnhance.Contrast's degenerate grey: int(mean of convert('L') + 0.5), the mean being sum / count in double"""
    l = luma(rgb)
    return int(float(int(l.sum())) / float(l.size) + 0.5)


def brightness(rgb, factor):
    return blend(np.zeros_like(rgb), rgb, factor)


def saturation(rgb, factor):
    return blend(np.repeat(luma(rgb)[..., None], 3, -1), rgb, factor)


def contrast(rgb, factor, mean=None):
    return blend(np.full_like(rgb, contrast_mean(rgb) if mean is None else mean), rgb, factor)


def rgb_to_hsv(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = (maxc - minc).astype(F32)
    crs = np.where(grey, F32(1), cr)
    s = cr / np.where(maxc == 0, 1, maxc).astype(F32)
    rc, gc, bc = ((maxc - c).astype(F32) / crs for c in (r, g, b))
    h = np.where(r == maxc, bc - gc,                                           # float32 difference; the sums with a literal are double
                 np.where(g == maxc, (2.0 + rc.astype(F64) - bc.astype(F64)).astype(F32),
                          (4.0 + gc.astype(F64) - rc.astype(F64)).astype(F32))).astype(F32)
    h = np.fmod(h.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
    uh = np.clip((h.astype(F64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(F64) * 255.0).astype(np.int64), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    h, s, v = (hsv[..., k].astype(np.int32) for k in range(3))
    hh = h.astype(F32) * F32(6) / F32(255)
    i = np.floor(hh)
    f = hh - i
    fs = s.astype(F32) / F32(255)
    maxc = v.astype(F32)
    one = F32(1)

    def rnd(x):
        assert x.dtype == F32
        return np.clip(np.floor(x.astype(F64) + 0.5).astype(np.int64), 0, 255)      # C round(): halves away from zero (x >= 0)
    p, q, t = rnd(maxc * (one - fs)), rnd(maxc * (one - fs * f)), rnd(maxc * (one - fs * (one - f)))
    k = i.astype(np.int32) % 6
    out = np.stack([np.choose(k, [v, q, p, p, t, v]), np.choose(k, [t, v, v, q, p, p]), np.choose(k, [p, p, t, v, v, q])], -1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def hue_shift(hue_factor):
    """the uint8 that adjust_hue adds to the H channel: int(hue_factor * 255) truncated toward zero, modulo 256"""
    return int(hue_factor * 255) % 256


def hue(rgb, factor):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = hsv[..., 0] + np.uint8(hue_shift(factor))                   # uint8 wrap-around
    return hsv_to_rgb(hsv)


def jitter(rgb, order, factors, hue_factor):
    """ColorJitter's shuffled chain on an (H, W, 3) uint8 image: order is a permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE)"""
    for op in order:
        if op == BRIGHTNESS:
            rgb = brightness(rgb, factors[0])
        elif op == CONTRAST:
            rgb = contrast(rgb, factors[1])
        elif op == SATURATION:
            rgb = saturation(rgb, factors[2])
        else:
            rgb = hue(rgb, hue_factor)
    return rgb


def inverse_affine_matrix(width, height, angle, translate, scale, shear):
    """torchvision 0.3 F.affine's matrix for Image.transform (output -> input), float64 libm"""
    cx, cy = width * 0.5 + 0.5, height * 0.5 + 0.5
    a, sh = math.radians(angle), math.radians(shear)
    k = 1.0 / scale
    d = math.cos(a + sh) * math.cos(a) + math.sin(a + sh) * math.sin(a)
    m = [math.cos(a + sh), math.sin(a + sh), 0, -math.sin(a), math.cos(a), 0]
    m = [k / d * v for v in m]
    m[2] += m[0] * (-cx - translate[0]) + m[1] * (-cy - translate[1])
    m[5] += m[3] * (-cx - translate[0]) + m[4] * (-cy - translate[1])
    m[2] += cx
    m[5] += cy
    return m


def affine(img, m, fill=127):
    """Image.transform(size, AFFINE, m, BILINEAR, fillcolor=fill) of an (H, W, C) uint8 image"""
    H, W, C = img.shape
    ys, xs = np.mgrid[0:H, 0:W]
    xo, yo = xs + 0.5, ys + 0.5
    xin = m[0] * xo + m[1] * yo + m[2]
    yin = m[3] * xo + m[4] * yo + m[5]
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = xin - x, yin - y
    x0, x1, y0, y1 = np.clip(x, 0, W - 1), np.clip(x + 1, 0, W - 1), np.clip(y, 0, H - 1), np.clip(y + 1, 0, H - 1)
    out = np.full_like(img, fill)
    for c in range(C):
        p = img[:, :, c].astype(F64)
        v1 = p[y0, x0] + (p[y0, x1] - p[y0, x0]) * dx
        v2 = p[y1, x0] + (p[y1, x1] - p[y1, x0]) * dx
        v = v1 + (v2 - v1) * dy
        out[:, :, c] = np.where(inside, v.astype(np.uint8), fill)
    return out


def augment(rgb, jit=None, aff=None, bw=False, flip=False):
    """the chain between the patch crop and to_tensor: jitter -> affine -> convert('L') -> hflip; (H, W, 3) uint8 -> (H, W, C) uint8.
    jit = (order, (b, c, s), hue_factor) or None; aff = six matrix doubles or None"""
    if jit is not None:
        rgb = jitter(rgb, *jit)
    if aff is not None:
        rgb = affine(rgb, aff)
    if bw:
        rgb = luma(rgb).astype(np.uint8)[..., None]
    if flip:
        rgb = rgb[:, ::-1]
    return np.ascontiguousarray(rgb)
