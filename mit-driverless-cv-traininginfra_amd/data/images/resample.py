"""Pillow's 8-bit convolution resize (`Image.resize(size, filter)`, reducing_gap=None) -- LANCZOS for tile-and-scale (`ts`,
utils.py:321-326 `scale_image`), antialiased BILINEAR for pad-and-resize -- with coefficient tables computed here in float64 the way
Pillow's `precompute_coeffs` computes them (cached per (in, out, filter)); the 127 padding, the patch crop (`Image.crop` rounds the box
with `round`), `convert('L')`, `FLIP_LEFT_RIGHT` and `/255` in fp32 around it all run on the device."""
import math
from functools import lru_cache

import numpy as np

PRECISION_BITS = 22                      # Pillow Resample.c: 32 - 8 - 2
LANCZOS, BILINEAR = "lanczos", "bilinear"


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x               # libm sin, as Pillow: a one-ulp difference can flip a fixed-point rounding


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


_FILTERS = {LANCZOS: (_lanczos, 3.0), BILINEAR: (_bilinear, 1.0)}


@lru_cache(maxsize=512)
def resample_coeffs(in_size, out_size, filt):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for a full-width box -> (ksize, first[out], count[out], kk[out, ksize] int32).

    A same-size axis is a copy (Pillow skips that pass): one tap of weight 1 << 22."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resample: sizes must be positive, got {in_size} -> {out_size}")
    if in_size == out_size:
        r = np.arange(out_size, dtype=np.int32)
        return 1, r, np.ones(out_size, np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)
    fn, fsupport = _FILTERS[filt]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)
        first[xx], count[xx] = xmin, xmax
    return ksize, first, count, kk
