"""Seeded boxes for the detect-and-draw tests (tests/test_detect_host.py, tests/test_gpu_detect.py, tests/golden/make_golden_detect.py).

Boxes are chosen in FRAME coordinates by category and carried back to detector coordinates as float32((f + pad) * ratio), the inverse of
detect.py:100-103.  The round trip is exact where ratio is a power of two (integer pads), so the settings below include such ratios: the
"exactly W - 1", "exactly W" and "in (-1, 0)" categories then land exactly; under the letterbox ratios they land within an ulp of the edge,
on either side, which is the other half of the coverage."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((1, 1), (12, 10), (37, 23))            # (W, H)


def letterbox(W, H, side):
    from mdcv.data.images import letterbox as lb
    pad_w, pad_h, ratio = lb(W, H, side, side)
    return float(ratio), int(pad_w), int(pad_h)


def settings(W, H):
    """(ratio, pad_w, pad_h) used per frame size: two exact ones, and letterbox() at 64 x 64 and at 416 x 416"""
    return [(1.0, 0, 0), (0.5, 3, 2), letterbox(W, H, 64), letterbox(W, H, 416)]


def _axis_pairs(rng, n):
    """(lo, hi) pairs in frame coordinates along an axis of n pixels, by category; every pair has lo <= hi"""
    u = rng.uniform
    far = 3.0 * n + 7.0
    pairs = [
        (u(0, n - 1), None),                         # inside
        (u(-far, -1.5), u(0, n - 1)),                # straddles the low edge
        (u(0, n - 1), u(n, far)),                    # straddles the high edge
        (u(-far, -1.5), u(n, far)),                  # straddles both
        (u(-far, -2.0), -1.25),                      # fully outside, low side
        (n + 0.5, u(n + 1, far)),                    # fully outside, high side
        (-u(0.01, 0.99), u(0, n - 1)),               # lo in (-1, 0): truncates to 0
        (-u(0.01, 0.99), -0.005),                    # both in (-1, 0): truncate to 0, 0
        (u(0, n - 1), "same"),                       # degenerate after truncation: hi in the same pixel
        (0.0, float(n - 1)),                         # reaches exactly n - 1
        (u(0, n - 1), float(n - 1)),
        (0.0, float(n)),                             # reaches exactly n
        (float(n - 1), float(n)),
        (float(n), float(n)),                        # starts exactly at n
        (-1.0, 0.0),
        (-1.5, -1.0),                                # -1.5 -> -1, -1.0 -> -1: degenerate, outside
    ]
    out = []
    for lo, hi in pairs:
        lo = float(lo)
        if hi is None:
            hi = rng.uniform(lo, max(lo, n - 1))
        elif isinstance(hi, str):
            hi = min(np.floor(lo) + 0.99, lo + rng.uniform(0, 0.9)) if lo >= 0 else lo
        hi = float(hi)
        if hi < lo:
            lo, hi = hi, lo
        out.append((lo, hi))
    return out


def frame_boxes(W, H, seed):
    """about 200 valid boxes (x0, y0, x1, y1) in frame coordinates: every category of x against a rotating category of y, so that each
    edge, each corner, each outside side and the three degenerate forms (width, height, both) occur"""
    rng = np.random.default_rng(seed)
    xs, ys = _axis_pairs(rng, W), _axis_pairs(rng, H)
    boxes = []
    for i, (x0, x1) in enumerate(xs):
        for j in range(len(ys)):
            if (i + j) % 4 == 0 or i == j or j == 8 or i == 8:
                y0, y1 = ys[j]
                boxes.append((x0, y0, x1, y1))
    for _ in range(200 - min(200, len(boxes))):
        (x0, x1), (y0, y1) = _axis_pairs(rng, W)[int(rng.integers(16))], _axis_pairs(rng, H)[int(rng.integers(16))]
        boxes.append((x0, y0, x1, y1))
    return np.array(boxes, np.float64)


def to_detector(fb, ratio, pad_w, pad_h):
    """frame coordinates -> float32 detector coordinates; pairs that float32 rounding inverted are put back in order"""
    pads = np.array([pad_w, pad_h, pad_w, pad_h], np.float64)
    d = ((np.asarray(fb, np.float64) + pads) * ratio).astype(np.float32)
    d[:, 2] = np.maximum(d[:, 2], d[:, 0])
    d[:, 3] = np.maximum(d[:, 3], d[:, 1])
    return d


def bad_boxes():
    """float32 detector boxes that must be skipped under any ratio up to 2^10: inverted in x, in y, NaN, +-inf, magnitude >= 2^30"""
    big = np.float32(2.0 ** 40)
    return np.array([[5, 1, 4, 3], [1, 6, 4, 3], [np.nan, 1, 4, 3], [1, 1, np.inf, 3], [-np.inf, 1, 4, 3], [1, 1, 4, np.nan],
                     [1, 1, big, 3], [-big, 1, 4, 3], [1, -big, 4, big]], np.float32)


def random_frame(W, H, seed):
    f = np.random.default_rng(seed).integers(0, 255, (H, W, 3), dtype=np.uint8)       # never 255: a drawn red byte always differs somewhere
    return f
