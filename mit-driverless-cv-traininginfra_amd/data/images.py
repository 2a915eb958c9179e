"""Real-image detector batches: `ImageLabelBatches` stands where `DataLoader(ImageLabelDataset(...))` stands in CVC-YOLOv3/train.py:124-141.

The host decodes (Pillow, on a thread pool) and crops each frame to the source window its output patch reads; everything from that
uint8 window to the `[B,C,H,W]` fp32 batch runs in csrc/imgload.hip (two launches per batch) or, for a batch with an augmented sample,
csrc/imgaug.hip (three or four), and one more launch of csrc/imgfx.hip for a batch with a blurred / noised / contrasted / sharpened
sample.  What the reference's chain computes
(CVC-YOLOv3/utils/datasets.py:124-315 with utils/utils.py's geometry and label helpers, torchvision 0.3's pad / resize / to_grayscale /
hflip / to_tensor over Pillow) is reproduced exactly:

* images: Pillow's 8-bit convolution resize (`Image.resize(size, filter)`, reducing_gap=None) -- LANCZOS for tile-and-scale (`ts`,
  utils.py:321-326 `scale_image`), antialiased BILINEAR for pad-and-resize -- with coefficient tables computed here in float64 the way
  Pillow's `precompute_coeffs` computes them (cached per (in, out, filter)); the 127 padding, the patch crop (`Image.crop` rounds the box
  with `round`), `convert('L')`, `FLIP_LEFT_RIGHT` and `/255` in fp32 around it, all on the device.
* labels: the reference's helpers restated in NumPy with torch's arithmetic (float32 tensors; a Python scalar meeting one is rounded to
  float32 first; `filter_and_offset_labels` mixes 0-dim float32 tensors with Python doubles), computed on the host and shipped with the
  pixels in the same pinned buffer and the same copy.
* augmentation (`augment_hsv`, `augment_affine`, `data_aug`; datasets.py:226-242): torchvision 0.3's `ColorJitter(brightness=0.25,
  contrast=0.25, saturation=0.25, hue=0.04)` with probability 0.5, then `F.affine(angle, translate, scale, shear, BILINEAR, fillcolor=127)`
  of every sample that has boxes, between the patch crop and to_grayscale.  Both are glue over Pillow and are reproduced byte for byte:
  `ImageEnhance.Brightness / Contrast / Color` are `Image.blend` against 0 / the mean luma / the pixel's luma, `adjust_hue` is
  `convert('HSV')`, a wrapping uint8 shift of H and `convert('RGB')`, `F.affine` is `Image.transform(AFFINE, BILINEAR)` with the inverse
  matrix computed here in float64 (libm).  The hue shift is `int(hue_factor * 255)` truncated toward zero, modulo 256: what
  `np.uint8(float)` gave on x86-64 with the NumPy of torchvision 0.3's time (NumPy 2 raises OverflowError for the negative ones).
  The boxes follow `affine_labels` in float32 torch CPU arithmetic, in the reference's sequence of operations.
* random draws: per sample from `random.Random(f"{seed}/{epoch}/{index}")`, in the reference's order: the patch; with `augment_hsv or
  data_aug` the jitter gate `random()`, and when it is `> 0.5` the brightness, contrast, saturation (`uniform(0.75, 1.25)`) and hue
  (`uniform(-0.04, 0.04)`) factors and the `shuffle` of the four ops; with `augment_affine or data_aug` the gate `random()` (`> 0`), angle
  `uniform(-10, 10)`, tx, ty `uniform(-40, 40)`, scale `uniform(0.9, 1.1)`, shear `uniform(-3, 3)`; then the flip.  A sample without boxes
  returns before all of this, as in the reference.  With the three options off no extra draw happens.
* the imgaug options (`blur`, `noise`, `contrast`, `sharpen`; datasets.py:253-295, imgaug 0.3.0 over OpenCV 4.1): `iaa.GaussianBlur`,
  `iaa.AdditiveGaussianNoise(per_channel=0.5)`, `iaa.SigmoidContrast` and `iaa.Sharpen` on the 8-bit image behind the flip, in that
  order.  Neither library can be pinned here, so DESIGN §16.3 defines the bytes: the blur is OpenCV's 8-bit fixed-point separable filter
  with imgaug's kernel-size rule (cv2's own rounding is declared unpinned), the contrast imgaug's float32 256-entry table, the sharpen one
  correctly rounded double expression over imgaug's float32 matrix, and the noise a counter-based integer generator of the same
  distribution (imgaug draws from NumPy's global Mersenne stream, which no device reproduces: the distribution matches, not the stream).
  Kernel tables, the contrast tables and the sharpen coefficients are computed here and shipped with the descriptors.  Draws continue the
  sample's stream behind the flip in the reference's order: blur gate `random()` (`> 0.2`), `uniform(40, -40)` (drawn and discarded, as
  the reference does), sigma `uniform(0, 3)`; noise gate (`> 0.3`), scale `uniform(0, 7.65)`; contrast gate (`> 0.5`), cutoff
  `uniform(0.45, 0.75)`, gain `randint(5, 10)`; sharpen gate (`> 0.3`), alpha `uniform(0, 0.5)`.  imgaug's own draws (the per_channel coin
  and the noise seed) come from a second generator, `random.Random(f"{seed}/{epoch}/{index}/imgaug")`.  With the four options off no
  extra draw happens and no extra launch runs.  `salt` is accepted and ignored with a warning (the reference stores it and never reads
  it); any of the four with `bw` raises ValueError (the reference then hands a 2-D array to `Image.fromarray(..., 'RGB')`).
"""
import csv
import json
import math
import os
import random
import warnings
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np
import torch

from .. import _lib
from . import framecache

PRECISION_BITS = 22                      # Pillow Resample.c: 32 - 8 - 2
DESC = 20                                # MDCV_IMGLOAD_DESC
AUG_DESC = 24                            # MDCV_IMGAUG_DESC
FREF = 4                                 # MDCV_IMGLOAD_FREF
STAGED = (-1, 0, 0, 0)                   # a frame reference that says: this image's window is in the staging buffer
LANCZOS, BILINEAR = "lanczos", "bilinear"
FX_DESC = 24                             # MDCV_IMGFX_DESC
FX_MAX_R = 7                             # csrc/imgfx_desc.h IMGFX_MAX_R
UNSUPPORTED = ()                         # every option of the reference's ImageLabelDataset is implemented
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3        # ColorJitter.get_params appends its four ops in this order
_F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- Pillow's resampler
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


# ------------------------------------------------------------------------------------------------- frame layout (both modes)
# The arithmetic below is what makes the labels exact, so its form is fixed: Python ints where the layout is whole pixels, int()
# truncation toward zero of the letterbox border, ceil of half the missing width, and patch starts that stay unrounded floats.

def letterbox(frame_w, frame_h, out_w, out_h):
    """Pad-and-resize layout (CVC-YOLOv3/utils/utils.py calculate_padding) -> (border_x, border_y, label_scale).

    The frame gets a 127 border on its shorter-than-needed axis so that it takes the output's aspect ratio, then the bordered frame is
    resized to out_w x out_h.  A frame at least as tall as it is wide is bordered left and right; any other, top and bottom."""
    if frame_h >= frame_w:
        return int((frame_h * out_w / out_h - frame_w) / 2), 0, out_h / frame_h
    return 0, int((frame_w * out_h / out_w - frame_h) / 2), out_w / frame_w


def scaled_size(width, height, scale):
    return int(width * scale), int(height * scale)          # scale_image: (int(W * s), int(H * s))


def tile_grid(scaled_w, scaled_h, patch_w, patch_h):
    """Tile-and-scale layout (utils.py pre_tile_padding / get_patch_spacings) of a scaled frame
    -> (border_x, border_y, cols, rows, step_back_x, step_back_y).

    An axis shorter than a patch is centred between 127 borders of ceil(missing / 2); the bordered axis is then covered by the fewest
    patches that reach its end, and the surplus is shared evenly: patch k along an axis starts at k * (patch - step_back)."""
    def axis(n, p):
        border = math.ceil((p - n) / 2) if n < p else 0
        full = n + 2 * border
        count = math.ceil(full / p)
        back = (count * p - full) / (count - 1) if count > 1 else 0
        return border, count, back
    bx, cols, sx = axis(scaled_w, patch_w)
    by, rows, sy = axis(scaled_h, patch_h)
    return bx, by, cols, rows, sx, sy


def patch_box(grid, patch_w, patch_h, index):
    """Unrounded (left, top, right, bottom) of patch `index` (row-major over the grid) in bordered-frame coordinates: the box that
    utils.py get_patch crops (after Image.crop rounds it) and filters the labels against (as it is)."""
    _, _, cols, _, sx, sy = grid
    c, r = index % cols, index // cols
    left = patch_w * c - sx * c
    top = patch_h * r - sy * r
    return left, top, left + patch_w, top + patch_h


def n_patches(frame_w, frame_h, scale, width, height):
    g = tile_grid(*scaled_size(frame_w, frame_h, scale), width, height)
    return g[2] * g[3]


# ------------------------------------------------------------------------------------------------------------- per-sample geometry
class Geometry:
    """Where one output image comes from: the frame window to upload, its kernel descriptor (offsets left 0) and tables, and the
    quantities the label pipeline needs (paddings, the unrounded patch boundary, the pad-and-resize ratio)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _axis(in_size, out_size, filt, o2s, n_out, src_lo, src_hi):
    """One axis of the resize: output index o reads resized index o + o2s (inside [0, out_size)); the resize input is a virtual
    line of in_size samples of which [src_lo, src_hi) are frame samples and the rest the 127 canvas."""
    ksize, first, count, kk = resample_coeffs(in_size, out_size, filt)
    s0, s1 = max(0, o2s), min(out_size, o2s + n_out)
    if s1 <= s0:
        s0 = s1 = max(0, min(out_size, o2s))
    f, c = first[s0:s1].astype(np.int64), count[s0:s1].astype(np.int64)
    tmin, tmax = (int(f.min()), int((f + c).max())) if s1 > s0 else (0, 0)
    w0, w1 = max(tmin, src_lo), min(tmax, src_hi)
    if w1 <= w0:
        w0 = w1 = tmin
    return dict(ksize=ksize, s0=s0, n=s1 - s0, first=f, count=c, kk=kk[s0:s1], tmin=tmin, tmax=tmax, w0=w0, w1=w1,
                src_lo=src_lo, off=o2s - s0)


def sample_geometry(frame_w, frame_h, width, height, ts, scale=1.0, patch_index=0, flip=False):
    frame_w, frame_h, width, height = int(frame_w), int(frame_h), int(width), int(height)
    if ts:
        sw, sh = scaled_size(frame_w, frame_h, scale)
        if sw <= 0 or sh <= 0:
            raise ValueError(f"scale {scale} shrinks a {frame_w}x{frame_h} frame to nothing")
        grid = tile_grid(sw, sh, width, height)
        hp, vp, n = grid[0], grid[1], grid[2] * grid[3]
        if not 0 <= patch_index < n:
            raise ValueError(f"patch index {patch_index} outside 0..{n - 1}")
        boundary = patch_box(grid, width, height, patch_index)
        x0, y0, x1, y1 = map(int, map(round, boundary))           # Image.crop
        if x1 - x0 != width or y1 - y0 != height:
            raise ValueError(f"patch box {boundary} rounds to {x1 - x0}x{y1 - y0}, not {width}x{height} (odd patch size with a .5 offset)")
        ax = _axis(frame_w, sw, LANCZOS, x0 - hp, width, 0, frame_w)
        ay = _axis(frame_h, sh, LANCZOS, y0 - vp, height, 0, frame_h)
        pad_x, pad_y = (-hp, sw + hp), (-vp, sh + vp)
        g = dict(hp=hp, vp=vp, boundary=boundary, n_patches=n, ratio=None, pad_w=None, pad_h=None)
    else:
        pad_w, pad_h, ratio = letterbox(frame_w, frame_h, width, height)
        pw_, ph_ = frame_w + 2 * pad_w, frame_h + 2 * pad_h
        if pw_ <= 0 or ph_ <= 0:
            raise ValueError(f"padding {pad_w},{pad_h} leaves nothing of a {frame_w}x{frame_h} frame")
        ax = _axis(pw_, width, BILINEAR, 0, width, pad_w, pad_w + frame_w)
        ay = _axis(ph_, height, BILINEAR, 0, height, pad_h, pad_h + frame_h)
        pad_x, pad_y = (0, width), (0, height)
        g = dict(hp=None, vp=None, boundary=None, n_patches=1, ratio=ratio, pad_w=pad_w, pad_h=pad_h)
    win = (ax["w0"] - ax["src_lo"], ay["w0"] - ay["src_lo"], ax["w1"] - ax["w0"], ay["w1"] - ay["w0"])   # frame x, y, w, h
    col = np.empty((ax["n"], ax["ksize"] + 2), np.int32)
    col[:, 0], col[:, 1], col[:, 2:] = ax["first"] - ax["w0"], ax["count"], ax["kk"]
    row = np.empty((ay["n"], ay["ksize"] + 2), np.int32)
    row[:, 0], row[:, 1], row[:, 2:] = ay["first"] - ay["tmin"], ay["count"], ay["kk"]
    desc = [0, win[2], win[3], ax["ksize"], ay["ksize"], 0, 0, ax["n"], ay["tmax"] - ay["tmin"], ay["tmin"] - ay["w0"], ay["n"],
            ax["off"], ay["off"], pad_x[0] - ax["s0"], pad_x[1] - ax["s0"], pad_y[0] - ay["s0"], pad_y[1] - ay["s0"], int(bool(flip)), 0, 0]
    return Geometry(ts=bool(ts), frame=(frame_w, frame_h), width=width, height=height, scale=scale, patch_index=patch_index,
                    flip=bool(flip), window=win, desc=desc, col=col, row=row, **g)


def crop_window(frame, geom):
    """The bytes the kernel reads: the frame (H, W, 3 uint8) cropped to geom.window, contiguous."""
    x, y, w, h = geom.window
    if frame.shape[1] != geom.frame[0] or frame.shape[0] != geom.frame[1]:
        raise ValueError(f"frame is {frame.shape[1]}x{frame.shape[0]}, the geometry was planned for {geom.frame[0]}x{geom.frame[1]}")
    return np.ascontiguousarray(frame[y:y + h, x:x + w, :3], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ augmentation (draws, matrix, boxes)
class Augmentation:
    """One sample's ColorJitter / affine parameters.  jitter: None or (order, (brightness, contrast, saturation), hue) with `order` the
    shuffled permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE); affine: None or (angle, (tx, ty), scale, shear).  `matrix` (the six
    doubles Image.transform gets) is filled in by `plan()`; `hue_shift` is the uint8 added to H.  The contrast op's grey level is the
    one value only the device knows: the mean luma of the patch at that point of the chain."""

    def __init__(self, jitter=None, affine=None):
        self.jitter, self.affine, self.matrix, self.hue_shift = None, None, None, 0
        if jitter is not None:
            order, factors, hue = jitter
            if sorted(order) != [0, 1, 2, 3] or len(factors) != 3:
                raise ValueError(f"jitter {jitter!r}: the order must be a permutation of 0..3, with three factors and a hue")
            self.jitter = (tuple(int(o) for o in order), tuple(float(f) for f in factors), float(hue))
            self.hue_shift = hue_shift(self.jitter[2])
        if affine is not None:
            angle, (tx, ty), scale, shear = affine
            self.affine = (float(angle), (float(tx), float(ty)), float(scale), float(shear))

    def __bool__(self):
        return self.jitter is not None or self.affine is not None


def hue_shift(hue_factor):
    """adjust_hue's `np.uint8(hue_factor * 255)`: truncated toward zero, modulo 256"""
    return int(hue_factor * 255) % 256


def draw_augmentation(rng, jitter_on, affine_on):
    """The draws of datasets.py:226-242 from `rng`, in its order (ColorJitter.get_params draws the four factors, then shuffles the ops)."""
    jitter = affine = None
    if jitter_on and rng.random() > 0.5:
        factors = tuple(rng.uniform(0.75, 1.25) for _ in range(3))
        hue = rng.uniform(-0.04, 0.04)
        order = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
        rng.shuffle(order)
        jitter = (tuple(order), factors, hue)
    if affine_on and rng.random() > 0:
        angle = rng.uniform(-10, 10)
        translate = (rng.uniform(-40, 40), rng.uniform(-40, 40))
        scale = rng.uniform(0.9, 1.1)
        shear = rng.uniform(-3, 3)
        affine = (angle, translate, scale, shear)
    return Augmentation(jitter, affine)


def inverse_affine_matrix(width, height, angle, translate, scale, shear):
    """torchvision 0.3 F.affine's data for Image.transform(AFFINE): output pixel centre -> input position, about the centre
    (W / 2 + 0.5, H / 2 + 0.5).  float64 with libm, the form fixed: the device reproduces Pillow only from the same six doubles."""
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


def affine_labels(height, width, labels, angle, translate, scale, shear):
    """datasets.py affine_labels on corner boxes (float32 [n,5] numpy): float32 torch CPU arithmetic in the reference's sequence of
    operations (3x3 float32 matrices built from float64 entries, S @ T @ R, the four corners warped, their bounding box shrunk by the
    angle's reduction and clamped to [0, max(W, H)]); a row is replaced when its warped box passes the size / area / aspect tests."""
    t = torch.from_numpy(np.array(labels, dtype=_F32))
    side = max(width, height)
    alpha = scale * math.cos(math.radians(angle))
    beta = scale * math.sin(math.radians(angle))
    rot = torch.tensor(((alpha, beta, (1 - alpha) * (width / 2.0) - beta * (height / 2.0)),
                        (-beta, alpha, (beta * width / 2.0) + (1 - alpha) * (height / 2.0)),
                        (0, 0, 1)), dtype=torch.float)
    tr = torch.eye(3)
    tr[0, 2] = translate[0]
    tr[1, 2] = translate[1]
    sh = torch.eye(3)
    sh[0, 1] = math.tan(math.radians(shear[0]))
    sh[0, 2] = -math.tan(math.radians(shear[0])) * height / 2.0
    sh[1, 0] = math.tan(math.radians(shear[1]))
    sh[1, 2] = -math.tan(math.radians(shear[1])) * width / 2.0
    m = sh @ tr @ rot
    n = t.shape[0]
    pts = t[:, 1:5]
    area0 = (pts[:, 2] - pts[:, 0]) * (pts[:, 3] - pts[:, 1])
    xy = torch.ones((n * 4, 3))
    xy[:, :2] = pts[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(n * 4, 2)
    xy = xy @ m.transpose(0, 1)
    xy = xy[:, :2] / xy[:, 2].unsqueeze(1).expand(-1, 2)
    xy = xy[:, :2].reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    xy = torch.cat((x.min(1)[0], y.min(1)[0], x.max(1)[0], y.max(1)[0])).reshape(4, n).transpose(0, 1)
    rad = angle * math.pi / 180
    reduction = max(abs(math.sin(rad)), abs(math.cos(rad))) ** 0.5
    cx, cy = (xy[:, 2] + xy[:, 0]) / 2, (xy[:, 3] + xy[:, 1]) / 2
    w, h = (xy[:, 2] - xy[:, 0]) * reduction, (xy[:, 3] - xy[:, 1]) * reduction
    xy = torch.cat((cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)).reshape(4, n).transpose(0, 1)
    xy = torch.clamp(xy, 0, side)
    w, h = xy[:, 2] - xy[:, 0], xy[:, 3] - xy[:, 1]
    area = w * h
    ar = torch.max(w / (h + 1e-16), h / (w + 1e-16))
    keep = (w > 4) & (h > 4) & (area / (area0 + 1e-16) > 0.1) & (ar < 10)
    t[keep, 1:5] = xy[keep]
    return t.numpy()


def aug_descriptor(aug):
    """MDCV_IMGAUG_DESC ints for one image (include/mdcv_hip.h); `aug` None or empty: the identity, which the kernel copies through"""
    d = np.zeros(AUG_DESC, np.int32)
    matrix, order, factors, shift = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], (0, 1, 2, 3), (1.0, 1.0, 1.0), 0
    if aug is not None and aug.jitter is not None:
        order, factors, shift = aug.jitter[0], aug.jitter[1], aug.hue_shift
        d[12] = 1
    if aug is not None and aug.affine is not None:
        if aug.matrix is None:
            raise ValueError("an affine augmentation needs its matrix (inverse_affine_matrix) before it is packed")
        matrix = aug.matrix
        d[21] = 1
    d[0:12] = np.array(matrix, np.float64).view(np.int32)
    d[13:17] = order
    d[17:20] = np.array(factors, _F32).view(np.int32)           # Image.blend takes its alpha as a C float
    d[20] = shift
    return d


# ------------------------------------------------------------------------------- blur / noise / contrast / sharpen (draws and tables)
class ImageFx:
    """One sample's imgaug parameters, each None when its op does not run.  blur: sigma; noise: (scale, per_channel, seed) with seed the
    32 bits that key the device's counter-based generator; contrast: (gain, cutoff); sharpen: alpha."""

    def __init__(self, blur=None, noise=None, contrast=None, sharpen=None):
        self.blur = None if blur is None else float(blur)
        self.noise = None if noise is None else (float(noise[0]), bool(noise[1]), int(noise[2]) & 0xffffffff)
        self.contrast = None if contrast is None else (int(contrast[0]), float(contrast[1]))
        self.sharpen = None if sharpen is None else float(sharpen)
        if self.blur is not None and not (self.blur < 5.0 and blur_radius(self.blur) <= FX_MAX_R):
            raise ValueError(f"blur sigma {self.blur}: sigma must stay below 5 (kernel radius {FX_MAX_R} at most; the reference draws it below 3)")
        if self.noise is not None and not 0.0 <= self.noise[0] <= 255.0:
            raise ValueError(f"noise scale {self.noise[0]} outside [0, 255]")
        if self.sharpen is not None and not 0.0 <= self.sharpen <= 1.0:
            raise ValueError(f"sharpen alpha {self.sharpen} outside [0, 1]")

    def __bool__(self):
        return any(v is not None for v in (self.blur, self.noise, self.contrast, self.sharpen))

    def runs(self):
        """some op changes bytes: a blur whose sigma imgaug skips does not"""
        return (self.blur is not None and blur_radius(self.blur) > 0) or any(v is not None for v in (self.noise, self.contrast, self.sharpen))


def draw_imgfx(rng, second, blur_on, noise_on, contrast_on, sharpen_on):
    """The draws of datasets.py:253-295 from `rng`, in its order, unused ones included; `second()` -> the generator of imgaug's own
    draws (the per_channel coin, then the noise seed), asked for only when the noise runs."""
    blur = noise = contrast = sharpen = None
    if blur_on and rng.random() > 0.2:
        rng.uniform(40, -40)                                     # the reference's unused `angle`
        blur = rng.uniform(0, 3.00)
    if noise_on and rng.random() > 0.3:
        scale = rng.uniform(0, 0.03 * 255)
        r2 = second()
        per_channel = r2.random() < 0.5                          # per_channel=0.5: a fair coin per image
        noise = (scale, per_channel, r2.getrandbits(32))
    if contrast_on and rng.random() > 0.5:
        cutoff = rng.uniform(0.45, 0.75)
        contrast = (rng.randint(5, 10), cutoff)
    if sharpen_on and rng.random() > 0.3:
        sharpen = rng.uniform(0, 0.5)
    return ImageFx(blur, noise, contrast, sharpen)


def blur_radius(sigma):
    """imgaug 0.3.0 blur_gaussian_ (cv2 backend): 0 when the op is skipped, else the radius of its kernel size"""
    if sigma <= 1e-3:
        return 0
    k = 3.3 * sigma if sigma < 3.0 else (2.9 * sigma if sigma < 5.0 else 2.6 * sigma)
    k = int(max(k, 5))
    return (k + 1 if k % 2 == 0 else k) // 2


@lru_cache(maxsize=512)
def blur_table(sigma):
    """-> (r, half table q[0..r], centre first): the Gaussian in float64 normalised to sum 1, each tap floor(w * 256 + 0.5), the centre
    corrected so that the whole kernel sums to 256 (OpenCV 4.1's 8-bit fixed point)"""
    r = blur_radius(sigma)
    w = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(r + 1)]
    total = w[0] + 2.0 * sum(w[1:])
    q = [int(math.floor(v / total * 256.0 + 0.5)) for v in w]
    q[0] = 256 - 2 * sum(q[1:])
    return r, tuple(q)


@lru_cache(maxsize=64)
def sigmoid_table(gain, cutoff):
    """imgaug 0.3.0 adjust_contrast_sigmoid's uint8 table, in its float32 arithmetic; the cast truncates"""
    v = np.linspace(0, 1, 256, dtype=_F32)
    table = 0 + 255 * 1 / (1 + np.exp(_F32(gain) * (_F32(cutoff) - v)))
    return np.clip(table, 0, 255).astype(np.uint8)


def sharpen_coefficients(alpha):
    """imgaug 0.3.0 Sharpen's matrix at lightness 1: float32 arrays combined with the Python-float alpha -> (centre, neighbour) float32"""
    nochange = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=_F32)
    effect = np.array([[-1, -1, -1], [-1, 8 + 1, -1], [-1, -1, -1]], dtype=_F32)
    m = (1 - alpha) * nochange + alpha * effect
    assert m.dtype == _F32
    return m[1, 1], m[0, 0]


def fx_descriptor(fx, lut_index=0):
    """MDCV_IMGFX_DESC ints for one image (include/mdcv_hip.h); `fx` None or empty, or an op that is off: the identity"""
    d = np.zeros(FX_DESC, np.int32)
    r, q, scale, kc, kn = 1, (256, 0), 0.0, _F32(1), _F32(0)
    if fx is not None and fx.blur is not None and blur_radius(fx.blur) > 0:
        r, q = blur_table(fx.blur)
        d[0] = 1
    if fx is not None and fx.noise is not None:
        scale = fx.noise[0]
        d[10], d[11] = 1, int(fx.noise[1])
        d[12:13] = np.array([fx.noise[2]], np.uint32).view(np.int32)
    if fx is not None and fx.contrast is not None:
        d[15], d[16] = 1, lut_index
    if fx is not None and fx.sharpen is not None:
        kc, kn = sharpen_coefficients(fx.sharpen)
        d[17] = 1
    d[1] = r
    d[2:2 + len(q)] = q
    d[13:15] = np.array([scale], np.float64).view(np.int32)
    d[18:20] = np.array([kc, kn], _F32).view(np.int32)
    return d


# ----------------------------------------------------------------------------------------------------------- labels (host, exact)
def _t(a, b):            # a 0-dim float32 tensor meeting a Python number: the number is rounded to float32 first
    if isinstance(a, np.float32) or isinstance(b, np.float32):
        return _F32(a), _F32(b)
    return a, b


def _sub(a, b):
    a, b = _t(a, b)
    return a - b


def _min(a, b):          # Python's min / max over (tensor, float): compare in float32, keep the first on ties
    x, y = _t(a, b)
    return b if y < x else a


def _max(a, b):
    x, y = _t(a, b)
    return b if y > x else a


def filter_and_offset_labels(labels, boundary):
    """utils.py filter_and_offset_labels with its mixed float32 / double arithmetic; labels float32 [n,5]"""
    left, top, right, bottom = boundary
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for c, x0, y0, x1, y1 in labels:
            box_area = _F32(_F32(x1 - x0) * _F32(y1 - y0))
            dx = _sub(_min(x1, right), _max(x0, left))
            dy = _sub(_min(y1, bottom), _max(y0, top))
            if dx >= 0 and dy >= 0:
                p = _t(dx, dy)
                overlap = float(p[0] * p[1])
            else:
                overlap = 0
            if _F32(overlap) / box_area > _F32(0.5) or overlap > 1000:
                nx0, ny0 = _max(x0, left), _max(y0, top)
                nx1, ny1 = _min(x1, right), _min(y1, bottom)
                out.append([c, _sub(nx0, left), _sub(ny0, top), _sub(nx1, left), _sub(ny1, top)])
    if out:
        return np.array([[_F32(v) for v in r] for r in out], dtype=_F32)
    return np.zeros((len(labels), 5), _F32)


def sample_labels(boxes, geom, num_targets, aug=None):
    """ImageLabelDataset.__getitem__'s label half for raw CSV boxes [n,4] (x, y, h, w) -> float32 [num_targets, 5] (cls, cx, cy, w, h).
    `aug` with an affine: the boxes are warped between the patch offset / letterbox scale and the flip, as in the reference."""
    boxes = np.asarray(boxes, _F32).reshape(-1, 4)
    out = np.zeros((num_targets, 5), _F32)
    if len(boxes) == 0:
        return out
    l = np.zeros((len(boxes), 5), _F32)                      # add_class_dimension_to_labels, xyhw2xyxy_corner (class stays 0)
    l[:, 1], l[:, 2] = boxes[:, 0], boxes[:, 1]
    l[:, 3], l[:, 4] = boxes[:, 0] + boxes[:, 3], boxes[:, 1] + boxes[:, 2]
    if geom.ts:
        l[:, 1:5] = _F32(geom.scale) * l[:, 1:5]              # scale_labels
        l[:, 1:5] = l[:, 1:5] + np.array([geom.hp, geom.vp, geom.hp, geom.vp], _F32)   # add_padding_on_each_side
        l = filter_and_offset_labels(l, geom.boundary)
    else:
        l[:, 1:5] = l[:, 1:5] + np.array([geom.pad_w, geom.pad_h, geom.pad_w, geom.pad_h], _F32)
        l[:, 1:5] = _F32(geom.ratio) * l[:, 1:5]
    if aug is not None and aug.affine is not None:
        angle, translate, scale, shear = aug.affine
        l = affine_labels(geom.height, geom.width, l, -angle, translate, scale, (-shear, 0))
    if geom.flip:
        l[:, 1] = _F32(geom.width) - l[:, 1]
        l[:, 3] = _F32(geom.width) - l[:, 3]
    x = l[:, 1:5].copy()                                       # xyxy2xywh
    l[:, 1], l[:, 2] = (x[:, 0] + x[:, 2]) / _F32(2), (x[:, 1] + x[:, 3]) / _F32(2)
    l[:, 3], l[:, 4] = np.abs(x[:, 2] - x[:, 0]), np.abs(x[:, 3] - x[:, 1])
    l[:, (1, 3)] /= _F32(geom.width)
    l[:, (2, 4)] /= _F32(geom.height)
    if len(l) > num_targets:
        raise ValueError(f"{len(l)} labels for {num_targets} target rows")
    out[:len(l)] = l
    if (out < 0).any():
        raise ValueError("labels have negative values")
    return out


def read_label_csv(path, dataset_path):
    """ImageLabelDataset's CSV contract -> [(file, width, height, scale, boxes float32 [n,4])]: rows from the third line on, boxes are the
    JSON cells from column 5 on, rows with a negative coordinate are skipped with a warning."""
    rows = []
    with open(path) as f:
        for i, row in enumerate(csv.reader(f)):
            if i < 2:
                continue
            boxes = [json.loads(cell) for cell in row[5:] if cell]
            boxes = np.array(boxes, _F32).reshape(-1, 4) if boxes else np.zeros((0, 4), _F32)
            if (boxes < 0).any():
                warnings.warn(f"Image {os.path.join(dataset_path, row[0])} at line {i + 1} has negative bounding box coordinates; skipping")
                continue
            rows.append((os.path.join(dataset_path, row[0]), int(row[2]), int(row[3]), float(row[4]), boxes))
    return rows


# -------------------------------------------------------------------------------------------------------------------- the batch
def _align(n, a=16):
    return (n + a - 1) // a * a


class _Packed:
    pass


def frame_reference(geom, offset):
    """The MDCV_IMGLOAD_FREF words of a sample whose whole frame lies at byte `offset` of the pool: (off, pitch, x0, y0).  An empty
    window reads nothing; its origin (which may lie outside the frame) is replaced by (0, 0)."""
    x, y, w, h = geom.window
    if w == 0 or h == 0:
        x = y = 0
    return (int(offset), 3 * geom.frame[0], x, y)


def pack_layout(geoms, windows_nbytes, num_targets, frefs=None):
    """Byte layout of one batch's staging buffer: [descriptors][labels][coefficient tables][pixels], and behind them, only when a
    sample of the batch is augmented, [augmentation descriptors] (a batch without one is laid out exactly as before).  `frefs` (one
    frame reference per sample, `STAGED` for a staged one; a pooled sample's window has 0 bytes): the batch reads a frame cache, and
    [frame references] follow.  Only when a sample has an imgaug op, [fx descriptors][contrast tables] come last."""
    p = _Packed()
    B = len(geoms)
    p.B, p.T = B, num_targets
    p.desc_off, p.lab_off = 0, _align(B * DESC * 4)
    p.coef_off = _align(p.lab_off + B * num_targets * 5 * 4)
    n_coef = sum(g.col.size + g.row.size for g in geoms)
    p.n_coefs = max(n_coef, 1)
    p.pix_off = _align(p.coef_off + p.n_coefs * 4)
    p.src_bytes = sum(windows_nbytes)
    p.nbytes = _align(p.pix_off + p.src_bytes)
    p.aug = any(bool(getattr(g, "aug", None)) for g in geoms)
    if p.aug:
        p.aug_off = p.nbytes
        p.nbytes = _align(p.aug_off + B * AUG_DESC * 4)
    p.fref = frefs is not None
    if p.fref:
        p.fref_off = p.nbytes
        p.nbytes = _align(p.fref_off + B * FREF * 8)
    p.fx = any(bool(getattr(g, "fx", None)) and g.fx.runs() for g in geoms)
    if p.fx:
        p.n_luts = sum(1 for g in geoms if getattr(g, "fx", None) and g.fx.contrast is not None)
        p.fx_off = p.nbytes
        p.lut_off = _align(p.fx_off + B * FX_DESC * 4)
        p.nbytes = _align(p.lut_off + p.n_luts * 256)
    p.max_scr_w = max(g.desc[7] for g in geoms)
    p.max_scr_h = max(g.desc[8] for g in geoms)
    return p


def pack_batch(buf, p, geoms, windows, labels=None, frefs=None):
    """Fill a uint8 numpy buffer of at least p.nbytes bytes (the pinned staging) with the batch; a pooled sample's window is None."""
    desc = buf[p.desc_off:p.desc_off + p.B * DESC * 4].view(np.int32).reshape(p.B, DESC)
    coefs = buf[p.coef_off:p.coef_off + p.n_coefs * 4].view(np.int32)
    c, s = 0, 0
    for b, (g, w) in enumerate(zip(geoms, windows)):
        d = list(g.desc)
        d[0] = s
        d[5] = c
        coefs[c:c + g.col.size] = g.col.reshape(-1)
        c += g.col.size
        d[6] = c
        coefs[c:c + g.row.size] = g.row.reshape(-1)
        c += g.row.size
        desc[b] = d
        if w is not None:
            buf[p.pix_off + s:p.pix_off + s + w.nbytes] = w.reshape(-1)
            s += w.nbytes
    if p.aug:
        aug = buf[p.aug_off:p.aug_off + p.B * AUG_DESC * 4].view(np.int32).reshape(p.B, AUG_DESC)
        for b, g in enumerate(geoms):
            aug[b] = aug_descriptor(getattr(g, "aug", None))
    if p.fref:
        buf[p.fref_off:p.fref_off + p.B * FREF * 8].view(np.int64).reshape(p.B, FREF)[:] = np.asarray(frefs, np.int64).reshape(p.B, FREF)
    if p.fx:
        fxd = buf[p.fx_off:p.fx_off + p.B * FX_DESC * 4].view(np.int32).reshape(p.B, FX_DESC)
        luts = buf[p.lut_off:p.lut_off + p.n_luts * 256].reshape(p.n_luts, 256)
        n = 0
        for b, g in enumerate(geoms):
            fx = getattr(g, "fx", None)
            fxd[b] = fx_descriptor(fx, n)
            if fx and fx.contrast is not None:
                luts[n] = sigmoid_table(*fx.contrast)
                n += 1
    if p.T and labels is not None:
        buf[p.lab_off:p.lab_off + p.B * p.T * 20].view(np.float32)[:] = np.asarray(labels, np.float32).reshape(-1)


def launch_batch(dev_buf, host_buf, p, channels, height, width, stream, pool=None):
    """Enqueue the kernels on `stream` for a staged batch already copied to `dev_buf` (device uint8) -> imgs [B,C,H,W]: the pair of
    csrc/imgload.hip, or csrc/imgaug.hip's sequence when the batch carries augmentation descriptors.  A batch with frame references
    goes through the two `_frames_` entry points with `pool` (device uint8, or None): the same launches.  A batch with fx descriptors
    gets csrc/imgfx.hip's one launch behind them, out of place into a second batch buffer allocated here."""
    imgs = _launch_load(dev_buf, host_buf, p, channels, height, width, stream, pool)
    if not getattr(p, "fx", False):
        return imgs
    if channels != 3:
        raise ValueError("blur / noise / contrast / sharpen need RGB batches (bw=False)")
    out = torch.empty_like(imgs)
    base, hb = dev_buf.data_ptr(), host_buf.ctypes.data
    L = _lib.lib()
    L.check(L.imgfx_batch(hb + p.fx_off, base + p.fx_off, p.B, base + p.lut_off if p.n_luts else None, p.n_luts, channels, height, width,
                          imgs.data_ptr(), out.data_ptr(), stream.cuda_stream), "imgfx_batch")
    return out


def _launch_load(dev_buf, host_buf, p, channels, height, width, stream, pool):
    L = _lib.lib()
    dev = dev_buf.device
    imgs = torch.empty(p.B, channels, height, width, dtype=torch.float32, device=dev)
    wsb = L.imgload_workspace_bytes(p.B, p.max_scr_w, p.max_scr_h)
    ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=dev)
    base = dev_buf.data_ptr()
    hb = host_buf.ctypes.data
    if p.fref:
        frames = (hb + p.fref_off, base + p.fref_off)
        source = (base + p.pix_off, p.src_bytes, pool.data_ptr() if pool is not None else None, int(pool.numel()) if pool is not None else 0)
    if p.aug:
        awb = L.imgaug_workspace_bytes(p.B, height, width)
        if awb < 0:
            raise ValueError(f"augmented batches need 0 < H * W <= 4096 * 4096, got {height}x{width}")
        aws = torch.empty(int(awb), dtype=torch.uint8, device=dev)
        if p.fref:
            L.check(L.imgload_aug_frames_batch(hb + p.desc_off, base + p.desc_off, *frames, hb + p.aug_off, base + p.aug_off, p.B,
                                               base + p.coef_off, p.n_coefs, *source, p.max_scr_w, p.max_scr_h, channels, height, width,
                                               ws.data_ptr(), aws.data_ptr(), imgs.data_ptr(), stream.cuda_stream), "imgload_aug_frames_batch")
            return imgs
        L.check(L.imgload_aug_batch(hb + p.desc_off, base + p.desc_off, hb + p.aug_off, base + p.aug_off, p.B, base + p.coef_off, p.n_coefs,
                                    base + p.pix_off, p.src_bytes, p.max_scr_w, p.max_scr_h, channels, height, width, ws.data_ptr(),
                                    aws.data_ptr(), imgs.data_ptr(), stream.cuda_stream), "imgload_aug_batch")
        return imgs
    if p.fref:
        L.check(L.imgload_frames_batch(hb + p.desc_off, base + p.desc_off, *frames, p.B, base + p.coef_off, p.n_coefs, *source, p.max_scr_w,
                                       p.max_scr_h, channels, height, width, ws.data_ptr(), imgs.data_ptr(), stream.cuda_stream),
                "imgload_frames_batch")
        return imgs
    L.check(L.imgload_batch(host_buf.ctypes.data + p.desc_off, base + p.desc_off, p.B, base + p.coef_off, p.n_coefs, base + p.pix_off,
                            p.src_bytes, p.max_scr_w, p.max_scr_h, channels, height, width, ws.data_ptr(), imgs.data_ptr(),
                            stream.cuda_stream), "imgload_batch")
    return imgs


def transform_batch(frames, geoms, bw=False, device=None, pool=None, offsets=None):
    """Synchronous convenience (tests, probes): decoded frames [(H, W, 3) uint8] + their geometries (each may carry `.aug`, an
    `Augmentation` with its matrix set, and `.fx`, an `ImageFx`) -> imgs [B,C,H,W] fp32 on the device.  With `pool` (device uint8) and `offsets` (per sample: the
    byte offset in `pool` at which its whole frame already lies, rows of 3 * frame width bytes; None: stage the window from `frames`),
    pooled samples are read in place and their entry of `frames` is not looked at."""
    _lib.require_gpu()
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if pool is None:
        frefs = None
        windows = [crop_window(f, g) for f, g in zip(frames, geoms)]
    else:
        frefs = [STAGED if o is None else frame_reference(g, o) for g, o in zip(geoms, offsets)]
        windows = [crop_window(f, g) if o is None else None for f, g, o in zip(frames, geoms, offsets)]
    p = pack_layout(geoms, [0 if w is None else w.nbytes for w in windows], 0, frefs)
    host = np.zeros(p.nbytes, np.uint8)
    pack_batch(host, p, geoms, windows, frefs=frefs)
    with torch.cuda.device(device):
        dev = torch.from_numpy(host).to(device)
        return launch_batch(dev, host, p, 1 if bw else 3, geoms[0].height, geoms[0].width, torch.cuda.current_stream(device), pool)


def _default_decode(path):
    from PIL import Image
    return Image.open(path).convert("RGB")


class _Slot:
    def __init__(self):
        self.pinned, self.event = None, None


class ImageLabelBatches:
    """Iterable of `(uris, imgs [B,C,H,W] fp32, targets [B,T,5] fp32)` on the device, C = 1 when `bw` else 3: the batches that
    `DataLoader(ImageLabelDataset(path, dataset_path, width, height, ..., num_images, bw, lr_flip, ts), batch_size, shuffle)` yields.

    `decode(path)` -> a PIL image or an (H, W, 3) uint8 array (default: `PIL.Image.open(path).convert('RGB')`), run on `num_workers`
    threads.  `augment_hsv` / `augment_affine` / `data_aug` (both) turn on the reference's ColorJitter / affine augmentation, `blur` /
    `noise` / `contrast` / `sharpen` its four imgaug options (not with `bw`); `salt` is accepted and ignored, as the reference ignores it.
    `draws(epoch, index)` -> (patch_index, flip), (patch_index, flip, aug) or (patch_index, flip, aug, fx) overrides the random draws
    (tests); `aug` is None, an `Augmentation`, or a dict with `jitter` and / or `affine` in `Augmentation`'s form; `fx` is None, an
    `ImageFx`, or a dict with `blur`, `noise`, `contrast`, `sharpen` in `ImageFx`'s form; what is left out stays as drawn.  `subset_seed` seeds the
    `random.sample` of `num_images`; its default 0 is the `random.seed(0)` that CVC-YOLOv3/train.py:40 runs before it builds its
    loaders, so the training loader's subset is the one train.py draws.  `debug_mode` forces patch 0 as the reference does (the patch
    draw still happens first, so the flip draw is unchanged).  With `prefetch`, batch i+1 is decoded and
    staged while batch i is consumed; its copy runs on a side stream that the consumer's stream waits for when the batch is handed over.

    `cache_bytes`: None, or the HBM budget of a device-resident frame cache (mdcv/data/framecache.py).  Files are admitted
    in CSV order by their CSV sizes until the budget is used; an admitted file is decoded once in the loader's lifetime, its whole frame
    stays on the device, and from then on its samples stage no pixels: the resize reads their windows in place.  The batches are the
    same bytes with and without it.  `cache_stats()` counts what happened; `close()` frees the pool.
    """

    def __init__(self, path, dataset_path, width, height, num_images=-1, bw=False, lr_flip=False, ts=True, batch_size=1, shuffle=True,
                 num_workers=None, seed=0, device=None, decode=None, ud_flip=False, subset_seed=0, draws=None, prefetch=True, debug_mode=False,
                 augment_hsv=False, augment_affine=False, data_aug=False, cache_bytes=None, **options):
        self.blur, self.noise, self.contrast, self.sharpen = (bool(options.pop(k, False)) for k in ("blur", "noise", "contrast", "sharpen"))
        self.salt = options.pop("salt", False)                   # accepted and ignored: the reference stores it and never reads it
        if self.salt:
            warnings.warn("ImageLabelBatches: salt is ignored, as in the reference (ImageLabelDataset stores it and never reads it)")
        self._fx_on = self.blur or self.noise or self.contrast or self.sharpen
        if self._fx_on and bw:
            raise ValueError("ImageLabelBatches: blur / noise / contrast / sharpen cannot be combined with bw (the reference builds an "
                             "'RGB' image from the 2-D grayscale array there, which has no defined meaning)")
        for k in ("vis_batch", "upload_dataset", "n_cpu"):
            options.pop(k, None)
        if options:
            raise TypeError(f"ImageLabelBatches: unknown arguments {sorted(options)}")
        self.width, self.height, self.bw, self.lr_flip, self.ts = int(width), int(height), bool(bw), bool(lr_flip), bool(ts)
        self.ud_flip = ud_flip                                   # accepted and ignored, as in the reference
        self.augment_hsv, self.augment_affine, self.data_aug = bool(augment_hsv), bool(augment_affine), bool(data_aug)
        self.debug_mode = bool(debug_mode)
        self.batch_size, self.shuffle, self.seed = int(batch_size), bool(shuffle), int(seed)
        self.num_workers = int(num_workers) if num_workers is not None else max(1, min(16, os.cpu_count() or 1))
        self.decode, self.draws, self.prefetch = decode or _default_decode, draws, bool(prefetch)
        self._device = device
        self.img_files, self.labels, self.scales, self.sizes = [], [], [], []
        for file, w, h, scale, boxes in read_label_csv(path, dataset_path):
            n = n_patches(w, h, scale, self.width, self.height) if self.ts else 1
            self.img_files += [file] * n
            self.labels += [boxes] * n
            self.scales += [scale] * n
            self.sizes += [(w, h)] * n
        if num_images >= 0:
            idx = random.Random(subset_seed).sample(range(len(self.img_files)), k=num_images)
            if len(idx) > 1:                                     # the reference keeps everything for k <= 1
                for name in ("img_files", "labels", "scales", "sizes"):
                    v = getattr(self, name)
                    setattr(self, name, [v[i] for i in idx])
        self.num_targets_per_image = max((len(l) for l in self.labels), default=0)
        self.dataset = range(len(self.img_files))               # len(loader.dataset), as train.py prints it
        self.epoch = 0
        self._pool = None
        self._slots = [_Slot() for _ in range(3)]
        self._cache = None if cache_bytes is None else framecache.FrameCache(self.img_files, self.sizes, cache_bytes)

    def cache_stats(self):
        """None without `cache_bytes`; else hits / fills (samples that read the pool without / after decoding their file), misses by
        reason (samples staged the old way), bytes_reserved (by admission) and pool_bytes (allocated)."""
        return None if self._cache is None else self._cache.stats()

    def __len__(self):
        return (len(self.img_files) + self.batch_size - 1) // self.batch_size

    @property
    def channels(self):
        return 1 if self.bw else 3

    def order(self, epoch):
        idx = list(range(len(self.img_files)))
        if self.shuffle:
            random.Random(f"{self.seed}/{epoch}/order").shuffle(idx)
        return idx

    def plan(self, index, epoch=0, frame_size=None):
        """Host-only: the draws, geometry, augmentation (`.aug`: None or an `Augmentation` with its matrix; `.fx`: None or an `ImageFx`)
        and labels of sample `index` in `epoch` (frame_size: the decoded (W, H); default the CSV's)."""
        w, h = frame_size if frame_size is not None else self.sizes[index]
        rng = random.Random(f"{self.seed}/{epoch}/{index}")
        patch = rng.randint(0, n_patches(w, h, self.scales[index], self.width, self.height) - 1) if self.ts else 0
        if self.debug_mode:
            patch = 0
        boxed = len(self.labels[index]) > 0                          # raw-empty samples return before the augmentation and the flip
        aug = None
        if boxed and (self.augment_hsv or self.augment_affine or self.data_aug):
            aug = draw_augmentation(rng, self.augment_hsv or self.data_aug, self.augment_affine or self.data_aug)
        flip = bool(self.lr_flip and boxed and rng.random() > 0.5)
        fx = None
        if boxed and self._fx_on:
            fx = draw_imgfx(rng, lambda: random.Random(f"{self.seed}/{epoch}/{index}/imgaug"), self.blur, self.noise, self.contrast, self.sharpen)
        if self.draws is not None:
            d = self.draws(epoch, index)
            patch, flip = d[0], bool(d[1]) and boxed
            if len(d) > 2:
                aug = d[2] if boxed else None
                if isinstance(aug, dict):
                    aug = Augmentation(aug.get("jitter"), aug.get("affine"))
            if len(d) > 3:
                fx = d[3] if boxed else None
                if isinstance(fx, dict):
                    fx = ImageFx(fx.get("blur"), fx.get("noise"), fx.get("contrast"), fx.get("sharpen"))
                if fx and self.bw:
                    raise ValueError("blur / noise / contrast / sharpen cannot be combined with bw")
        if aug is not None and aug.affine is not None:
            aug.matrix = inverse_affine_matrix(self.width, self.height, *aug.affine)
        g = sample_geometry(w, h, self.width, self.height, self.ts, self.scales[index] if self.ts else 1.0, patch, flip)
        g.index, g.uri = index, self.img_files[index]
        g.aug = aug if aug else None
        g.fx = fx if fx else None
        g.labels = sample_labels(self.labels[index], g, self.num_targets_per_image, g.aug)
        return g

    # -- host half: decode, plan, crop, stage
    def _decode(self, path):
        img = self.decode(path)
        frame = img if isinstance(img, np.ndarray) else np.asarray(img, dtype=np.uint8)
        if frame.ndim != 3 or frame.shape[2] < 3 or frame.dtype != np.uint8:
            raise ValueError(f"{path}: decode must give an (H, W, 3) uint8 RGB frame, got {frame.shape} {frame.dtype}")
        return frame

    def _sample(self, epoch, index):
        """-> (geometry, window bytes or None, cache entry or None): a sample of a cached frame has no window, only its entry"""
        if self._cache is not None:
            ent, frame = self._cache.lookup(self.img_files[index], self._decode)
            if ent is not None:
                return self.plan(index, epoch, ent.size), None, ent
        else:
            frame = self._decode(self.img_files[index])
        g = self.plan(index, epoch, (frame.shape[1], frame.shape[0]))
        return g, crop_window(frame, g), None

    def _stage(self, epoch, bi, slot):
        order = self._orders[epoch]
        idx = order[bi * self.batch_size:(bi + 1) * self.batch_size]
        if self._pool is not None:
            got = list(self._pool.map(lambda i: self._sample(epoch, i), idx))
        else:
            got = [self._sample(epoch, i) for i in idx]
        geoms, windows, ents = [g for g, _, _ in got], [w for _, w, _ in got], [e for _, _, e in got]
        frefs, fills = None, []
        if any(e is not None for e in ents):                     # a batch with no cached sample is staged and launched as without a cache
            frefs = [STAGED if e is None else frame_reference(g, e.offset) for g, e in zip(geoms, ents)]
            fills = self._cache.take_fills(ents)
        p = pack_layout(geoms, [0 if w is None else w.nbytes for w in windows], self.num_targets_per_image, frefs)
        p.fills, need = [], p.nbytes                             # first sight: the whole frames ride behind the batch, one copy each
        for e in fills:
            p.fills.append((e, need))
            need = _align(need + e.nbytes)
        if slot.event is not None:
            slot.event.synchronize()                             # the previous copy out of this buffer has completed
        if slot.pinned is None or slot.pinned.numel() < need:
            slot.pinned = torch.empty(_align(need, 1 << 20), dtype=torch.uint8, pin_memory=True)
        host = slot.pinned.numpy()
        pack_batch(host, p, geoms, windows, [g.labels for g in geoms], frefs)
        for e, at in p.fills:
            host[at:at + e.nbytes] = e.frame.reshape(-1)
        return [g.uri for g in geoms], p, slot

    # -- device half: one H2D copy and the kernel pair on the side stream
    def _enqueue(self, staged):
        uris, p, slot = staged
        dev = self.device
        with torch.cuda.device(dev), torch.cuda.stream(self._stream):
            dbuf = torch.empty(p.nbytes, dtype=torch.uint8, device=dev)
            dbuf.copy_(slot.pinned[:p.nbytes], non_blocking=True)
            pool = None
            if p.fref:
                pool = self._cache.pool
                for e, at in p.fills:                            # pinned -> the file's slot, in front of this batch's kernels
                    pool[e.offset:e.offset + e.nbytes].copy_(slot.pinned[at:at + e.nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
            slot.event = ev
            if p.fref:
                self._cache.filled([e for e, _ in p.fills], ev)
            imgs = launch_batch(dbuf, slot.pinned.numpy(), p, self.channels, self.height, self.width, self._stream, pool)
            tg = dbuf[p.lab_off:p.lab_off + p.B * p.T * 20].view(torch.float32).view(p.B, p.T, 5).clone()
            ready = torch.cuda.Event()
            ready.record(self._stream)
        return uris, imgs, tg, ready

    @property
    def device(self):
        if self._device is None:
            return torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._device)

    def __iter__(self):
        _lib.require_gpu()
        epoch = self.epoch
        self.epoch += 1
        self._orders = {epoch: self.order(epoch)}
        dev = self.device
        self._stream = torch.cuda.Stream(dev)
        if self._cache is not None:
            self._cache.restart()
            if self._cache.pool is None:
                with torch.cuda.device(dev):
                    if self._cache.ensure_pool(dev) is not None:  # allocated on the consumer's stream, written on the side streams
                        self._stream.wait_stream(torch.cuda.current_stream(dev))
            if self._cache.last_fill is not None:                # slots filled on an earlier epoch's stream, read on this one
                self._stream.wait_event(self._cache.last_fill)
        nb = len(self)
        if self.num_workers > 1 and self._pool is None:
            self._pool = ThreadPoolExecutor(self.num_workers, thread_name_prefix="mdcv-decode")
        stager = ThreadPoolExecutor(1, thread_name_prefix="mdcv-stage") if self.prefetch else None
        try:
            pending = {}
            depth = 2 if self.prefetch else 0
            for bi in range(nb):
                for j in range(bi, min(nb, bi + depth + 1)):
                    if j not in pending and self.prefetch:
                        pending[j] = stager.submit(self._stage, epoch, j, self._slots[j % 3])
                staged = pending.pop(bi).result() if self.prefetch else self._stage(epoch, bi, self._slots[bi % 3])
                uris, imgs, tg, ready = self._enqueue(staged)
                cons = torch.cuda.current_stream(dev)
                cons.wait_event(ready)
                imgs.record_stream(cons)
                tg.record_stream(cons)
                yield uris, imgs, tg
        finally:
            if stager is not None:
                stager.shutdown(wait=True, cancel_futures=True)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        if self._cache is not None:
            if self._cache.pool is not None and getattr(self, "_stream", None) is not None:
                self._cache.pool.record_stream(self._stream)     # the last epoch's kernels may still read it
            self._cache.close()
