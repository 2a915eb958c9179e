"""Frame layout of both modes (CVC-YOLOv3/utils/utils.py's geometry helpers) and the per-sample geometry the resize kernel reads.

The arithmetic below is what makes the labels exact, so its form is fixed: Python ints where the layout is whole pixels, int()
truncation toward zero of the letterbox border, ceil of half the missing width, and patch starts that stay unrounded floats."""
import math

import numpy as np

from .resample import BILINEAR, LANCZOS, resample_coeffs


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


class Geometry:
    """Where one output image comes from: the frame window to upload (frame x, y, w, h), its kernel descriptor (offsets left 0) and
    tables, and the quantities the label pipeline needs (paddings, the unrounded patch boundary, the pad-and-resize ratio)."""
    aug = fx = None                          # a loader's plan(): None or an `Augmentation` with its matrix / an `ImageFx`
    labels = index = uri = None              # and the sample's labels, index and file

    def __init__(self, ts, frame, width, height, scale, patch_index, flip, window, desc, col, row, n_patches=1, hp=None, vp=None,
                 boundary=None, ratio=None, pad_w=None, pad_h=None):
        self.ts, self.frame, self.width, self.height, self.scale = ts, frame, width, height, scale
        self.patch_index, self.flip, self.window, self.desc, self.col, self.row = patch_index, flip, window, desc, col, row
        self.n_patches, self.hp, self.vp, self.boundary = n_patches, hp, vp, boundary      # tile-and-scale: borders, unrounded patch box
        self.ratio, self.pad_w, self.pad_h = ratio, pad_w, pad_h                            # pad-and-resize: letterbox()'s


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
        g = dict(hp=hp, vp=vp, boundary=boundary, n_patches=n)
    else:
        pad_w, pad_h, ratio = letterbox(frame_w, frame_h, width, height)
        pw_, ph_ = frame_w + 2 * pad_w, frame_h + 2 * pad_h
        if pw_ <= 0 or ph_ <= 0:
            raise ValueError(f"padding {pad_w},{pad_h} leaves nothing of a {frame_w}x{frame_h} frame")
        ax = _axis(pw_, width, BILINEAR, 0, width, pad_w, pad_w + frame_w)
        ay = _axis(ph_, height, BILINEAR, 0, height, pad_h, pad_h + frame_h)
        pad_x, pad_y = (0, width), (0, height)
        g = dict(ratio=ratio, pad_w=pad_w, pad_h=pad_h)
    win = (ax["w0"] - ax["src_lo"], ay["w0"] - ay["src_lo"], ax["w1"] - ax["w0"], ay["w1"] - ay["w0"])
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


def frame_reference(geom, offset):
    """The MDCV_IMGLOAD_FREF words of a sample whose whole frame lies at byte `offset` of the pool: (off, pitch, x0, y0).  An empty
    window reads nothing; its origin (which may lie outside the frame) is replaced by (0, 0)."""
    x, y, w, h = geom.window
    if w == 0 or h == 0:
        x = y = 0
    return (int(offset), 3 * geom.frame[0], x, y)
