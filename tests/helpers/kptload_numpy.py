"""NumPy side of the key-point crop loader (csrc/kptload.hip, mdcv/data/crops.py): ConeDataset.__getitem__ (RektNet/dataset.py:34-56) for
one decoded crop, COMPOSED from the oracle's existing restatements -- `resize_bilinear_u8` for prep_image, `_resize_onehot_axis` and
`_blur_reflect101` for prep_label -- without restating either rule again.  Test infrastructure only: the product never imports it."""
import math

import numpy as np

from oracle.pipeline_oracle import resize_bilinear_u8
from oracle.synth_oracle import _blur_reflect101, _resize_onehot_axis

F = np.float32


def image(crop_rgb, size):
    """(h, w, 3) uint8 RGB -> [3, S, S] float32, planes B, G, R: cv2.resize of the 8-bit image, then `transpose / 255.0` in float64"""
    bgr = np.ascontiguousarray(np.asarray(crop_rgb)[:, :, 2::-1].transpose(2, 0, 1))
    return (resize_bilinear_u8(bgr, size, size).astype(np.float64) / 255.0).astype(F)


def resized_axis(hot, src, size):
    """the resized one-hot of one axis before the blur, float64 [S]"""
    return _resize_onehot_axis(int(hot), int(src), int(size))


def axis_vector(hot, src, size):
    """the blurred, resized one-hot of one axis, float64 [S]"""
    return _blur_reflect101(resized_axis(hot, src, size))


def heatmap(x, y, h, w, size):
    """prep_label for one key point at label (x, y) of an h x w crop -> float32 [S, S]; all NaN when the total is 0 (0 / 0)"""
    vy, vx = axis_vector(int(y), h, size), axis_vector(int(x), w, size)
    tot = sum(vy.tolist()) * sum(vx.tolist())                 # sequential float64 sums (index order), as cone_crops and the kernel
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.outer(vy, vx) / tot).astype(F)


def points(label, h, w, size):
    """scale_labels(label, size / h, size / w) / size (RektNet/utils.py:98-111, dataset.py:41-43) -> float32 [n, 2]"""
    hs, ws = size / h, size / w
    return np.array([[math.ceil(int(px) * ws) / size, math.ceil(int(py) * hs) / size] for px, py in np.asarray(label)], np.float64).astype(F)


def sample(crop_rgb, label, size):
    """-> (image [3,S,S], heatmaps [n,S,S], points [n,2])"""
    h, w = crop_rgb.shape[:2]
    hm = np.stack([heatmap(px, py, h, w, size) for px, py in np.asarray(label)])
    return image(crop_rgb, size), hm, points(label, h, w, size)


def batch(crops, labels, size):
    got = [sample(c, l, size) for c, l in zip(crops, labels)]
    return tuple(np.stack([g[i] for g in got]) for i in range(3))


def make_crop(h, w, seed):
    """a deterministic (h, w, 3) uint8 crop with gradients, noise and hard edges"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), (3 * x + 5 * y) % 256], -1).astype(np.int16)
    img += rng.integers(-40, 41, img.shape, dtype=np.int16)
    img[h // 3:h // 2, w // 4:w // 2] = (255, 0, 128)
    return np.clip(img, 0, 255).astype(np.uint8)


def make_label(h, w, seed):
    """seven (x, y) labels with fractional parts, inside the crop"""
    rng = np.random.default_rng(seed + 1000)
    return np.stack([rng.uniform(0, w, 7), rng.uniform(0, h, 7)], -1)
