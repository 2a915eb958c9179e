"""Labels: the reference's helpers restated in NumPy with torch's arithmetic (float32 tensors; a Python scalar meeting one is rounded to
float32 first; `filter_and_offset_labels` mixes 0-dim float32 tensors with Python doubles), computed on the host and shipped with the
pixels in the same pinned buffer and the same copy.  The boxes of an affine sample follow `affine_labels` in float32 torch CPU
arithmetic, in the reference's sequence of operations."""
import csv
import json
import math
import os
import warnings

import numpy as np
import torch

_F32 = np.float32


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
