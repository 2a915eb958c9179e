"""Shared by tests/test_anchors_host.py and tests/test_gpu_anchors.py: kmeans_anchors with the restatement in the kernel's place, and a
small raw dataset in the published label format."""
import os

import numpy as np

import anchor_refs as ar
from mdcv.data import prep


def host_kmeans(boxes_hw, num_clst=9, *, seed=0, restarts=1, init=None, check_every=8, max_iter=10000):
    """kmeans_anchors with the restatement in the kernel's place (shared with tests/test_gpu_anchors.py)"""
    pts = prep.check_boxes(boxes_hw)
    idx = prep.initial_indices(len(pts), num_clst, seed, restarts) if init is None else np.asarray(init)
    runs = [ar.lloyd(pts, i, max_iter) for i in idx]
    d, n = [r["distortion"] for r in runs], [r["nan"] for r in runs]
    best = prep.select_best(d, n)
    if best is None:
        raise ValueError("every restart ended with an empty cluster")
    return prep.AnchorKMeans(runs[best]["centroids"], runs[best]["assign"], runs[best]["iterations"], d, n, best,
                             np.array([r["centroids"] for r in runs]), np.array([r["iterations"] for r in runs]))


def write_raw_dataset(root, n_rows=12):
    """a handful of PNGs of two sizes and a raw label file in the published format; row 3 has no box, row 5 has three"""
    from PIL import Image
    rng = np.random.default_rng(3)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    sizes = [(96, 64), (80, 112)]
    lines = ["exported labels\n", "Name,URL,boxes\n"]
    for i in range(n_rows):
        W, H = sizes[i % 2]
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "images", f"f{i}.png"))
        cells = []
        for _ in range(0 if i == 3 else 3 if i == 5 else 2):
            h = int(rng.integers(8, 40))
            w = int(rng.integers(4, 30))
            cells.append('"[%d, %d, %d, %d]"' % (rng.integers(0, W - w), rng.integers(0, H - h), h, w))
        if i == 4:
            cells.insert(1, "")                                               # an empty cell between two boxes stays in the row
        lines.append(",".join([f"f{i}.png", f"http://x/f{i}.png"] + cells) + "\n")
    src = os.path.join(root, "raw.csv")
    with open(src, "w") as f:
        f.writelines(lines)
    return src, os.path.join(root, "images")
