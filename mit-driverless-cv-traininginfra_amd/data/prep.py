"""Dataset preparation: from a raw label file to the `train.csv` that `Darknet(cfg)` and `ImageLabelBatches` read -- the reference's
CVC-YOLOv3/generate_kmeans_dataset_csvs.py, working and reproducible, with the k-means on the device (csrc/anchors.hip).

    python -m mdcv.data.prep --input_csvs all.csv --dataset_path images/ --output_path dataset/ --restarts 16

`prepare_dataset` follows the reference's `main` step by step: image sizes, one camera scale per image-size group from the 5th / 95th
percentile box heights, all scaled boxes clustered into `num_clst` anchors, the rows split by `i % 100` into five CSV files with the
anchors in row 0 of train.csv.  Everything but the clustering is host work in Python floats, one operation at a time.  Departures from
the reference ("Dataset preparation"):

  - boxes are the JSON cells `[x, y, h, w]` of the published label format (the reference's `int(row[2])` cannot read them); a row may
    hold any number of boxes, also none
  - image sizes come from the file header through Pillow, without a decode and without EXIF rotation: the size ImageLabelBatches sees
  - the initial centroids are drawn from `np.random.RandomState(seed)`: two runs give the same anchors; `restarts` > 1 keeps the restart
    with the smallest distortion
  - anchors are written with `repr(float)`, and as (w, h) by default, the order `Darknet` reads (`anchor_order="hw"`: the reference's)
  - an empty cluster raises instead of writing `nan`
  - without a box-less validation row nothing is traded (the reference then moves EVERY labelled training row to the validation file:
    its counter can never equal zero; `split_rows(..., reference_trade=True)` keeps that behaviour for comparison)
  - `anchors.txt` goes to `output_path`, not the working directory; there are no plots

`kmeans_anchors` is the clustering alone."""
import argparse
import collections
import csv
import json
import os

import numpy as np

MAX_K, MAX_R = 16, 64                        # MDCV_KMEANS_MAX_K, MDCV_KMEANS_MAX_R
REC_HEAD = 4                                 # MDCV_KMEANS_REC_HEAD
MAX_N = 1 << 24
COORD_LIMIT = 16384.0                        # |x| < 2^14
NOTES = "please see k-means anchor boxes in train.csv"
SECOND_ROW = ['Name', 'URL', 'Width', 'Height', 'Scale', 'X0, Y0, H0, W0', 'X1, Y1, H1, W1', 'etc', '\n']
FILES = ("train.csv", "test.csv", "validate.csv", "train-validate.csv", "all.csv")

AnchorKMeans = collections.namedtuple(
    "AnchorKMeans", "centroids assignment iterations distortions nan best all_centroids all_iterations")
AnchorKMeans.__doc__ = """centroids [K,2] fp64 (h, w), assignment uint8 [N] and iterations of the BEST restart; per restart: distortions
(Python integers), nan (a centroid is NaN), all_centroids [R,K,2], all_iterations [R]; best = the chosen restart's index"""


# ----------------------------------------------------------------------------------------------------------------------- k-means
def check_boxes(boxes_hw):
    """-> float64 [N,2], or ValueError naming the first box the kernel's fixed-point sums cannot hold exactly"""
    pts = np.ascontiguousarray(np.asarray(boxes_hw, dtype=np.float64))
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"kmeans_anchors: boxes must be [N,2] (h, w), got shape {pts.shape}")
    n = len(pts)
    if not 1 <= n < MAX_N:
        raise ValueError(f"kmeans_anchors: needs 1 <= N < 2^24 boxes, got {n}")
    finite = np.isfinite(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        small = np.abs(pts) < COORD_LIMIT
        scaled = np.where(finite & small, pts, 0.0) * 2.0 ** 64          # exact: a power of two, no overflow
        whole = np.floor(scaled) == scaled
    bad = ~(finite & small & whole)
    if bad.any():
        i = int(np.argmax(bad.any(axis=1)))
        why = ("is not finite" if not finite[i].all() else "has a coordinate of magnitude >= 2^14" if not small[i].all()
               else "is not a multiple of 2^-64")
        raise ValueError(f"kmeans_anchors: box {i} = ({pts[i, 0]!r}, {pts[i, 1]!r}) {why}")
    return pts


def initial_indices(n, num_clst, seed, restarts):
    """[R][K] box indices: restart r, cluster i is draw number r*K + i of np.random.RandomState(seed).randint(0, N), one call per draw --
    restart 0 is what the reference picks after np.random.seed(seed)"""
    rs = np.random.RandomState(seed)
    return np.array([[int(rs.randint(0, n)) for _ in range(num_clst)] for _ in range(restarts)], dtype=np.int32).reshape(restarts, num_clst)


def select_best(distortions, nans):
    """the restart with the smallest distortion among those without a NaN centroid, the lowest index on ties; None if there is none"""
    best = None
    for r, (d, bad) in enumerate(zip(distortions, nans)):
        if not bad and (best is None or d < distortions[best]):
            best = r
    return best


def kmeans_anchors(boxes_hw, num_clst=9, *, seed=0, restarts=1, init=None, check_every=8, max_iter=10000):
    """Lloyd's k-means over boxes (h, w) on the GPU, `restarts` initialisations at once -> AnchorKMeans.

    The arithmetic is the reference's `assignment` / `update` with exact cluster sums (include/mdcv_hip.h), so a restart stops at the first
    iteration that repeats its assignment, exactly.  The host enqueues `check_every` iterations at a time and reads one small record per
    chunk.  init: [R][K] box indices instead of the seeded draws.  RuntimeError after `max_iter` iterations without a fixed point;
    ValueError if every restart ends with an empty cluster (a NaN centroid)."""
    import torch
    from .. import _lib
    pts = check_boxes(boxes_hw)
    n = len(pts)
    if not 1 <= int(num_clst) <= MAX_K:
        raise ValueError(f"kmeans_anchors: num_clst must be in 1..{MAX_K}, got {num_clst}")
    K = int(num_clst)
    if init is None:
        if not 1 <= int(restarts) <= MAX_R:
            raise ValueError(f"kmeans_anchors: restarts must be in 1..{MAX_R}, got {restarts}")
        idx = initial_indices(n, K, seed, int(restarts))
    else:
        idx = np.asarray(init)
        if idx.ndim != 2 or idx.shape[1] != K or not 1 <= idx.shape[0] <= MAX_R or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"kmeans_anchors: init must be integer indices [R][{K}] with 1 <= R <= {MAX_R}")
        if (idx < 0).any() or (idx >= n).any():
            raise ValueError(f"kmeans_anchors: init indices must be in 0..{n - 1}")
        idx = np.ascontiguousarray(idx.astype(np.int32))
    R = idx.shape[0]
    if check_every < 1 or max_iter < 1:
        raise ValueError("kmeans_anchors: check_every and max_iter must be >= 1")
    _lib.require_gpu()
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    nbytes = L.kmeans_workspace_bytes(n, K, R)
    if nbytes < 0:
        raise _lib.MdcvError("kmeans_workspace_bytes refused the shape")
    rec_words = REC_HEAD + 2 * K
    d_pts = torch.from_numpy(pts).to(dev)
    d_init = torch.from_numpy(idx).to(dev)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    assign = torch.empty(R * n, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(R * rec_words, dtype=torch.int64, device=dev)
    h_rec = torch.empty(R * rec_words, dtype=torch.int64).pin_memory()
    stream = torch.cuda.current_stream(dev)
    L.check(L.kmeans_begin(ws.data_ptr(), d_pts.data_ptr(), d_init.data_ptr(), n, K, R, stream.cuda_stream), "kmeans_begin")
    done = 0                                   # steps enqueued: step 0 is the initial assignment, steps 1.. are the iterations
    while True:
        steps = min(check_every + (1 if done == 0 else 0), max_iter + 1 - done)
        L.check(L.kmeans_steps(ws.data_ptr(), d_pts.data_ptr(), assign.data_ptr(), d_rec.data_ptr(), n, K, R, done, steps,
                               stream.cuda_stream), "kmeans_steps")
        h_rec.copy_(d_rec, non_blocking=True)
        stream.synchronize()                   # the chunk's one host read
        done += steps
        rec = h_rec.numpy().reshape(R, rec_words)
        if (rec[:, 0] >= 0).all():
            break
        if done > max_iter:
            raise RuntimeError(f"kmeans_anchors: {int((rec[:, 0] < 0).sum())} of {R} restarts reached no fixed point in {max_iter} iterations")
    rec = rec.copy()
    iters = rec[:, 0].astype(np.int64)
    distortions = [(int(rec[r, 2]) << 32) + int(rec[r, 1]) for r in range(R)]
    nans = [bool(rec[r, 3]) for r in range(R)]
    cents = rec[:, REC_HEAD:].copy().view(np.float64).reshape(R, K, 2)
    best = select_best(distortions, nans)
    if best is None:
        raise ValueError(f"kmeans_anchors: every restart ended with an empty cluster (a NaN centroid); initial indices {idx.tolist()}")
    a = assign[best * n:(best + 1) * n].cpu().numpy()
    return AnchorKMeans(cents[best].copy(), a, int(iters[best]), distortions, nans, best, cents, iters)


# ------------------------------------------------------------------------------------------------------------------ the host steps
def read_raw_labels(csv_uri, dataset_path):
    """-> [(row as read, image width, image height, [(h, w), ..])] for every row from the third line on; a row is `Name, URL, box cells..`,
    its boxes all non-empty JSON cells `[x, y, h, w]` from column 2 on.  The size is read from the image header; a missing file raises."""
    from PIL import Image
    out = []
    with open(csv_uri) as f:
        next(f)                                                     # the reference skips a line, then the row at index 0
        for i, row in enumerate(csv.reader(f)):
            if i < 1:
                continue
            path = os.path.join(dataset_path, row[0])
            if not os.path.isfile(path):
                raise FileNotFoundError(f"{csv_uri}: row {i + 2} names an image that is not there: {path}")
            with Image.open(path) as im:
                img_w, img_h = im.size
            boxes = []
            for cell in row[2:]:
                if cell == "":
                    continue
                b = json.loads(cell)
                if not (isinstance(b, list) and len(b) == 4):
                    raise ValueError(f"{csv_uri}: row {i + 2} ({row[0]}): box cell {cell!r} is not [x, y, h, w]")
                boxes.append((b[2], b[3]))
            out.append((row, img_w, img_h, boxes))
    return out


def camera_scales(box_dict, max_cone=83, min_cone=10):
    """box_dict {(img_h, img_w): [(h, w), ..]} in first-seen order -> (scale {(img_h, img_w): h_ratio}, scaled heights, scaled widths), the
    reference's lines 100-132: per group the boxes stable-sorted by h, max = sorted[int(.95 n) - 1], min = sorted[int(.05 n)],
    h_ratio = (max_cone - min_cone) / (max_h - min_h), scaled = (x - min_x) * h_ratio + min_cone, w with the SAME ratio."""
    scale, hs, ws = {}, [], []
    for key, group in box_dict.items():
        boxes = sorted(group, key=lambda x: x[0])
        max_h, max_w = boxes[int(.95 * len(boxes)) - 1]
        min_h, min_w = boxes[int(0.05 * (len(boxes)))]
        h_ratio = (max_cone - min_cone) / (max_h - min_h)
        scale[key] = scale.get(key, 0) + h_ratio
        for box_h, box_w in group:
            hs.append((box_h - min_h) * h_ratio + min_cone)
            ws.append((box_w - min_w) * h_ratio + min_cone)
    return scale, hs, ws


def split_rows(rows, split_up=(75, 15, 0), *, reference_trade=False):
    """rows `[Name, URL, Width, Height, Scale, cells..]` -> dict of the five row lists.  Row i goes by i % 100: below split_up[0] to train,
    below split_up[0] + split_up[1] to validate, else to test; train-validate and all keep that first membership.  Then the validation
    rows without a box go to the END of train, and as many labelled rows from the FRONT of train go to the end of validate.
    reference_trade: with no box-less validation row the reference moves every labelled training row (docstring of the module)."""
    train, validate, test, train_validate, every = [], [], [], [], []
    for i, row in enumerate(rows):
        every.append(row)
        remainder = i % 100
        if remainder < int(split_up[0]):
            train.append(row)
            train_validate.append(row)
        elif remainder < int(split_up[0]) + int(split_up[1]):
            validate.append(row)
            train_validate.append(row)
        else:
            test.append(row)
    empty = [row for row in validate if "" == "".join(str(c) for c in row[5:])]
    for row in empty:
        validate.remove(row)
    compensate = []
    if empty or reference_trade:
        for row in train:
            if not "" == "".join(str(c) for c in row[5:]):
                compensate.append(row)
                if len(compensate) == len(empty):
                    break
    for row in compensate:
        train.remove(row)
    train.extend(empty)
    validate.extend(compensate)
    return {"train.csv": train, "test.csv": test, "validate.csv": validate, "train-validate.csv": train_validate, "all.csv": every,
            "traded": len(empty)}


def anchor_row(centroids_hw, anchor_order="wh"):
    """row 0 of train.csv: the anchors sorted by h*w, each `repr(float(a)) + ", " + repr(float(b))`, joined by `|` -- the text numpy 1.x's
    `str([a, b])[1:-1]` gave the reference.  "wh": (w, h), what Darknet reads; "hw": the reference's order."""
    if anchor_order not in ("wh", "hw"):
        raise ValueError('anchor_order must be "wh" or "hw"')
    anchors = [[float(c[0]), float(c[1])] for c in centroids_hw]
    anchors.sort(key=lambda x: x[0] * x[1])
    if anchor_order == "wh":
        anchors = [[a[1], a[0]] for a in anchors]
    return "|".join(repr(a[0]) + ", " + repr(a[1]) for a in anchors)


def write_csvs(output_path, split, first_row):
    """the five files, as the reference's csv.writer writes them: row 0 = the anchors (train.csv) or the note, row 1 = the column names"""
    for name in FILES:
        with open(os.path.join(output_path, name), "w") as f:
            w = csv.writer(f)
            w.writerow([first_row if name == "train.csv" else NOTES])
            w.writerow(SECOND_ROW)
            for row in split[name]:
                w.writerow(row)


def prepare_dataset(csv_uri, dataset_path, output_path, num_clst=9, max_cone=83, min_cone=10, if_plot=False, split_up=(75, 15, 0), *,
                    seed=0, restarts=1, anchor_order="wh"):
    """The reference's `main` (module docstring) -> the AnchorKMeans of the clustering.  Writes train.csv, validate.csv, test.csv,
    train-validate.csv, all.csv and anchors.txt into `output_path`."""
    if anchor_order not in ("wh", "hw"):
        raise ValueError('anchor_order must be "wh" or "hw"')
    if if_plot:
        print("if_plot: the reference's scatter plots are not produced here")
    raw = read_raw_labels(csv_uri, dataset_path)
    box_dict = {}
    for _, img_w, img_h, boxes in raw:
        if boxes:
            box_dict[(img_h, img_w)] = box_dict.get((img_h, img_w), []) + boxes
    if not box_dict:
        raise ValueError(f"{csv_uri}: no row holds a box")
    scale, hs, ws = camera_scales(box_dict, max_cone, min_cone)
    for (h, w), s in scale.items():
        print("{height}x{width} images are scaled by {scale}".format(height=h, width=w, scale=s))
    km = kmeans_anchors(np.array([hs, ws], dtype=np.float64).T, num_clst, seed=seed, restarts=restarts)
    rows = []
    for row, img_w, img_h, _ in raw:
        if (img_h, img_w) not in scale:
            raise ValueError(f"{row[0]}: no box in any {img_h}x{img_w} image, so images of that size have no scale")
        rows.append(row[:2] + [img_w, img_h, scale[(img_h, img_w)]] + row[2:])
    split = split_rows(rows, split_up)
    print(str(split["traded"]) + " '0 label images' got traded from validation set to training set.")
    os.makedirs(output_path, exist_ok=True)
    with open(os.path.join(output_path, "anchors.txt"), "w") as f:
        for c in km.centroids:                                       # the reference's file: h,w per cluster, in cluster order
            f.write('%0.2f,%0.2f \n' % (c[0], c[1]))
    write_csvs(output_path, split, anchor_row(km.centroids, anchor_order))
    return km


def main(argv=None):
    ap = argparse.ArgumentParser(description="raw label CSV -> camera scales, k-means anchors and the train / validate / test CSVs")
    ap.add_argument("--input_csvs", default="dataset/all.csv", help="the raw label file: two header lines, then Name, URL, box cells")
    ap.add_argument("--dataset_path", default="dataset/YOLO_Dataset/", help="directory of the images the label file names")
    ap.add_argument("--output_path", default="dataset/", help="directory the five CSV files and anchors.txt are written to")
    ap.add_argument("--num_clst", type=int, default=9, help="number of anchors")
    ap.add_argument("--max_cone_height", type=int, default=83, help="height the 95th-percentile box of every camera is scaled to")
    ap.add_argument("--min_cone_height", type=int, default=10, help="height the 5th-percentile box of every camera is scaled to")
    ap.add_argument("--split_up", default="75-15-0", help="train-validate-test shares of every 100 rows")
    ap.add_argument("--seed", type=int, default=0, help="seed of the initial centroids")
    ap.add_argument("--restarts", type=int, default=1, help="k-means initialisations; the one with the smallest distortion is kept")
    ap.add_argument("--anchor_order", choices=("wh", "hw"), default="wh", help="wh: what Darknet reads; hw: the reference's order")
    ap.add_argument("--if_plot", dest="if_plot", action="store_true", default=False, help="accepted for compatibility: no plots are produced")
    ap.add_argument("--no_if_plot", dest="if_plot", action="store_false", help="accepted for compatibility")
    opt = ap.parse_args(argv)
    prepare_dataset(csv_uri=opt.input_csvs, dataset_path=opt.dataset_path, output_path=opt.output_path, num_clst=opt.num_clst,
                    max_cone=opt.max_cone_height, min_cone=opt.min_cone_height, if_plot=opt.if_plot,
                    split_up=[int(x) for x in opt.split_up.split('-')], seed=opt.seed, restarts=opt.restarts,
                    anchor_order=opt.anchor_order)


if __name__ == "__main__":
    main()
