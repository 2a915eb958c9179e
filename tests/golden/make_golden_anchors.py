"""Writes tests/golden/anchors.npz from a checkout of the reference project (cv-core/MIT-Driverless-CV-TrainingInfra):

    python tests/golden/make_golden_anchors.py <path to the reference checkout>

The reference's CVC-YOLOv3/generate_kmeans_dataset_csvs.py is imported from that checkout at run time, with an empty stand-in module
registered as `cv2` (only its `main` uses cv2, and cv2 is not installed here).  The fixture is DATA: inputs and recorded results, numbers
only -- never the reference's formatted anchor string, which under numpy >= 2 holds `np.float64(...)` text.

  k-means, the reference's own `assignment` / `update` driven as the loop of its `main` (lines 139-149) drives them:
    <set>::points          [n,2] fp64   scaled boxes (h, w); sets: "dyadic" (ratio 0.25: every sum is exact in any order), "generic"
                                        (ratio 73 / (max_h - min_h))
    <set>::seeds           [4]          np.random.seed(seed) before the draws
    <set>::init            [4,K]        the drawn box indices
    <set>::centroids       [4,K,2] fp64 after the loop
    <set>::assign          [4,n]        the last `closest` column
    <set>::iterations      [4]          passes of the while loop
    repeat::*              the same for one run on the dyadic set whose initial indices repeat one box (an empty cluster: NaN)

  scales and splits, `main` itself in a temporary directory on the one input shape its code accepts (integer h, w in columns 2 and 3;
  `cv2.imread` stood in by Pillow), 230 rows, two image sizes, many boxes of equal height:
    main::names, main::sizes [n,2] (W,H of the image written), main::hw [n,2]   the input
    main::scale            [n] fp64     the Scale column of all.csv
    main::wh_cols          [n,2]        its Width and Height columns
    main::anchors_txt      [K,2] fp64   the numbers of anchors.txt (h, w to two decimals, cluster order) after np.random.seed(0)
    main::<file>           names in each of the five files, in file order
    main::head_note, main::second_row    row 0 of validate.csv, and row 1 as csv.reader returns it
"""
import csv
import importlib
import os
import sys
import tempfile
import types

import numpy as np

K = 9


def load_reference(ref):
    sys.modules["cv2"] = types.ModuleType("cv2")                       # empty: only main() touches cv2
    sys.path.insert(0, os.path.join(ref, "CVC-YOLOv3"))
    return importlib.import_module("generate_kmeans_dataset_csvs")


def run_reference_loop(mod, points, init):
    """the loop of main lines 139-149 around the reference's own functions, from given initial boxes"""
    import pandas as pd
    boxes = pd.DataFrame({'h': points[:, 0].tolist(), 'w': points[:, 1].tolist()})
    centroids = {i: [boxes['h'][j], boxes['w'][j]] for i, j in enumerate(init)}
    boxes = mod.assignment(boxes, centroids)
    it = 0
    while True:
        it += 1
        before = boxes['closest'].copy(deep=True)
        centroids = mod.update(boxes, centroids)
        boxes = mod.assignment(boxes, centroids)
        if before.equals(boxes['closest']):
            break
    cent = np.array([[centroids[i][0], centroids[i][1]] for i in range(len(init))], np.float64)
    return cent, boxes['closest'].to_numpy().astype(np.uint8), it


def raw_boxes(rng, n):
    h = rng.integers(8, 200, n)
    w = np.maximum(3, (h * rng.uniform(0.45, 0.95, n)).astype(np.int64) + rng.integers(-2, 3, n))
    return h, w


def scaled_points(h, w, ratio_of):
    order = sorted(zip(h.tolist(), w.tolist()), key=lambda x: x[0])
    max_h, _ = order[int(.95 * len(order)) - 1]
    min_h, min_w = order[int(0.05 * len(order))]
    ratio = ratio_of(max_h, min_h)
    return np.array([[(a - min_h) * ratio + 10, (b - min_w) * ratio + 10] for a, b in zip(h.tolist(), w.tolist())], np.float64)


def kmeans_fixtures(mod, out):
    rng = np.random.default_rng(20240611)
    sets = {"dyadic": scaled_points(*raw_boxes(rng, 397), lambda a, b: 0.25),
            "generic": scaled_points(*raw_boxes(rng, 389), lambda a, b: 73 / (a - b))}
    for name, pts in sets.items():
        seeds = [0, 1, 2, 3]
        init, cents, assigns, its = [], [], [], []
        for seed in seeds:
            np.random.seed(seed)
            idx = [int(np.random.randint(0, len(pts))) for _ in range(K)]
            c, a, it = run_reference_loop(mod, pts, idx)
            init.append(idx), cents.append(c), assigns.append(a), its.append(it)
            print(name, "seed", seed, "iterations", it, "nan", bool(np.isnan(c).any()))
        out[f"{name}::points"] = pts
        out[f"{name}::seeds"] = np.array(seeds)
        out[f"{name}::init"] = np.array(init)
        out[f"{name}::centroids"] = np.array(cents)
        out[f"{name}::assign"] = np.array(assigns)
        out[f"{name}::iterations"] = np.array(its)
    pts = sets["dyadic"]
    idx = [5, 120, 5, 301]                                             # box 5 twice: cluster 2 can never win and stays empty
    c, a, it = run_reference_loop(mod, pts, idx)
    print("repeat: iterations", it, "nan rows", np.isnan(c).any(axis=1).tolist())
    out["repeat::init"] = np.array([idx])
    out["repeat::centroids"] = c[None]
    out["repeat::assign"] = a[None]
    out["repeat::iterations"] = np.array([it])


def main_fixture(mod, out):
    from PIL import Image
    rng = np.random.default_rng(7)
    n = 230
    sizes = [(64, 48), (40, 56)]                                       # (W, H)
    which = rng.integers(0, 2, n)
    h = rng.integers(10, 22, n)                                        # twelve heights over 230 boxes: ties everywhere
    w = rng.integers(4, 30, n)
    names = [f"img_{i:03d}.png" for i in range(n)]
    mod.cv2.imread = lambda p: np.array(Image.open(p).convert("RGB"))
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "images")
        outp = os.path.join(tmp, "out")
        os.makedirs(data), os.makedirs(outp)
        for i, nm in enumerate(names):
            Image.new("RGB", sizes[which[i]]).save(os.path.join(data, nm))
        src = os.path.join(tmp, "in.csv")
        with open(src, "w") as f:
            f.write("first line\nsecond line\n")
            for i, nm in enumerate(names):
                f.write(f"{nm},http://x/{nm},{h[i]},{w[i]}\n")
        cwd, tdir = os.getcwd(), tempfile.tempdir
        os.chdir(tmp)
        tempfile.tempdir = outp                                        # main renames its temporary files into output_path
        real_ntf = tempfile.NamedTemporaryFile
        tempfile.NamedTemporaryFile = lambda *a, **k: real_ntf(*a, delete=False, **k)    # (the renamed file is gone at close)
        try:
            np.random.seed(0)
            mod.main(src, data, outp, K, 83, 10, False, [75, 15, 0])
        finally:
            os.chdir(cwd)
            tempfile.tempdir, tempfile.NamedTemporaryFile = tdir, real_ntf
        files = {}
        for fn in ("train.csv", "test.csv", "validate.csv", "train-validate.csv", "all.csv"):
            with open(os.path.join(outp, fn)) as f:
                files[fn] = list(csv.reader(f))
        with open(os.path.join(tmp, "anchors.txt")) as f:             # written to the working directory: '%0.2f,%0.2f' per cluster
            out["main::anchors_txt"] = np.array([[float(v) for v in line.split(",")] for line in f if line.strip()], np.float64)
    out["main::names"] = np.array(names)
    out["main::sizes"] = np.array([sizes[k] for k in which])
    out["main::hw"] = np.stack([h, w], 1)
    rows = files["all.csv"][2:]
    assert [r[0] for r in rows] == names
    out["main::scale"] = np.array([float(r[4]) for r in rows], np.float64)
    out["main::wh_cols"] = np.array([[int(r[2]), int(r[3])] for r in rows])
    for fn, rws in files.items():
        out[f"main::{fn}"] = np.array([r[0] for r in rws[2:]], dtype="U16")
        print(fn, len(rws) - 2, "rows")
    out["main::head_note"] = np.array(files["validate.csv"][0])
    out["main::second_row"] = np.array(files["validate.csv"][1])


if __name__ == "__main__":
    mod = load_reference(sys.argv[1])
    out = {}
    kmeans_fixtures(mod, out)
    main_fixture(mod, out)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "anchors.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
