"""The anchor k-means of csrc/anchors.hip restated with NumPy and math.fsum, one rounding at a time (the contract in include/mdcv_hip.h).

    assignment   for k in index order: q = fl(fl(dh*dh) + fl(dw*dw)), d = sqrt(q) (NumPy's is correctly rounded); the first minimum wins,
                 a NaN centroid never wins
    update       c[k] = fl(fsum(members) / n_k) per coordinate; NaN for an empty cluster
    distortion   sum_i floor(q_i * 2^32) as a Python integer, q_i to the box's own centroid at the fixed point

`lloyd` runs the loop of generate_kmeans_dataset_csvs.py:139-149: assign to the initial boxes, then update + assign until the assignment
repeats; `iterations` counts the update + assign passes, the last one included."""
import math

import numpy as np


def assign(points, cent):
    """-> (index uint8 [N], q of the winner float64 [N])"""
    points = np.asarray(points, np.float64)
    n = len(points)
    best = np.full(n, np.inf)
    bq = np.zeros(n)
    bi = np.zeros(n, np.uint8)
    with np.errstate(invalid="ignore"):
        for k in range(len(cent)):
            dh = points[:, 0] - cent[k][0]
            dw = points[:, 1] - cent[k][1]
            q = dh * dh + dw * dw
            d = np.sqrt(q)
            win = d < best                    # strict: the first minimum stays; NaN compares false
            best[win], bq[win], bi[win] = d[win], q[win], k
    return bi, bq


def update(points, idx, K):
    points = np.asarray(points, np.float64)
    cent = np.full((K, 2), np.nan)
    for k in range(K):
        m = points[idx == k]
        if len(m):
            cent[k, 0] = math.fsum(m[:, 0].tolist()) / len(m)
            cent[k, 1] = math.fsum(m[:, 1].tolist()) / len(m)
    return cent


def distortion(q):
    return sum(int(math.floor(v * 4294967296.0)) for v in q.tolist())


def lloyd(points, init_idx, max_iter=10000):
    """-> dict(centroids [K,2], assign uint8 [N], iterations, distortion, nan)"""
    points = np.asarray(points, np.float64)
    K = len(init_idx)
    cent = points[np.asarray(init_idx, np.int64)].copy()
    idx, _ = assign(points, cent)
    it = 0
    while True:
        it += 1
        if it > max_iter:
            raise RuntimeError("no fixed point")
        cent = update(points, idx, K)
        new, q = assign(points, cent)
        same = np.array_equal(new, idx)
        idx = new
        if same:
            break
    return dict(centroids=cent, assign=idx, iterations=it, distortion=distortion(q), nan=bool(np.isnan(cent).any()))


def select_best(distortions, nans):
    """the smallest distortion among restarts without a NaN centroid; ties go to the lowest index; None when every restart has one"""
    best = None
    for r, (d, bad) in enumerate(zip(distortions, nans)):
        if not bad and (best is None or d < distortions[best]):
            best = r
    return best


def pairwise_mean_bound(x):
    """|mean by pairwise fp64 summation - fl(exact sum / n)| <= (ceil(log2 n) + 1) * 2^-53 * sum|x| / n for the summation (that many roundings
    of relative size 2^-53 on partial sums bounded by sum|x|), plus one rounding of the quotient, 2^-53 * |mean|"""
    x = np.asarray(x, np.float64)
    n = len(x)
    u = 2.0 ** -53
    s = math.fsum(np.abs(x).tolist())
    depth = math.ceil(math.log2(n)) + 1 if n > 1 else 1
    return depth * u * s / n + u * abs(math.fsum(x.tolist()) / n)


def draws(seed, N, count):
    """the boxes np.random.seed(seed) + `count` calls of np.random.randint(0, N) pick"""
    rs = np.random.RandomState(seed)
    return [int(rs.randint(0, N)) for _ in range(count)]


def equal_root_case():
    """-> (points [3,2], init [2]): box 2 = (0, 0) is at q = 1 + 2^-52 from box 0 = (1, 2^-26) and at q = 1 from box 1 = (-1, 0).  The two q
    differ and both roots round to 1.0, so the initial assignment sends box 2 to cluster 0, the lower index, although its q is the larger:
    a comparison of squared distances would pick cluster 1."""
    pts = np.array([[1.0, 2.0 ** -26], [-1.0, 0.0], [0.0, 0.0]])
    q0 = pts[0, 0] * pts[0, 0] + pts[0, 1] * pts[0, 1]
    assert q0 == 1.0 + 2.0 ** -52 and math.sqrt(q0) == 1.0
    return pts, [0, 1]
