"""-m gpu: csrc/anchors.hip (mdcv_kmeans_*) through the C ABI and through mdcv.data.kmeans_anchors against the NumPy + math.fsum
restatement that tests/test_anchors_host.py pins to the reference (tests/helpers/anchor_refs.py): `==` on the bit patterns of every
centroid, on every assignment, iteration count, distortion (Python integers) and NaN flag; guard bands around every buffer the kernels
write; every refusal without a launch.  Then prepare_dataset end to end into the loader and the network."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import anchor_refs as ar  # noqa: E402

from mdcv import _lib  # noqa: E402
from mdcv.data import kmeans_anchors, prep  # noqa: E402

SENT = 0x5A5A5A5A5A5A5A5A
HEAD = 4


class Guarded:
    """`nbytes` (rounded up to 8) between two sentinel-filled guard bands of 32 eight-byte words"""

    def __init__(self, nbytes, guard=32):
        self.n, self.g = (int(nbytes) + 7) // 8, guard
        self.raw = torch.full((self.n + 2 * guard,), SENT, dtype=torch.int64, device="cuda")
        self.ptr = self.raw.data_ptr() + 8 * guard

    def words(self):
        return self.raw[self.g:self.g + self.n]

    def guards_intact(self):
        return bool((self.raw[:self.g] == SENT).all()) and bool((self.raw[self.g + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.raw == SENT).all())


def run_abi(points, init, chunk=8, max_steps=400, one_chunk=False):
    """the C ABI on guarded buffers, on the current stream -> dict of per-restart results (as anchor_refs.lloyd names them)"""
    L = _lib.lib()
    pts = np.ascontiguousarray(points, np.float64)
    init = np.ascontiguousarray(init, np.int32)
    R, K = init.shape
    N = len(pts)
    d_pts, d_init = torch.from_numpy(pts).cuda(), torch.from_numpy(init).cuda()
    ws, asg, rec = Guarded(L.kmeans_workspace_bytes(N, K, R)), Guarded(R * N), Guarded(8 * R * (HEAD + 2 * K))
    st = torch.cuda.current_stream().cuda_stream
    assert L.kmeans_begin(ws.ptr, d_pts.data_ptr(), d_init.data_ptr(), N, K, R, st) == 0
    done = 0
    while True:
        n = chunk + (1 if done == 0 and not one_chunk else 0)
        assert L.kmeans_steps(ws.ptr, d_pts.data_ptr(), asg.ptr, rec.ptr, N, K, R, done, n, st) == 0
        done += n
        r = rec.words().cpu().numpy().reshape(R, HEAD + 2 * K)
        if one_chunk or (r[:, 0] >= 0).all():
            break
        assert done < max_steps, "no fixed point"
    assert ws.guards_intact() and asg.guards_intact() and rec.guards_intact()
    a = asg.words().cpu().numpy().view(np.uint8)[:R * N].reshape(R, N)
    return dict(iterations=r[:, 0].tolist(), distortion=[(int(x[2]) << 32) + int(x[1]) for x in r], nan=[bool(x[3]) for x in r],
                centroids=r[:, HEAD:].copy().view(np.float64).reshape(R, K, 2), assign=a, steps=done)


def same_centroids(got, want):
    """bit patterns, NaN against NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def check_against_helper(points, init, got):
    for r, idx in enumerate(init):
        want = ar.lloyd(points, idx)
        assert got["iterations"][r] == want["iterations"], r
        assert np.array_equal(got["assign"][r], want["assign"]), r
        assert same_centroids(got["centroids"][r], want["centroids"]), r
        assert got["distortion"][r] == want["distortion"], r
        assert got["nan"][r] == want["nan"], r


def boxes(n, seed):
    """scaled boxes as prepare_dataset makes them: fl(fl(k * ratio) + 10) with integer k of both signs -> negative coordinates too"""
    rng = np.random.default_rng(seed)
    h = rng.integers(8, 200, n)
    w = np.maximum(3, (h * rng.uniform(0.45, 0.95, n)).astype(np.int64))
    ratio = 73 / 97
    return np.array([[(a - 60) * ratio + 10, (b - 70) * ratio + 10] for a, b in zip(h.tolist(), w.tolist())], np.float64)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", [1, 9, 16])
@pytest.mark.parametrize("N", [1, "K", 255, 257, 5000])
def test_kernel_against_restatement(N, K, R):
    N = K if N == "K" else N
    pts = boxes(N, 100 * N + K)
    assert (pts < 0).any() or N < 255
    init = prep.initial_indices(N, K, seed=N + K, restarts=R)           # N < K: repeated boxes, empty clusters, NaN centroids
    check_against_helper(pts, init, run_abi(pts, init))


def test_exact_ties_between_two_centroids():
    """a 5 x 5 integer grid between two initial centroids at equal distance from its middle column: the first minimum wins, every step"""
    pts = np.array([[float(i), float(j)] for i in range(5) for j in range(5)] + [[-3.0, -2.0]])
    init = np.array([[10, 14], [14, 10], [2, 22]], np.int32)           # (2,0) / (2,4): column 2 ties; swapped; (0,2) / (4,2): row 2 ties
    got = run_abi(pts, init, one_chunk=True, chunk=1)
    a0, _ = ar.assign(pts, pts[init[0]])
    assert a0[12] == 0 and got["assign"][0].tolist() == a0.tolist() and got["assign"][1][12] == 0
    check_against_helper(pts, init, run_abi(pts, init))


def test_equal_roots_keep_the_lower_index():
    pts, init = ar.equal_root_case()
    got = run_abi(pts, np.array([init], np.int32), one_chunk=True, chunk=1)         # step 0 alone
    assert got["assign"][0].tolist() == [0, 1, 0]
    q = (pts[2, 0] - pts[0, 0]) ** 2 + (pts[2, 1] - pts[0, 1]) ** 2
    assert got["distortion"][0] == int(q * 2.0 ** 32) and got["iterations"] == [-1]
    check_against_helper(pts, [init], run_abi(pts, np.array([init], np.int32)))


def test_repeated_index_nan_cluster(golden_dir):
    z = np.load(os.path.join(golden_dir, "anchors.npz"))
    pts, init = z["dyadic::points"], z["repeat::init"]
    got = run_abi(pts, init)
    assert got["nan"] == [True] and np.isnan(got["centroids"][0]).any(axis=1).tolist() == [False, False, True, False]
    check_against_helper(pts, init, got)
    alive = [0, 1, 3]
    assert same_centroids(got["centroids"][0][alive], z["repeat::centroids"][0][alive])     # the reference's own numbers (exact sums)
    assert got["iterations"] == z["repeat::iterations"].tolist()
    with pytest.raises(ValueError, match="empty cluster"):
        kmeans_anchors(pts, 4, init=init)
    km = kmeans_anchors(pts, 4, init=[[5, 120, 5, 301], [5, 120, 200, 301]])
    assert km.nan == [True, False] and km.best == 1


def test_reference_numbers_on_the_dyadic_set(golden_dir):
    z = np.load(os.path.join(golden_dir, "anchors.npz"))
    km = kmeans_anchors(z["dyadic::points"], 9, init=z["dyadic::init"])
    assert same_centroids(km.all_centroids, z["dyadic::centroids"]) and km.all_iterations.tolist() == z["dyadic::iterations"].tolist()
    one = kmeans_anchors(z["dyadic::points"], 9, seed=int(z["dyadic::seeds"][1]))
    assert same_centroids(one.centroids, z["dyadic::centroids"][1]) and np.array_equal(one.assignment, z["dyadic::assign"][1])


def same_result(a, b):
    return (same_centroids(a.all_centroids, b.all_centroids) and np.array_equal(a.assignment, b.assignment) and a.distortions == b.distortions
            and a.all_iterations.tolist() == b.all_iterations.tolist() and a.nan == b.nan and a.best == b.best and a.iterations == b.iterations)


def test_wrapper_chunks_runs_streams_and_selection():
    pts = boxes(5000, 5)
    a = kmeans_anchors(pts, 9, seed=3, restarts=3, check_every=8)
    assert same_result(a, kmeans_anchors(pts, 9, seed=3, restarts=3, check_every=1))          # converged_at is the device's, not the chunk's
    assert same_result(a, kmeans_anchors(pts, 9, seed=3, restarts=3, check_every=8))          # two runs
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = kmeans_anchors(pts, 9, seed=3, restarts=3)
    s.synchronize()
    assert same_result(a, b)
    init = prep.initial_indices(len(pts), 9, 3, 3)
    want = [ar.lloyd(pts, i) for i in init]
    assert a.distortions == [w["distortion"] for w in want] and a.all_iterations.tolist() == [w["iterations"] for w in want]
    assert a.best == ar.select_best(a.distortions, a.nan) and a.iterations == want[a.best]["iterations"]
    assert same_centroids(a.centroids, want[a.best]["centroids"]) and np.array_equal(a.assignment, want[a.best]["assign"])
    assert a.centroids.shape == (9, 2) and a.assignment.shape == (5000,) and a.assignment.dtype == np.uint8
    assert min(w["iterations"] for w in want) > 2
    with pytest.raises(RuntimeError, match="fixed point"):
        kmeans_anchors(pts, 9, seed=3, restarts=3, max_iter=2)
    with pytest.raises(RuntimeError, match="fixed point"):
        kmeans_anchors(pts, 9, seed=3, restarts=3, max_iter=2, check_every=1)
    it = max(w["iterations"] for w in want)
    assert same_result(a, kmeans_anchors(pts, 9, seed=3, restarts=3, max_iter=it, check_every=5))     # exactly enough


def test_refusals_launch_nothing():
    L = _lib.lib()
    pts = torch.ones(10, 2, dtype=torch.float64, device="cuda")
    init = torch.zeros(64 * 16, dtype=torch.int32, device="cuda")
    ws, asg, rec = Guarded(1 << 16), Guarded(64 * 10), Guarded(8 * 64 * 40)
    st = torch.cuda.current_stream().cuda_stream
    for N, K, R in ((0, 2, 1), (1 << 24, 2, 1), (10, 0, 1), (10, 17, 1), (10, 2, 0), (10, 2, 65), (-1, 2, 1)):
        assert L.kmeans_workspace_bytes(N, K, R) == -1
        assert L.kmeans_begin(ws.ptr, pts.data_ptr(), init.data_ptr(), N, K, R, st) == -1
        assert L.kmeans_steps(ws.ptr, pts.data_ptr(), asg.ptr, rec.ptr, N, K, R, 0, 1, st) == -1
    assert L.kmeans_begin(None, pts.data_ptr(), init.data_ptr(), 10, 2, 1, st) == -1
    assert L.kmeans_begin(ws.ptr, None, init.data_ptr(), 10, 2, 1, st) == -1
    assert L.kmeans_begin(ws.ptr, pts.data_ptr(), None, 10, 2, 1, st) == -1
    for args in ((None, pts.data_ptr(), asg.ptr, rec.ptr, 10, 2, 1, 0, 1), (ws.ptr, None, asg.ptr, rec.ptr, 10, 2, 1, 0, 1),
                 (ws.ptr, pts.data_ptr(), None, rec.ptr, 10, 2, 1, 0, 1), (ws.ptr, pts.data_ptr(), asg.ptr, None, 10, 2, 1, 0, 1),
                 (ws.ptr, pts.data_ptr(), asg.ptr, rec.ptr, 10, 2, 1, -1, 1), (ws.ptr, pts.data_ptr(), asg.ptr, rec.ptr, 10, 2, 1, 0, 0),
                 (ws.ptr, pts.data_ptr(), asg.ptr, rec.ptr, 10, 2, 1, 2 ** 31 - 1, 1)):
        assert L.kmeans_steps(*args, st) == -1
    torch.cuda.synchronize()
    assert ws.untouched() and asg.untouched() and rec.untouched()
    assert L.kmeans_workspace_bytes(200000, 9, 64) == 8 * (64 * 9 * 2 + 3 * 64 * (9 * 7 + 3) + 64)


def test_prepare_dataset_end_to_end(tmp_path, golden_dir):
    """a handful of PNGs of two sizes -> the five files byte-equal to the host restatement; the loader builds a batch from train.csv and
    the network reports the written anchors"""
    from anchor_cases import host_kmeans, write_raw_dataset
    from mdcv.data import ImageLabelBatches, prepare_dataset
    from mdcv.yolo.models import Darknet
    src, images = write_raw_dataset(str(tmp_path))
    out, out_host = str(tmp_path / "dataset"), str(tmp_path / "host")
    km = prepare_dataset(src, images, out, num_clst=6, restarts=4, seed=1)
    real = prep.kmeans_anchors
    prep.kmeans_anchors = host_kmeans
    try:
        prepare_dataset(src, images, out_host, num_clst=6, restarts=4, seed=1)
    finally:
        prep.kmeans_anchors = real
    for fn in prep.FILES + ("anchors.txt",):
        with open(os.path.join(out, fn), "rb") as a, open(os.path.join(out_host, fn), "rb") as b:
            assert a.read() == b.read(), fn
    loader = ImageLabelBatches(os.path.join(out, "train.csv"), images, 64, 64, batch_size=4, shuffle=False, ts=False)
    uris, imgs, targets = next(iter(loader))
    assert imgs.shape == (4, 3, 64, 64) and targets.shape[0] == 4 and targets.shape[2] == 5 and bool(torch.isfinite(imgs).all())
    assert int((targets[:, :, 3] > 0).sum()) == 2 + 2 + 2 + 0
    with open(os.path.join(golden_dir, "mini", "mini.cfg")) as f:
        cfg = f.read().replace("train_uri=dataset/train.csv", "train_uri=" + os.path.join(out, "train.csv"))
    assert os.path.join(out, "train.csv") in cfg
    with open(tmp_path / "mini.cfg", "w") as f:
        f.write(cfg)
    net = Darknet(str(tmp_path / "mini.cfg"), 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    order = sorted(range(6), key=lambda k: km.centroids[k, 0] * km.centroids[k, 1])
    assert net.get_anchors() == [[float(km.centroids[k, 1]), float(km.centroids[k, 0])] for k in order]
