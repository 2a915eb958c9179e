"""Cone key points on whole frames and on crop files, drawn on the device: the three kernels of csrc/kpt_detect.hip through the C ABI against
tests/helpers/kpt_draw_numpy.py (byte for byte), then mdcv.yolo.detect.FrameConeDetector and mdcv.rektnet.detect end to end, each stage held
to its restatement given the previous stage's device output."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detect_cases as C  # noqa: E402
import detect_draw_numpy as D  # noqa: E402
import kpt_draw_numpy as KD  # noqa: E402
import kptload_numpy as KN  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
F = np.float32
GUARD = 0x5A
SIZES = [(37, 29), (64, 48)]                     # (W, H)
ONE = int(np.array([1.0]).view(np.int64)[0])
EARG = -1


def _lib():
    from mdcv import _lib as m
    return m.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pool(sizes, seed, first=5, gap=7):
    """random frames at UNALIGNED pool offsets with guard bytes in front of, between and behind them -> (frames, pool, desc)"""
    frames = [C.random_frame(w, h, seed + i) for i, (w, h) in enumerate(sizes)]
    offs, at = [], first
    for f in frames:
        offs.append(at)
        at += f.size + gap
    pool = np.full(at, GUARD, np.uint8)
    for f, o in zip(frames, offs):
        pool[o:o + f.size] = f.reshape(-1)
    desc = np.array([[o, f.shape[1], f.shape[0], ONE, 0, 0] for f, o in zip(frames, offs)], np.int64)
    assert any(o % 4 for o in offs)
    return frames, pool, desc


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------ kernel b: the discs
def _at(x, y, W, H):
    """a normalised point that lands on pixel (x, y) of a whole-image window: (x + 0.5) / W truncates to x, also for x = -1 (-0.5 -> 0
    would not: so outside points aim at the pixel's far side)"""
    fx = (x + 0.5) / W if x >= 0 else (x - 0.5) / W
    fy = (y + 0.5) / H if y >= 0 else (y - 0.5) / H
    return [fx, fy]


def _draw_points(desc, pool, pts, window, owner, colours=KD.COLOURS_RGB):
    L = _lib()
    n, M = len(desc), len(pts)
    d_desc, d_pool = _dev(desc), _dev(pool)
    d_pts, d_win, d_own = _dev(np.asarray(pts, F)), _dev(np.asarray(window, np.int32)), _dev(np.asarray(owner, np.int32))
    centers = torch.full((max(M, 1), 7, 2), -7, dtype=torch.int32, device="cuda")
    skipped = torch.full((n,), 12345, dtype=torch.int32, device="cuda")
    col = np.ascontiguousarray(colours, np.uint8)
    rc = L.kpt_draw_points(desc.ctypes.data, d_desc.data_ptr(), n, d_pool.data_ptr(), d_pool.numel(), d_pts.data_ptr(), d_win.data_ptr(),
                           d_own.data_ptr(), M, col.ctypes.data, centers.data_ptr(), skipped.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, d_pool.cpu().numpy(), centers.cpu().numpy()[:M], skipped.cpu().numpy()


def test_draw_points_parity():
    frames, pool, desc = _pool(SIZES, 70)
    pts, window, owner = [], [], []

    def cone(img, points, win=None):
        W, H = SIZES[img]
        win = win or (0, 0, W, H)
        assert len(points) == 7
        pts.append(points), window.append(win), owner.append((img, len(owner)))

    for img, (W, H) in enumerate(SIZES):
        # corners and one pixel outside each edge
        cone(img, [_at(0, 0, W, H), _at(W - 1, H - 1, W, H), _at(-1, H // 2, W, H), _at(W, H // 2, W, H), _at(W // 2, -1, W, H),
                   _at(W // 2, H, W, H), _at(W - 1, 0, W, H)])
        # two pixels outside (one disc pixel left inside), fully outside on each side, and far away
        cone(img, [_at(-2, 5, W, H), _at(W + 1, 5, W, H), _at(-3, 9, W, H), _at(W + 2, 9, W, H), _at(9, -3, W, H), _at(9, H + 2, W, H),
                   [-40.0, 55.0]])
    W, H = SIZES[0]
    a = [_at(10 + i, 12 + (i % 2), W, H) for i in range(7)]                     # a chain of intersecting discs inside one cone
    b = [_at(11 + i, 13 - (i % 2), W, H) for i in range(7)]                     # and a second cone across it
    cone(0, a), cone(0, b)
    W, H = SIZES[1]
    a = [_at(20 + i, 30 + (i % 2), W, H) for i in range(7)]
    b = [_at(21 + i, 31 - (i % 2), W, H) for i in range(7)]
    cone(1, b), cone(1, a)                                                      # the same crossing in the other order
    sub = (40, 20, 17, 11)                                                      # a window inside the image: points beyond it still drawn
    cone(1, [[0.0, 0.0], [0.999, 0.999], [1.2, 0.5], [-0.2, 0.5], [float("nan"), 0.5], [0.5, float("inf")], [0.5, 0.5]], sub)
    order = np.argsort([o[0] for o in owner], kind="stable")                    # image-major, cone order kept
    pts, window = np.array(pts, F)[order], np.array(window, np.int32)[order]
    owner = np.array(owner, np.int32)[order]
    rc, got, centers, skipped = _draw_points(desc, pool, pts, window, owner)
    assert rc == 0
    want, want_centers, want_skipped = KD.draw_points(pool, desc, pts, window, owner)
    assert np.array_equal(centers, want_centers)
    assert np.array_equal(skipped, want_skipped) and list(skipped) == [0, 2]
    assert np.array_equal(got, want)                                            # frames AND the guard bytes around them
    assert (got != pool).sum() > 300
    m0 = int(np.nonzero(owner[:, 0] == 0)[0][0])
    assert tuple(centers[m0, 0]) == (0, 0) and tuple(centers[m0, 1]) == (36, 28) and tuple(centers[m0, 2]) == (-1, 14)
    # M == 0: the counters are zeroed, nothing else is touched
    rc, got, _, skipped = _draw_points(desc, pool, np.zeros((0, 7, 2), F), np.zeros((0, 4), np.int32), np.zeros((0, 2), np.int32))
    assert rc == 0 and np.array_equal(got, pool) and not skipped.any()


def test_draw_points_many_cones_of_one_image():
    """more later cones than one LDS refill holds (36): 80 cones of random points crowded into one 64 x 48 image, behind 3 of another"""
    frames, pool, desc = _pool(SIZES, 90)
    rng = np.random.default_rng(5)
    M = 83
    owner = np.array([[0, m] if m < 3 else [1, m] for m in range(M)], np.int32)
    window = np.array([[0, 0, 37, 29] if m < 3 else [rng.integers(0, 30), rng.integers(0, 20), 30, 25] for m in range(M)], np.int32)
    pts = rng.uniform(-0.1, 1.1, (M, 7, 2)).astype(F)
    rc, got, centers, skipped = _draw_points(desc, pool, pts, window, owner)
    want, want_centers, want_skipped = KD.draw_points(pool, desc, pts, window, owner)
    assert rc == 0 and np.array_equal(centers, want_centers) and np.array_equal(skipped, want_skipped)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ kernel a: the crops
def _crop_case():
    sizes = [SIZES[0], (12, 10), SIZES[1]]                                      # the frame in the middle keeps nothing
    frames, pool, desc = _pool(sizes, 30)
    K = 8
    rects = np.zeros((3, K, 4), np.int32)
    W, H = sizes[0]
    rects[0] = [[3, 4, 20, 25], [7, 9, 7, 9], [-5, 3, 10, 12], [30, 3, W + 4, 12], [3, -6, 12, 8], [0, 0, -1, -1], [3, 20, 12, H + 9],
                [-2, -2, W + 1, H + 1]]
    W, H = sizes[2]
    rects[2] = [[0, 0, W - 1, H - 1], [W - 1, H - 1, W - 1, H - 1], [0, 0, -1, -1], [W, 3, W + 5, 9], [10, 11, 50, 40], [-9, 3, -1, 9],
                [60, 40, 70, 50], [1, 1, 2, 2]]
    rects[1] = [[1, 1, 5, 5]] * K                                               # good rects, not counted
    count = np.array([8, 0, 7], np.int32)
    return frames, pool, desc, rects, count, K


def _crop(desc, pool, rects, count, K, per, S, fill=-3.0, desc_dev=None):
    L = _lib()
    B = len(desc)
    cap = B * min(K, per) if B and K > 0 and per > 0 else 1
    d_desc, d_pool, d_rects, d_count = _dev(desc if desc_dev is None else desc_dev), _dev(pool), _dev(rects), _dev(count)
    crops = torch.full((cap, 3, S, S), fill, dtype=torch.float32, device="cuda")
    owner = torch.full((cap, 2), -7, dtype=torch.int32, device="cuda")
    window = torch.full((cap, 4), -7, dtype=torch.int32, device="cuda")
    total = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = L.crop_resize_frames_u8(desc.ctypes.data, d_desc.data_ptr(), B, d_pool.data_ptr(), d_pool.numel(), d_rects.data_ptr(),
                                 d_count.data_ptr(), K, per, S, crops.data_ptr(), owner.data_ptr(), window.data_ptr(), total.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_pool.cpu().numpy(), pool)                           # read only
    return rc, crops.cpu().numpy(), owner.cpu().numpy(), window.cpu().numpy(), int(total.cpu()[0])


@pytest.mark.parametrize("S", [16, 80])
def test_crop_resize_frames_parity(S):
    frames, pool, desc, rects, count, K = _crop_case()
    for per in (K, 5):
        want, want_owner, want_window, M = KD.crop_frames(frames, rects, count, per, S)
        rc, crops, owner, window, total = _crop(desc, pool, rects, count, K, per, S)
        assert rc == 0 and total == M and M == (11 if per == K else 8)
        assert np.array_equal(owner[:M], want_owner) and np.array_equal(window[:M], want_window)
        assert np.array_equal(crops[:M].view(np.int32), want.view(np.int32))    # the floats as bits
        assert (crops[M:] == -3.0).all() and (owner[M:] == -7).all() and (window[M:] == -7).all()      # rows past total: not written
    assert not (want_owner[:, 0] == 1).any()


def test_crop_resize_frames_unvectorised_and_bad_device_descriptor():
    """S % 4 != 0 takes the scalar store path; a device descriptor that differs from the validated host copy and points outside the pool
    gives that frame no crop instead of a read outside"""
    frames, pool, desc, rects, count, K = _crop_case()
    want, want_owner, want_window, M = KD.crop_frames(frames, rects, count, K, 18)
    rc, crops, owner, window, total = _crop(desc, pool, rects, count, K, K, 18)
    assert rc == 0 and total == M and np.array_equal(owner[:M], want_owner)
    assert np.array_equal(crops[:M].view(np.int32), want.view(np.int32))
    bad = desc.copy()
    bad[0, 0] = len(pool) - 10                                                  # frame 0 would run past the end of the pool
    keep = want_owner[:, 0] != 0
    rc, crops, owner, window, total = _crop(desc, pool, rects, count, K, K, 18, desc_dev=bad)
    assert rc == 0 and total == int(keep.sum()) and np.array_equal(owner[:total], want_owner[keep])
    assert np.array_equal(crops[:total].view(np.int32), want[keep].view(np.int32)) and (crops[total:] == -3.0).all()


# ----------------------------------------------------------------------------------------------------------- kernel c: the mosaic
def _mosaic(hm, S):
    L = _lib()
    B = len(hm)
    d_hm = _dev(hm)
    out = torch.full((max(B, 1), 7 * S, S), 0xA5, dtype=torch.uint8, device="cuda")
    rc = L.kpt_heatmap_mosaic(d_hm.data_ptr(), B, S, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:B]


def test_heatmap_mosaic_parity():
    rng = np.random.default_rng(21)
    B, S = 3, 16
    hm = rng.standard_normal((B, 7, S, S)).astype(F)
    hm[0, 1] = np.abs(hm[0, 1]) * F(1e-7)                                       # softmax-sized values
    hm[1, 4] = F(0.375)                                                         # a constant map
    tie = np.linspace(0, 1, S * S, dtype=F).reshape(S, S)                       # min 0, max 1: v == x
    tie[1, 1], tie[1, 2], tie[2, 2] = F(0.5), F(0.1171875), F(0.12109375)       # * 255 = 127.5 -> 128; 29.8828125; 30.87890625
    tie[3, 3], tie[3, 4] = F(0.00390625) * F(2), F(0.0234375)                   # 1.9921875; 5.9765625
    hm[2, 6] = tie
    hm[2, 0, 5, 5] = np.nan                                                     # a NaN poisons its own map only
    rc, got = _mosaic(hm, S)
    want = KD.mosaic(hm)
    assert rc == 0 and np.array_equal(got, want)
    assert got[2, 6 * S + 1, 1] == 128 and float(tie[1, 1]) * 255 == 127.5
    assert not got[1, 4 * S:5 * S].any() and not got[2, :S].any() and got[2, S:].any()
    hm2 = rng.uniform(0, 1, (1, 7, 80, 80)).astype(F)                           # more elements than lanes: the strided reduction
    rc, got = _mosaic(hm2, 80)
    assert rc == 0 and np.array_equal(got, KD.mosaic(hm2))


# -------------------------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_write_nothing():
    L = _lib()
    frames, pool, desc, rects, count, K = _crop_case()
    outside = desc.copy()
    outside[2, 0] = len(pool) - 100                                             # a frame outside the pool
    for d, S in ((outside, 16), (desc, 15), (desc, 257)):
        rc, crops, owner, window, total = _crop_raw(d, pool, rects, count, K, S)
        assert rc == EARG and (crops == -3.0).all() and (owner == -7).all() and (window == -7).all() and total == -7
    d_desc, d_pool, d_rects, d_count = _dev(desc), _dev(pool), _dev(rects), _dev(count)
    crops = torch.full((24, 3, 16, 16), -3.0, device="cuda")
    tab = torch.full((24, 8), -7, dtype=torch.int32, device="cuda")
    good = [desc.ctypes.data, d_desc.data_ptr(), 3, d_pool.data_ptr(), d_pool.numel(), d_rects.data_ptr(), d_count.data_ptr(), K, K, 16,
            crops.data_ptr(), tab.data_ptr(), tab.data_ptr() + 24 * 8, tab.data_ptr() + 24 * 24, _stream()]
    for i in (0, 1, 3, 5, 6, 10, 11, 12, 13):                                   # each pointer in turn
        args = list(good)
        args[i] = None
        assert L.crop_resize_frames_u8(*args) == EARG
    torch.cuda.synchronize()
    assert (crops == -3.0).all() and (tab == -7).all()
    # the draw: a frame outside the pool, null pointers
    pts, win, own = np.full((2, 7, 2), 0.5, F), np.array([[0, 0, 37, 29]] * 2, np.int32), np.array([[0, 0], [0, 1]], np.int32)
    rc, got, centers, skipped = _draw_points(outside[[0, 2]], pool, pts, win, own)
    assert rc == EARG and np.array_equal(got, pool) and (centers == -7).all() and (skipped == 12345).all()
    d_pts, d_win, d_own = _dev(pts), _dev(win), _dev(own)
    cen = torch.full((2, 7, 2), -7, dtype=torch.int32, device="cuda")
    skp = torch.full((3,), 12345, dtype=torch.int32, device="cuda")
    col = np.ascontiguousarray(KD.COLOURS_RGB)
    good = [desc.ctypes.data, d_desc.data_ptr(), 3, d_pool.data_ptr(), d_pool.numel(), d_pts.data_ptr(), d_win.data_ptr(), d_own.data_ptr(), 2,
            col.ctypes.data, cen.data_ptr(), skp.data_ptr(), _stream()]
    for i in (0, 1, 3, 5, 6, 7, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert L.kpt_draw_points(*args) == EARG
    torch.cuda.synchronize()
    assert np.array_equal(d_pool.cpu().numpy(), pool) and (cen == -7).all() and (skp == 12345).all()
    # the mosaic: S out of bounds, null pointers
    hm = torch.zeros(1, 7, 16, 16, device="cuda")
    out = torch.full((7 * 16 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert L.kpt_heatmap_mosaic(hm.data_ptr(), 1, 0, out.data_ptr(), _stream()) == EARG
    assert L.kpt_heatmap_mosaic(hm.data_ptr(), 1, 4097, out.data_ptr(), _stream()) == EARG
    assert L.kpt_heatmap_mosaic(None, 1, 16, out.data_ptr(), _stream()) == EARG
    assert L.kpt_heatmap_mosaic(hm.data_ptr(), 1, 16, None, _stream()) == EARG
    torch.cuda.synchronize()
    assert (out == 0xA5).all()


def _crop_raw(desc, pool, rects, count, K, S):
    """_crop with output buffers sized for a valid S, so that an S out of bounds cannot size them"""
    L = _lib()
    B = len(desc)
    d_desc, d_pool, d_rects, d_count = _dev(desc), _dev(pool), _dev(rects), _dev(count)
    crops = torch.full((B * K, 3, 16, 16), -3.0, dtype=torch.float32, device="cuda")
    owner = torch.full((B * K, 2), -7, dtype=torch.int32, device="cuda")
    window = torch.full((B * K, 4), -7, dtype=torch.int32, device="cuda")
    total = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = L.crop_resize_frames_u8(desc.ctypes.data, d_desc.data_ptr(), B, d_pool.data_ptr(), d_pool.numel(), d_rects.data_ptr(),
                                 d_count.data_ptr(), K, K, S, crops.data_ptr(), owner.data_ptr(), window.data_ptr(), total.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, crops.cpu().numpy(), owner.cpu().numpy(), window.cpu().numpy(), int(total.cpu()[0])


def test_map_boxes_is_the_draw_without_the_outline():
    """mdcv_detect_map_boxes: frame_boxes, rects and skipped are mdcv_detect_draw_boxes' bytes, and no pool is touched"""
    L = _lib()
    sizes = [(37, 23), (128, 96)]
    K = 8
    desc = np.zeros((2, 6), np.int64)
    boxes = np.zeros((2, K, 4), np.float32)
    at = 0
    for b, (w, h) in enumerate(sizes):
        ratio, pw, ph = C.letterbox(w, h, 64)
        desc[b] = [at, w, h, np.array([ratio]).view(np.int64)[0], pw, ph]
        at += 3 * w * h
        boxes[b] = C.to_detector(C.frame_boxes(w, h, 400 + b)[:K], ratio, pw, ph)
    boxes[1, [2, 5]] = C.bad_boxes()[[0, 3]]
    count = np.array([8, 7], np.int32)
    pool = np.zeros(at, np.uint8)
    _, want_fb, want_rects, want_skipped = D.draw_batch(pool, desc, boxes, count)
    d_desc, d_boxes, d_count = _dev(desc), _dev(boxes), _dev(count)
    fb = torch.full((2, K, 4), float("nan"), dtype=torch.float64, device="cuda")
    rects = torch.full((2, K, 4), -7, dtype=torch.int32, device="cuda")
    skipped = torch.full((2,), 12345, dtype=torch.int32, device="cuda")
    rc = L.detect_map_boxes(desc.ctypes.data, d_desc.data_ptr(), 2, d_boxes.data_ptr(), d_count.data_ptr(), K, at, fb.data_ptr(), rects.data_ptr(),
                            skipped.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(fb.cpu().numpy().view(np.int64), want_fb.view(np.int64))
    assert np.array_equal(rects.cpu().numpy(), want_rects) and np.array_equal(skipped.cpu().numpy(), want_skipped) and want_skipped[1] == 2


# ------------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def mini():
    from mdcv.yolo.models import Darknet
    cwd = os.getcwd()
    os.chdir(os.path.join(G, "mini"))
    try:
        net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
        net.load_weights("mini.weights", net.get_start_weight_dim())
    finally:
        os.chdir(cwd)
    return net.cuda().eval()


@pytest.fixture(scope="module")
def kpnet():
    from mdcv.rektnet.keypoint_net import KeypointNet
    torch.manual_seed(7)
    return KeypointNet(7, (80, 80), precision="fp32").cuda().eval()


@pytest.fixture(scope="module")
def scene(mini):
    """Three frames of three sizes and a confidence threshold, chosen from the model's own objectness: the frame in the middle is the
    candidate whose highest objectness is lowest and the threshold lies just above that, so it keeps nothing; the other two are the
    candidates of other sizes with the most cells above the threshold.  Candidates: the golden frames of the detect tests and seeded
    random frames of detect_cases' sizes."""
    from mdcv.data import images as I
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    cand = [np.ascontiguousarray(z[k]) for k in sorted(z.files)]
    cand += [C.random_frame(w, h, 800 + i) for i, (w, h) in enumerate(C.SIZES[1:])]
    cand += [np.full((40, 56, 3), 127, np.uint8), np.zeros((33, 47, 3), np.uint8)]
    W, H = mini.img_size()
    geoms = [I.sample_geometry(f.shape[1], f.shape[0], W, H, ts=False) for f in cand]
    with torch.no_grad():
        obj = mini(I.transform_batch(cand, geoms, bw=mini.get_bw()))[..., 4].float().cpu().numpy()
    top = obj.max(axis=1)
    quiet = int(np.argmin(top))
    above = np.sort(obj[obj > top[quiet]])
    assert len(above), "every candidate frame has the same highest objectness"
    thres = float((np.float64(top[quiet]) + np.float64(above[0])) / 2)
    score = (obj > thres).sum(axis=1)
    order = [i for i in np.argsort(-score, kind="stable") if i != quiet]
    first = order[0]
    second = next(i for i in order[1:] if cand[i].shape not in (cand[first].shape, cand[quiet].shape))
    frames = [cand[first], cand[quiet], cand[second]]
    assert len({f.shape for f in frames}) == 3
    print("scene: candidates", [f.shape for f in cand], "cells above", score.tolist(), "threshold", thres, "chosen", (first, quiet, second))
    return frames, thres


def _expected_batch(frames, results, kpnet, bucket, max_cones):
    """one batch: the crops of the returned rects cut out of the ORIGINAL frames, and kpnet on them in the same padded batch"""
    rects = np.zeros((len(frames), max(max(len(r.rects) for r in results), 1), 4), np.int32)
    for b, r in enumerate(results):
        rects[b, :len(r.rects)] = r.rects
    count = np.array([len(r.rects) for r in results], np.int32)
    crops, owner, window, M = KD.crop_frames(frames, rects, count, max_cones, 80)
    pts = np.zeros((0, 7, 2), F)
    if M:
        rows = (M + bucket - 1) // bucket * bucket
        batch = np.zeros((rows, 3, 80, 80), F)
        batch[:M] = crops
        with torch.no_grad():
            pts = kpnet(torch.from_numpy(batch).cuda())[1][:M].cpu().numpy()
    return crops, owner, window, pts


def test_frame_cone_detector_end_to_end(mini, kpnet, scene):
    from mdcv.yolo.detect import FrameConeDetector, FrameDetector
    frames, thres = scene
    bucket = 8
    plain = list(FrameDetector(mini, conf_thres=thres, batch_size=2).detect_frames(frames))
    det = FrameConeDetector(mini, kpnet, conf_thres=thres, batch_size=2, bucket=bucket)
    got = list(det.detect_frames(frames, return_crops=True))
    kept = [len(r.boxes) for r in got]
    print("boxes per frame", kept, "with a crop", [int(r.has_crop.sum()) for r in got])
    assert sum(kept) >= 5 and min(kept) == 0                                    # not vacuous: boxes, and a frame without any
    assert sum(int(r.has_crop.sum()) for r in got) >= 5
    # stage 1: the boxes are FrameDetector's, bit for bit
    for g, p in zip(got, plain):
        assert np.array_equal(g.boxes.view(np.int64), p.boxes.view(np.int64)) and np.array_equal(g.rects, p.rects)
        assert np.array_equal(g.prob, p.prob) and g.skipped == p.skipped
    for lo, hi in ((0, 2), (2, 3)):                                             # the two batches
        fr, res = frames[lo:hi], got[lo:hi]
        crops, owner, window, pts = _expected_batch(fr, res, kpnet, bucket, det.max_cones)
        for b, r in enumerate(res):
            rows = np.nonzero(owner[:, 0] == b)[0]
            n = len(r.rects)
            has = np.zeros(n, bool)
            has[owner[rows, 1]] = True
            assert np.array_equal(r.has_crop, has) and r.keypoints.shape == (n, 7, 2) and r.keypoints_frame.shape == (n, 7, 2)
            # stage 2: the crops are the NumPy resize of the rect windows of the original frame
            assert np.array_equal(r.crops.view(np.int32), crops[rows].view(np.int32))
            # stage 3: the key points are keypoint_net's on those crops in the same padded batch
            np.testing.assert_allclose(r.keypoints[has], pts[rows], atol=2e-4)
            assert np.isnan(r.keypoints[~has]).all() and (r.keypoints_frame[~has] == -1).all()
            # stage 4: outlines, then discs, drawn by NumPy from the RETURNED rects and key points on the original frame
            want = fr[b].copy()
            for rect in r.rects:
                if tuple(rect) != D.SKIPPED_RECT:
                    D.draw_rect(want, rect)
            skipped = 0
            for m, k in zip(rows, owner[rows, 1]):
                for i in range(7):
                    c = KD.center(r.keypoints[k, i], window[m])
                    if c is None:
                        skipped += 1
                        assert tuple(r.keypoints_frame[k, i]) == (-1, -1)
                        continue
                    assert tuple(r.keypoints_frame[k, i]) == c
                    KD.draw_disc(want, c[0], c[1], KD.COLOURS_RGB[i])
            assert r.skipped_points == skipped
            assert r.annotated.dtype == np.uint8 and np.array_equal(r.annotated, want)
    assert any((r.annotated != p.annotated).any() for r, p in zip(got, plain))  # the discs are there
    # the pixels stay on the device; max_cones caps the crops, not the boxes
    kept_dev = list(det.detect_frames(frames, keep_on_device=True))
    for k, g in zip(kept_dev, got):
        assert torch.is_tensor(k.annotated) and k.annotated.is_cuda and np.array_equal(k.annotated.cpu().numpy(), g.annotated) and k.crops is None
    one = list(FrameConeDetector(mini, kpnet, conf_thres=thres, batch_size=2, bucket=bucket, max_cones=1).detect_frames(frames))
    for o, g in zip(one, got):
        assert np.array_equal(o.rects, g.rects) and o.has_crop.sum() == min(1, int(g.has_crop[:1].sum())) and not o.has_crop[1:].any()


def test_two_synchronisations_per_batch(mini, kpnet, scene, monkeypatch):
    from mdcv.yolo.detect import FrameConeDetector
    frames, thres = scene
    calls = []

    def counted(owner, name, cuda_only):
        orig = getattr(owner, name)

        def wrapper(self, *a, **kw):
            if not cuda_only or self.is_cuda:
                calls.append(name)
            return orig(self, *a, **kw)
        monkeypatch.setattr(owner, name, wrapper)
    counted(torch.cuda.Event, "synchronize", False)
    counted(torch.cuda.Stream, "synchronize", False)
    for name in ("item", "cpu", "tolist", "numpy"):
        counted(torch.Tensor, name, True)
    orig_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (calls.append("device"), orig_sync(*a, **kw))[1])
    seen = {}
    for what, conf in (("few", thres), ("many", thres * 0.25)):
        det = FrameConeDetector(mini, kpnet, conf_thres=conf, batch_size=2, bucket=8)
        list(det.detect_frames(frames))                                         # plans and pinned buffers
        calls.clear()
        res = list(det.detect_frames(frames))
        seen[what] = (len(calls), sum(len(r.boxes) for r in res))
    print("synchronisations, boxes:", seen)
    assert seen["many"][1] > seen["few"][1] >= 5
    assert seen["few"][0] <= 2 * 2 and seen["many"][0] <= 2 * 2                 # two batches: at most two each, whatever the box count


# ------------------------------------------------------------------------------------------------------- mdcv.rektnet.detect on files
def test_rektnet_detect_files(kpnet, tmp_path):
    from PIL import Image
    from mdcv.rektnet import detect as RD
    src, out = tmp_path / "in", tmp_path / "out"
    os.makedirs(src), os.makedirs(out)
    crops = [KN.make_crop(29, 37, 1), KN.make_crop(64, 48, 2), KN.make_crop(90, 61, 3)]
    names = ["vid_3_frame_100_0.png", "vid_3_frame_100_1.png", "zed_vid_3_frame_100_2.png"]
    for n, c in zip(names, crops):
        Image.fromarray(c).save(src / n)
    (src / "notes.txt").write_text("not an image")
    got = list(RD.KeypointDetector(kpnet, img_size=80).detect_crops(crops))
    pool_want = []
    for c, (kp, centers, annotated, mosaic) in zip(crops, got):
        h, w = c.shape[:2]
        assert kp.shape == (7, 2) and kp.dtype == np.float32 and mosaic.shape == (7 * 80, 80) and mosaic.dtype == np.uint8
        want = c.copy()
        for i in range(7):
            cen = KD.center(kp[i], (0, 0, w, h))
            assert cen is not None and tuple(centers[i]) == cen
            KD.draw_disc(want, cen[0], cen[1], KD.COLOURS_RGB[i])
        assert np.array_equal(annotated, want) and (annotated != c).any()
        pool_want.append(want)
    # the key points and the mosaic are the model's on the NumPy-resized crops, in the same batch
    with torch.no_grad():
        hm, pts = kpnet(torch.from_numpy(np.stack([KN.image(c, 80) for c in crops])).cuda())
    np.testing.assert_allclose(np.stack([g[0] for g in got]), pts.cpu().numpy(), atol=2e-4)
    for g in got:                                                               # every map normalised on its own: each block spans 0..255
        blocks = g[3].reshape(7, 80 * 80)
        assert (blocks.min(axis=1) == 0).all() and (blocks.max(axis=1) == 255).all()
    paths = RD.detect(kpnet, str(src), 80, str(out) + "/", False, False, ext=".png")
    stems = ["vid_3_frame_100_0", "vid_3_frame_100_1", "vid_3_frame_100_2"]     # detect.py:25: the last five words
    assert paths == [(os.path.join(str(out) + "/", s + "_inference.png"), str(out) + "/" + s + "_hm.png") for s in stems]
    for (inf, hmp), g in zip(paths, got):
        assert np.array_equal(np.asarray(Image.open(inf)), g[2]) and np.array_equal(np.asarray(Image.open(hmp)), g[3])
    # one file, the reference's default extension, and a checkpoint path loaded as detect.py:36-37 loads it
    ckpt = str(tmp_path / "kp.pt")
    torch.save({"model": kpnet.state_dict()}, ckpt)
    (inf, hmp), = RD.detect(ckpt, str(src / names[0]), 80, str(out) + "/", flip=True, rotate=True)
    assert inf.endswith("vid_3_frame_100_0_inference.jpg") and hmp.endswith("vid_3_frame_100_0_hm.jpg")
    assert Image.open(inf).size == (37, 29) and Image.open(hmp).size == (80, 560) and Image.open(hmp).mode == "L"
