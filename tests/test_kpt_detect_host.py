"""Host side of the cone key-point path (csrc/kpt_detect.hip, mdcv.yolo.detect.FrameConeDetector, mdcv.rektnet.detect): the NumPy
restatements of tests/helpers/kpt_draw_numpy.py against literal statements of the rules, and the layout code of the two classes.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kpt_draw_numpy as KD  # noqa: E402
import kptload_numpy as KN  # noqa: E402

F = np.float32


# ------------------------------------------------------------------------------------------------------------------------- the disc
def test_disc_is_the_13_pixel_mask():
    """drawing.cpp's filled circle of radius 2: row cy five pixels, rows cy +- 1 three, rows cy +- 2 one"""
    assert KD.DISC.sum() == 13
    assert [int(r.sum()) for r in KD.DISC] == [1, 3, 5, 3, 1]
    yy, xx = np.mgrid[-2:3, -2:3]
    assert np.array_equal(KD.DISC, np.abs(xx) + np.abs(yy) <= 2)          # the kernel's test
    img = np.zeros((9, 11, 3), np.uint8)
    KD.draw_disc(img, 5, 4, (1, 2, 3))
    want = np.zeros((9, 11), bool)
    want[2:7, 3:8] = KD.DISC
    assert np.array_equal((img == (1, 2, 3)).all(-1), want) and np.array_equal(img[~want], np.zeros((int((~want).sum()), 3), np.uint8))


@pytest.mark.parametrize("cx,cy", [(0, 0), (10, 0), (0, 8), (10, 8), (5, 0), (5, 8), (0, 4), (10, 4),          # on corners and edges
                                   (-1, 4), (11, 4), (5, -1), (5, 9), (-2, -2), (12, 10), (-1, -1),            # one and two pixels outside
                                   (-3, 4), (13, 4), (5, -3), (5, 11), (100, 100)])                            # fully outside
def test_disc_clipping(cx, cy):
    H, W = 9, 11
    img = np.zeros((H, W, 3), np.uint8)
    KD.draw_disc(img, cx, cy, (9, 9, 9))
    big = np.zeros((H + 240, W + 240), bool)                               # the unclipped disc on a large canvas, then cut
    big[cy + 120 - 2:cy + 120 + 3, cx + 120 - 2:cx + 120 + 3] = KD.DISC
    assert np.array_equal((img == 9).all(-1), big[120:120 + H, 120:120 + W])


# --------------------------------------------------------------------------------------------------------------------- last writer
def _pool_of(frames):
    offs, at = [], 5                                                       # unaligned offsets, guard bytes around
    for f in frames:
        offs.append(at)
        at += f.size + 7
    pool = np.full(at, 0x5A, np.uint8)
    for f, o in zip(frames, offs):
        pool[o:o + f.size] = f.reshape(-1)
    desc = np.array([[o, f.shape[1], f.shape[0], 0, 0, 0] for f, o in zip(frames, offs)], np.int64)
    return pool, desc


def last_writer(pool, desc, centers, ok, owner, colours):
    """the kernel's rule, stated without a drawing order: a pixel takes the colour of the LAST point, in (cone, key point) order among the
    cones of its image, whose clipped disc covers it"""
    pool = pool.copy()
    for b in range(len(desc)):
        off, W, H = (int(v) for v in desc[b, :3])
        img = pool[off:off + 3 * W * H].reshape(H, W, 3)
        rank = np.full((H, W), -1)
        for m in np.nonzero(owner[:, 0] == b)[0]:
            for i in range(7):
                if ok[m, i]:
                    ys, xs = np.mgrid[0:H, 0:W]
                    cover = np.abs(xs - centers[m, i, 0]) + np.abs(ys - centers[m, i, 1]) <= 2
                    rank[cover] = np.maximum(rank[cover], m * 7 + i)
        for y, x in zip(*np.nonzero(rank >= 0)):
            img[y, x] = colours[rank[y, x] % 7]
    return pool


def test_last_writer_equals_sequential_loop():
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 200, (13, 17, 3), dtype=np.uint8), rng.integers(0, 200, (8, 9, 3), dtype=np.uint8)]
    pool, desc = _pool_of(frames)
    M = 12
    owner = np.array([[0 if m < 8 else 1, m] for m in range(M)], np.int32)
    window = np.array([[0, 0, 17, 13] if m < 8 else [1, 2, 7, 5] for m in range(M)], np.int32)
    pts = rng.uniform(-0.2, 1.2, (M, 7, 2)).astype(F)                       # crowded: most discs overlap others, some leave the image
    pts[3, 2] = np.nan
    got, centers, skipped = KD.draw_points(pool, desc, pts, window, owner)
    assert list(skipped) == [1, 0] and tuple(centers[3, 2]) == (-1, -1)
    ok = np.array([[KD.center(pts[m, i], window[m]) is not None for i in range(7)] for m in range(M)])
    assert ok.sum() == 7 * M - 1 and all(tuple(centers[m, i]) == KD.center(pts[m, i], window[m]) for m, i in zip(*np.nonzero(ok)))
    assert np.array_equal(got, last_writer(pool, desc, centers, ok, owner, KD.COLOURS_RGB))
    assert (got != pool).any() and np.array_equal(got[:5], pool[:5])


def test_colours_are_the_reference_table_reversed():
    from mdcv.yolo.detect import KPT_COLOURS_RGB, colour_table
    bgr = [(0, 255, 0), (255, 0, 0), (255, 255, 0), (0, 255, 255), (255, 0, 255), (127, 255, 127), (255, 127, 127)]     # RektNet/utils.py:62
    assert [tuple(c) for c in KPT_COLOURS_RGB] == [c[::-1] for c in bgr]
    assert np.array_equal(colour_table(KPT_COLOURS_RGB), KD.COLOURS_RGB) and colour_table(KPT_COLOURS_RGB).dtype == np.uint8
    with pytest.raises(ValueError):
        colour_table(KPT_COLOURS_RGB[:6])
    with pytest.raises(ValueError):
        colour_table([(0, 0, 256)] * 7)


# ----------------------------------------------------------------------------------------------------------------------- the centre
def test_center_truncates_the_double_product():
    assert KD.center((F(0.5), F(0.25)), (10, 20, 8, 8)) == (14, 22)
    assert KD.center((F(-0.3), F(0.999)), (10, 20, 8, 8)) == (10 + int(-2.4000000953674316), 20 + 7) == (8, 27)     # toward zero
    assert KD.center((F(np.nan), F(0.5)), (0, 0, 8, 8)) is None and KD.center((F(0.5), F(np.inf)), (0, 0, 8, 8)) is None
    assert KD.center((F(2.0 ** 20), F(0.5)), (0, 0, 1024, 8)) is None       # 2^30: refused
    assert KD.center((F(2.0 ** 20), F(0.5)), (0, 0, 1023, 8)) == (1023 * 2 ** 20, 4)
    # a float32 point whose product with w lies just under an integer in double and ON it in float32: found by search
    found = None
    for w in range(3, 200):
        for k in range(1, w):
            p = np.nextafter(F(k / w), F(0))
            for q in (p, F(k / w)):
                if int(np.float64(q) * w) != int(F(q) * F(w)):
                    found = (q, w)
                    break
            if found:
                break
        if found:
            break
    assert found is not None
    q, w = found
    d, s = int(np.float64(q) * np.float64(w)), int(F(q) * F(w))
    assert d != s and abs(d - s) == 1
    assert KD.center((q, q), (0, 0, w, w)) == (d, d)                        # the float64 rule (NumPy 1.x's `int(pt[0] * w)`)


# ----------------------------------------------------------------------------------------------------------------------- the mosaic
def _literal_mosaic(hm_b):
    """detect.py:40-47 as written, for one sample, then cv2.imwrite's conversion of `out * 255`"""
    out = np.empty(shape=(0, hm_b.shape[2]))
    for o in hm_b:
        chan = np.array(o)
        cmin = chan.min()
        cmax = chan.max()
        chan -= cmin
        chan /= cmax - cmin
        out = np.concatenate((out, chan), axis=0)
    return np.clip(np.rint(out * 255), 0, 255).astype(np.uint8)


def tie_map(S):
    """a float32 map with min 0 and max 1 holding 0.5 / 255 * k values that scale exactly onto .5: (x - 0) / 1 * 255 = k + 0.5"""
    m = np.linspace(0, 1, S * S, dtype=F).reshape(S, S)
    m[1, 1], m[1, 2], m[2, 1] = F(0.5), F(0.1171875), F(0.12109375)         # 127.5 -> 128, 29.8828125, 30.87890625
    m[3, 3] = F(2.5 / 255)                                                  # not exact in float32: stays off the tie
    m[4, 4] = F(0.5 + 1 / 255)
    return m


def test_mosaic_follows_the_reference_statements():
    rng = np.random.default_rng(11)
    S = 16
    hm = rng.standard_normal((3, 7, S, S)).astype(F)
    hm[0, 2] = np.abs(hm[0, 2]) * F(1e-6)                                   # a softmax-like map: tiny positive values
    hm[1, 3] = tie_map(S)
    got = KD.mosaic(hm)
    assert got.shape == (3, 7 * S, S) and got.dtype == np.uint8
    for b in range(3):
        assert np.array_equal(got[b], _literal_mosaic(hm[b]))
    assert got[1, 3 * S + 1, 1] == 128 and float(hm[1, 3, 1, 1]) * 255 == 127.5         # the tie goes to the even neighbour
    for c in range(7):                                                      # every map spans 0..255
        blk = got[0, c * S:(c + 1) * S]
        assert blk.min() == 0 and blk.max() == 255
    flat = hm.copy()
    flat[2, 5] = F(0.25)                                                    # a constant map: zeros, where the reference divides by zero
    got = KD.mosaic(flat)
    assert not got[2, 5 * S:6 * S].any()
    keep = np.ones(7 * S, bool)
    keep[5 * S:6 * S] = False
    assert np.array_equal(got[2][keep], _literal_mosaic(hm[2])[keep])
    flat[2, 6, 3, 3] = np.nan
    assert not KD.mosaic(flat)[2, 6 * S:].any()


# ---------------------------------------------------------------------------------------------------------------- windows and order
def test_window_clipping():
    W, H = 37, 29
    assert KD.clip_window((3, 4, 10, 12), W, H) == (3, 4, 8, 9)
    assert KD.clip_window((5, 6, 5, 6), W, H) == (5, 6, 1, 1)
    assert KD.clip_window((-4, -9, 10, 12), W, H) == (0, 0, 11, 13)
    assert KD.clip_window((30, 20, 40, 50), W, H) == (30, 20, 7, 9)
    assert KD.clip_window((-5, -5, 99, 99), W, H) == (0, 0, W, H)
    assert KD.clip_window((0, 0, -1, -1), W, H) is None                     # the skipped rect
    assert KD.clip_window((37, 3, 40, 9), W, H) is None and KD.clip_window((-9, 3, -1, 9), W, H) is None
    assert KD.clip_window((3, 29, 9, 31), W, H) is None and KD.clip_window((3, -4, 9, -1), W, H) is None
    assert KD.clip_window((0, 0, 4096, 3), 5000, 10) is None and KD.clip_window((0, 0, 4095, 3), 5000, 10) == (0, 0, 4096, 4)


def test_crop_order_is_an_exclusive_prefix():
    frames = [KN.make_crop(29, 37, 1), KN.make_crop(48, 64, 2), KN.make_crop(10, 12, 3)]
    K = 4
    rects = np.zeros((3, K, 4), np.int32)
    rects[0] = [[1, 1, 9, 9], [0, 0, -1, -1], [30, 20, 50, 50], [2, 2, 3, 3]]
    rects[1] = [[5, 5, 20, 30]] * K
    rects[2] = [[0, 0, 11, 9], [100, 100, 120, 120], [-3, -3, 2, 2], [4, 4, 4, 4]]
    count = np.array([4, 0, 3], np.int32)
    crops, owner, window, M = KD.crop_frames(frames, rects, count, per=3, size=16)
    assert M == 4 and crops.shape == (4, 3, 16, 16) and crops.dtype == F
    assert owner.tolist() == [[0, 0], [0, 2], [2, 0], [2, 2]]               # frame 1 keeps none; slot 3 of frame 0 is past `per`
    assert window.tolist() == [[1, 1, 9, 9], [30, 20, 7, 9], [0, 0, 12, 10], [0, 0, 3, 3]]
    assert np.array_equal(crops[1], KN.image(frames[0][20:29, 30:37], 16))
    from mdcv.yolo.detect import scatter_cones
    pts = np.arange(M * 14, dtype=F).reshape(M, 7, 2)
    cen = np.arange(M * 14, dtype=np.int32).reshape(M, 7, 2)
    kp, kf, has, rows = scatter_cones(owner, pts, cen, 0, 4)
    assert has.tolist() == [True, False, True, False] and rows.tolist() == [0, 1]
    assert np.array_equal(kp[2], pts[1]) and np.isnan(kp[1]).all() and (kf[1] == -1).all() and np.array_equal(kf[0], cen[0])
    kp, kf, has, rows = scatter_cones(owner, pts, cen, 1, 0)
    assert kp.shape == (0, 7, 2) and len(rows) == 0


# --------------------------------------------------------------------------------------------------------------- the classes' layout
def _regions(plan, names):
    offs = [getattr(plan, n) for n in names]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs) and offs[-1] <= plan.nbytes
    return offs


def test_cone_batch_plan_layout():
    from mdcv.yolo.detect import BatchPlan, ConeBatchPlan, padded_rows
    sizes = [(37, 29), (64, 48), (12, 10)]
    base, plan = BatchPlan(sizes, 64, 64, 200), ConeBatchPlan(sizes, 64, 64, 200, 5)
    for n in ("det_off", "pool_off", "in_bytes", "fb_off", "rect_off", "prob_off", "count_off", "skip_off", "offsets", "pool_bytes"):
        assert getattr(base, n) == getattr(plan, n)                         # FrameDetector's layout, untouched, with the cone tables behind
    assert plan.per == 5 and plan.cap == 15 and plan.total_off == base.nbytes
    offs = _regions(plan, ("total_off", "owner_off", "window_off", "pts_off", "centers_off", "kskip_off"))
    need = [4, 15 * 8, 15 * 16, 15 * 56, 15 * 56, 3 * 4]
    for o, n, nxt in zip(offs, need, offs[1:] + [plan.nbytes]):
        assert o + n <= nxt                                                 # no region overlaps the next
    assert ConeBatchPlan(sizes, 64, 64, 4, 64).per == 4                     # never more crops than box slots
    assert [padded_rows(m, 64) for m in (0, 1, 64, 65)] == [0, 64, 64, 128]


def test_crop_batch_plan_layout_and_names():
    from mdcv.rektnet.detect import CropBatchPlan, image_name
    crops = [KN.make_crop(29, 37, 1), KN.make_crop(48, 64, 2), KN.make_crop(1, 1, 3)]
    plan = CropBatchPlan([(c.shape[1], c.shape[0]) for c in crops], 16)
    offs = _regions(plan, ("desc_off", "rect_off", "count_off", "pool_off", "pts_off", "centers_off", "skip_off", "owner_off", "window_off",
                           "total_off", "mosaic_off"))
    need = [3 * 48, 3 * 16, 3 * 4, plan.pool_bytes, 3 * 56, 3 * 56, 3 * 4, 3 * 8, 3 * 16, 4, 3 * 7 * 256]
    for o, n, nxt in zip(offs, need, offs[1:] + [plan.nbytes]):
        assert o + n <= nxt
    host = np.full(plan.in_bytes, 0xEE, np.uint8)
    plan.pack(host, crops)
    desc = host[:3 * 48].view(np.int64).reshape(3, 6)
    assert desc[:, 1:3].tolist() == [[37, 29], [64, 48], [1, 1]] and (desc[:, 3].view(np.float64) == 1.0).all() and not desc[:, 4:].any()
    assert host[plan.rect_off:plan.rect_off + 48].view(np.int32).reshape(3, 4).tolist() == [[0, 0, 36, 28], [0, 0, 63, 47], [0, 0, 0, 0]]
    assert host[plan.count_off:plan.count_off + 12].view(np.int32).tolist() == [1, 1, 1]
    for c, off in zip(crops, desc[:, 0]):
        assert off % 16 == 0 and np.array_equal(host[plan.pool_off + off:plan.pool_off + off + c.size], c.reshape(-1))
    for c, r in zip(crops, plan.rects):                                     # the whole-image rect clips to the whole image
        assert KD.clip_window(r, c.shape[1], c.shape[0]) == (0, 0, c.shape[1], c.shape[0])
    with pytest.raises(ValueError):
        CropBatchPlan([(4097, 3)], 16)
    assert image_name("a/b/vid_3_frame_22063_0.jpg") == "vid_3_frame_22063_0"           # detect.py:25
    assert image_name("x/one_two_three_four_five_six_seven.png") == "three_four_five_six_seven"
    assert image_name("plain.tar.gz") == "plain"
