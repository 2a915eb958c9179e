"""Host half of the key-point crop loader (mdcv/data/crops.py) and the numpy helpers its GPU tests compare against; no GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import kptload_numpy as N  # noqa: E402
from mdcv.data import crops as C  # noqa: E402
from oracle import synth_oracle as SO  # noqa: E402

KEYS = ["top", "mid_L_top", "mid_R_top", "mid_L_bot", "mid_R_bot", "bot_L", "bot_R"]


# ---------------------------------------------------------------------------------------------------- the numpy helpers at any size
@pytest.mark.parametrize("size", [80, 48])
@pytest.mark.parametrize("h,w", [(13, 9), (131, 97), (40, 1), (10, 300)])
def test_helpers_work_at_arbitrary_sizes(h, w, size):
    crop, label = N.make_crop(h, w, h * 1000 + w), N.make_label(h, w, h + w)
    img, hm, pts = N.sample(crop, label, size)
    assert img.shape == (3, size, size) and hm.shape == (7, size, size) and pts.shape == (7, 2)
    assert img.dtype == hm.dtype == pts.dtype == np.float32
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    lvl = img.astype(np.float64) * 255.0
    assert np.abs(lvl - np.rint(lvl)).max() < 1e-4                           # every value is an 8-bit level / 255
    for k in range(7):
        if np.isnan(hm[k]).any():
            assert np.isnan(hm[k]).all()                                     # a missed tap: the whole map is 0 / 0
        else:
            assert abs(float(hm[k].astype(np.float64).sum()) - 1.0) < 1e-5
    assert (pts >= 0).all() and (pts <= 1).all()


def test_helper_image_is_bgr():
    crop = np.empty((20, 30, 3), np.uint8)
    crop[:] = (10, 20, 30)                                                   # R, G, B
    img = N.image(crop, 48)
    for plane, v in enumerate((30, 20, 10)):
        np.testing.assert_array_equal(img[plane], np.float32(v / 255.0))


def test_exact_half_is_the_rounded_2x2_mean():
    """160 -> 80: every tap pair has weights 1/2, 1/2, so INTER_LINEAR gives the 2x2 mean rounded half up -- the bytes INTER_AREA gives,
    to which cv2.resize switches at an exact 2x down-scale."""
    crop = N.make_crop(160, 160, 7)
    s = crop.astype(np.int64)
    mean = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    want = (mean[:, :, ::-1].transpose(2, 0, 1).astype(np.float64) / 255.0).astype(np.float32)
    np.testing.assert_array_equal(N.image(crop, 80), want)


def test_same_size_is_the_identity():
    crop = N.make_crop(80, 80, 8)
    want = (crop[:, :, ::-1].transpose(2, 0, 1).astype(np.float64) / 255.0).astype(np.float32)
    np.testing.assert_array_equal(N.image(crop, 80), want)


def test_missed_tap_sums():
    """200 -> 80 reads sources 0, 1 | 3, 4 | 5, 6 | ... (centres 0.75, 3.25, 5.75): pixel 2 is never read, pixel 3 with weight 0.75"""
    assert sum(N.resized_axis(2, 200, 80).tolist()) == 0.0 and sum(N.axis_vector(2, 200, 80).tolist()) == 0.0
    assert sum(N.resized_axis(3, 200, 80).tolist()) == 0.75
    # the blur keeps a zero vector zero; next to the border REFLECT_101 counts sample 1 twice in output 0: 0.75 * (1 + 4 / 16)
    assert sum(N.axis_vector(3, 200, 80).tolist()) == 0.9375
    hm = N.heatmap(2.7, 5.0, 40, 200, 80)
    assert np.isnan(hm).all()
    assert np.isfinite(N.heatmap(3.2, 5.0, 40, 200, 80)).all()
    # the loader's host-side test for the warning agrees with the oracle's vectors, hot pixel by hot pixel
    for src, dst in ((200, 80), (300, 48), (131, 80), (13, 80), (1, 48), (160, 80)):
        mask = C._read_mask(src, dst)
        for hot in range(src):
            assert bool(mask[hot]) == (SO._resize_onehot_axis(hot, src, dst).sum() > 0), (src, dst, hot)
    np.testing.assert_array_equal(C.zero_sum_maps([(2, 5), (3, 5)], 40, 200, 80), [True, False])


# ------------------------------------------------------------------------------------------------------------------- points
def test_points_follow_scale_labels():
    label = np.array([[3.9, 7.2], [0.0, 0.99], [12.5, 39.999], [5.0, 10.0], [8.7, 20.0], [1.2, 2.3], [15.99, 30.5]])
    h, w, S = 40, 16, 80                                                      # scales 2.0 and 5.0: int(pt) * scale is an exact integer
    got = C.scale_points(label, h, w, S)
    want = np.array([[math.ceil(int(x) * (S / w)) / S, math.ceil(int(y) * (S / h)) / S] for x, y in label]).astype(np.float32)
    np.testing.assert_array_equal(got, want)
    assert got[3, 0] == np.float32(25 / 80) and got[3, 1] == np.float32(20 / 80)      # exact products are not bumped by the ceil
    h, w = 131, 97                                                            # fractional scales: the ceil moves up
    label = N.make_label(h, w, 3)
    got = C.scale_points(label, h, w, S)
    np.testing.assert_array_equal(got, N.points(label, h, w, S))
    assert got.dtype == np.float32
    x0, y0 = int(label[0, 0]), int(label[0, 1])
    assert got[0, 0] == np.float32(math.ceil(x0 * (80 / 97)) / 80) and got[0, 1] == np.float32(math.ceil(y0 * (80 / 131)) / 80)


def test_label_outside_the_crop_raises():
    ok = np.full((7, 2), 3.5)
    assert C.hot_pixels(ok, 10, 12, "a.png").tolist() == [[3, 3]] * 7
    C.hot_pixels(np.array([[11.9, 9.9]] * 7), 10, 12, "a.png")               # int() keeps these inside
    C.hot_pixels(np.array([[-0.5, -0.9]] * 7), 10, 12, "a.png")              # int() truncates toward zero
    for bad in ((12.0, 3.0), (3.0, 10.0), (-1.0, 3.0), (3.0, -1.0)):
        lab = ok.copy()
        lab[4] = bad
        with pytest.raises(IndexError, match="cone_17.png"):
            C.hot_pixels(lab, 10, 12, "cone_17.png")


def test_decoder_must_give_three_channels():
    for shape in ((8, 8, 4), (8, 8, 1), (8, 8)):
        with pytest.raises(ValueError, match="a.png"):
            C._as_crop(np.zeros(shape, np.uint8), "a.png")
    with pytest.raises(ValueError, match="a.png"):
        C._as_crop(np.zeros((8, 8, 3), np.float32), "a.png")
    assert C._as_crop(np.zeros((8, 8, 3), np.uint8), "a.png").shape == (8, 8, 3)


def test_loader_raises_before_it_stages(tmp_path):
    """the IndexError comes from the host half (no GPU involved), with the image name"""
    from PIL import Image
    Image.fromarray(N.make_crop(20, 12, 0)).save(tmp_path / "c0.png")
    lab = np.full((7, 2), 2.0)
    lab[6] = (12.0, 5.0)                                                     # x = w
    ld = C.ConeCropBatches(["c0.png"], [lab], str(tmp_path), 80, 1, num_workers=1)
    with pytest.raises(IndexError, match="c0.png"):
        ld._sample(0)
    lab[6] = (5.0, -1.0)
    with pytest.raises(IndexError, match="c0.png"):
        C.ConeCropBatches(["c0.png"], [lab], str(tmp_path), 80, 1, num_workers=1)._sample(0)
    assert len(ld) == 1 and len(ld.dataset) == 1
    with pytest.raises(ValueError):
        C.ConeCropBatches(["c0.png"], [lab], str(tmp_path), (80, 64), 1)
    for s in (8, 264):
        with pytest.raises(ValueError):
            C.ConeCropBatches(["c0.png"], [lab], str(tmp_path), s, 1)


# ------------------------------------------------------------------------------------------------------------------ the CSV
def _write_dataset(tmp_path, heights):
    from PIL import Image
    rows = ["image,url," + ",".join(KEYS)]
    for i, h in enumerate(heights):
        name = f"cone_{i}.png"
        Image.fromarray(N.make_crop(h, 14, i)).save(tmp_path / name)
        cells = [f'"({k + 0.25 * i},{(k * h) // 8 + 0.5})"' for k in range(7)]
        if i == 1:
            cells = [""] * 7                                                 # an unlabelled row: first label NaN
        rows.append(",".join([name, "http://x"] + cells))
    path = tmp_path / "labels.csv"
    path.write_text("\n".join(rows) + "\n")
    return str(path)


def test_csv_parsing_split_and_cache(tmp_path, capsys):
    heights = [20, 30, 9, 10, 25, 40, 12, 33, 18, 27]                         # row 1 unlabelled, row 2 too short (h = 9), row 3 kept (h = 10)
    path = _write_dataset(tmp_path, heights)
    cache = tmp_path / "cache"
    seen = []

    def decode(p):
        from PIL import Image
        seen.append(os.path.basename(p))
        return Image.open(p).convert("RGB")

    ti, tl, vi, vl = C.load_train_csv_dataset(path, 0.3, KEYS, str(tmp_path), cache_location=str(cache), decode=decode)
    kept = [f"cone_{i}.png" for i in (0, 3, 4, 5, 6, 7, 8, 9)]
    assert "cone_1.png" not in seen and "cone_2.png" in seen                  # the NaN row is dropped before any decode
    assert list(vi) + list(ti) == kept
    n_val = int(8 * 0.3)
    assert len(vi) == len(vl) == n_val == 2 and len(ti) == len(tl) == 6
    lab = np.asarray(list(vl) + list(tl))
    assert lab.shape == (8, 7, 2)
    np.testing.assert_array_equal(lab[1], [[k + 0.25 * 3, (k * 10) // 8 + 0.5] for k in range(7)])       # cone_3
    files = sorted(os.path.relpath(os.path.join(d, f), cache) for d, _, fs in os.walk(cache) for f in fs)
    assert len(files) == 2 and files[0].endswith("images.npy") and files[1].endswith("labels.npy")
    assert len(files[0].split(os.sep)[0]) == 64                                # the sha256 folder

    def no_decode(p):
        raise AssertionError("the cache must be read, not the images")

    ti2, tl2, vi2, vl2 = C.load_train_csv_dataset(path, 0.3, KEYS, str(tmp_path), cache_location=str(cache), decode=no_decode)
    assert list(ti2) == list(ti) and list(vi2) == list(vi)
    np.testing.assert_array_equal(np.asarray(tl2), np.asarray(tl))
    np.testing.assert_array_equal(np.asarray(vl2), np.asarray(vl))
    assert "read from the cache" in capsys.readouterr().out
    ti3, _, vi3, _ = C.load_train_csv_dataset(path, 0.0, KEYS, str(tmp_path), decode=decode)             # no cache, no validation
    assert list(ti3) == kept and len(vi3) == 0
    text = open(path).read().replace('"(6.75,7.5)"', '"6.75;7.5"')             # cone_3's last cell
    bad = tmp_path / "bad.csv"
    bad.write_text(text)
    assert text != open(path).read()
    with pytest.raises(ValueError, match="cone_3.png"):
        C.load_train_csv_dataset(str(bad), 0.0, KEYS, str(tmp_path), decode=decode)


# ------------------------------------------------------------------------------------------------------------ the staging layout
def test_staging_layout_round_trips():
    shapes = [(13, 9), (131, 97), (40, 1), (10, 300)]
    crops = [N.make_crop(h, w, i) for i, (h, w) in enumerate(shapes)]
    labels = [N.make_label(h, w, i) for i, (h, w) in enumerate(shapes)]
    hots = [C.hot_pixels(l, h, w, "x") for l, (h, w) in zip(labels, shapes)]
    pts = [C.scale_points(l, h, w, 80) for l, (h, w) in zip(labels, shapes)]
    p = C.pack_layout(shapes)
    assert p.src_bytes == sum(3 * h * w for h, w in shapes)
    assert p.pts_off >= 4 * C.DESC * 4 and p.pix_off >= p.pts_off + 4 * 7 * 8 and p.nbytes >= p.pix_off + p.src_bytes
    assert p.pts_off % 16 == 0 and p.pix_off % 16 == 0
    buf = np.full(p.nbytes + 64, 0xAB, np.uint8)
    C.pack_batch(buf, p, crops, hots, pts)
    assert (buf[p.nbytes:] == 0xAB).all()
    desc = buf[:4 * C.DESC * 4].view(np.int32).reshape(4, C.DESC)
    offs = np.cumsum([0] + [3 * h * w for h, w in shapes])[:-1]
    np.testing.assert_array_equal(desc[:, 0], offs)
    assert offs[1] == 351 and offs[1] % 4 != 0                                 # a 13x9 crop is 351 bytes: the next one starts unaligned
    np.testing.assert_array_equal(desc[:, 1:3], shapes)
    assert (desc[:, 3] == 0).all() and (desc[:, 18:] == 0).all()
    c2, h2, p2 = C.unpack_batch(buf, p)
    for a, b in zip(crops, c2):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(h2, np.stack(hots))
    np.testing.assert_array_equal(p2, np.stack(pts))
    for b, (h, w) in enumerate(shapes):
        assert (h2[b, :, 0] < w).all() and (h2[b, :, 1] < h).all() and (h2[b] >= 0).all()


def test_header_declares_the_entry_point():
    from mdcv import _lib
    protos = _lib.parse_header()
    assert "mdcv_kptload_batch" in protos
    assert protos["mdcv_kptload_batch"][2] == ["desc_host", "desc", "B", "src", "src_bytes", "S", "images", "heatmaps", "stream"]
    text = open(_lib.HEADER).read()
    for name, v in (("MDCV_KPTLOAD_DESC", C.DESC), ("MDCV_KPTLOAD_MIN_SIZE", C.MIN_SIZE), ("MDCV_KPTLOAD_MAX_SIZE", C.MAX_SIZE),
                    ("MDCV_KPTLOAD_MAX_SIDE", C.MAX_SIDE)):
        assert f"#define {name} {v}\n" in text


def test_entry_rejects_bad_arguments_before_any_device_call():
    """the bounds are checked on the host copy of the table, so MDCV_EARG comes back without a GPU in the machine"""
    from mdcv import _lib
    L = _lib.lib()
    host = np.zeros((1, C.DESC), np.int32)
    src, out = np.zeros(4096, np.uint8), np.zeros(16, np.float32)

    def call(h, w, size, hot=(0, 0), res=0):
        host[0, :] = 0
        host[0, 1:4] = h, w, res
        host[0, 4:18] = list(hot) * 7
        return L.kptload_batch(host.ctypes.data, host.ctypes.data, 1, src.ctypes.data, src.nbytes, size, out.ctypes.data, out.ctypes.data, None)

    for size in (8, 15, 257, 264):
        assert call(8, 8, size) == -1
    assert call(C.MAX_SIDE + 1, 1, 80) == -1 and call(1, C.MAX_SIDE + 1, 80) == -1 and call(0, 8, 80) == -1
    assert call(37, 37, 80) == -1                                             # 4107 bytes: the crop ends past src
    assert call(8, 8, 80, hot=(8, 0)) == -1 and call(8, 8, 80, hot=(0, -1)) == -1 and call(8, 8, 80, res=1) == -1
