"""Real-image loader, host half (no GPU): Pillow's resize through the host coefficient tables, the descriptor / table layout the kernels
read (emulated in NumPy), the reference's labels, CSV / subset / length rules and the draws.  Golden data: tests/golden/imgload
(tests/golden/make_golden_imgload.py: Pillow 12.2 and the reference's label helpers)."""
import json
import os
import random
import warnings

import numpy as np
import pytest

from mdcv.data import images as I

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imgload")
NAMES = ["f0", "f1", "f2", "f3"]


def _npz(name):
    return np.load(os.path.join(G, name))


def _frames():
    z = _npz("frames.npz")
    return {k: z[k] for k in z.files}


def _resample(img, axis, first, count, kk):
    """Pillow's 8-bit pass along `axis` (1: horizontal, 0: vertical) fed the host tables; img uint8 [H, W, 3]"""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(first),) + src.shape[1:], np.int64)
    for j in range(len(first)):
        acc = np.full(src.shape[1:], 1 << (I.PRECISION_BITS - 1), np.int64)
        for t in range(count[j]):
            acc += src[first[j] + t] * int(kk[j, t])
        out[j] = np.clip(acc >> I.PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def _pillow_resize(img, w, h, filt):
    _, f, c, k = I.resample_coeffs(img.shape[1], w, filt)
    tmp = _resample(img, 1, f, c, k)
    _, f, c, k = I.resample_coeffs(img.shape[0], h, filt)
    return _resample(tmp, 0, f, c, k)


def _emulate(buf, p, C, H, W):
    """What the two kernels compute from a packed staging buffer (csrc/imgload.hip), in NumPy."""
    desc = buf[p.desc_off:p.desc_off + p.B * I.DESC * 4].view(np.int32).reshape(p.B, I.DESC)
    coefs = buf[p.coef_off:p.coef_off + p.n_coefs * 4].view(np.int32)
    src = buf[p.pix_off:p.pix_off + p.src_bytes]
    out = np.zeros((p.B, C, H, W), np.uint8)
    for b, d in enumerate(desc):
        win = src[d[0]:d[0] + 3 * d[1] * d[2]].reshape(d[2], d[1], 3).astype(np.int64)

        def px(y, x):
            if 0 <= y < d[2] and 0 <= x < d[1]:
                return win[y, x]
            return np.full(3, 127, np.int64)
        scr = np.zeros((d[8], d[7], 3), np.int64)
        for j in range(d[7]):
            e = coefs[d[5] + j * (d[3] + 2):d[5] + (j + 1) * (d[3] + 2)]
            for i in range(d[8]):
                acc = np.full(3, 1 << 21, np.int64)
                for t in range(e[1]):
                    acc += px(d[9] + i, e[0] + t) * int(e[2 + t])
                scr[i, j] = np.clip(acc >> 22, 0, 255)
        img = np.zeros((H, W, 3), np.int64)
        for oy in range(H):
            for ox in range(W):
                xr = (W - 1 - ox if d[17] else ox) + d[11]
                yr = oy + d[12]
                if 0 <= xr < d[7] and 0 <= yr < d[10]:
                    e = coefs[d[6] + yr * (d[4] + 2):d[6] + (yr + 1) * (d[4] + 2)]
                    acc = np.full(3, 1 << 21, np.int64)
                    for t in range(e[1]):
                        acc += scr[e[0] + t, xr] * int(e[2 + t])
                    img[oy, ox] = np.clip(acc >> 22, 0, 255)
                elif d[13] <= xr < d[14] and d[15] <= yr < d[16]:
                    img[oy, ox] = 127
        if C == 1:
            out[b, 0] = (img[..., 0] * 19595 + img[..., 1] * 38470 + img[..., 2] * 7471 + 0x8000) >> 16
        else:
            out[b] = np.moveaxis(img, -1, 0)
    return out


def _case(z, i):
    fi, ts, patch, flip, bw, W, H = (int(v) for v in z[f"c{i}_params"])
    return dict(name=NAMES[fi], ts=bool(ts), patch=patch, flip=bool(flip), bw=bool(bw), W=W, H=H, scale=float(z[f"c{i}_scale"]),
                u8=z[f"c{i}_u8"], labels=z[f"c{i}_labels"])


def _geom(c, frames, boxes):
    f = frames[c["name"]]
    empty = len(boxes[c["name"]]) == 0
    return I.sample_geometry(f.shape[1], f.shape[0], c["W"], c["H"], c["ts"], c["scale"], c["patch"], c["flip"] and not empty)


def _boxes():
    rows = I.read_label_csv(os.path.join(G, "dataset.csv"), "")
    return {os.path.splitext(os.path.basename(r[0]))[0]: r[4] for r in rows}


def test_fixture_provenance():
    meta = json.load(open(os.path.join(G, "meta.json")))
    assert meta["pillow"] == "12.2.0"


def test_coefficient_tables_reproduce_pillow_resize_byte_for_byte():
    frames, z = _frames(), _npz("resize.npz")
    for i in range(int(z["n"])):
        fi, w, h, f = (int(v) for v in z[f"r{i}_params"])
        got = _pillow_resize(frames[NAMES[fi]], w, h, I.LANCZOS if f == 0 else I.BILINEAR)
        assert np.array_equal(got, z[f"r{i}_out"]), (i, int((got != z[f"r{i}_out"]).sum()))


def test_coefficient_tables_are_cached_and_same_size_is_a_copy():
    assert I.resample_coeffs(301, 150, I.LANCZOS) is I.resample_coeffs(301, 150, I.LANCZOS)
    k, first, count, kk = I.resample_coeffs(57, 57, I.LANCZOS)
    assert k == 1 and np.array_equal(first, np.arange(57)) and (count == 1).all() and (kk == 1 << 22).all()
    k, _, count, kk = I.resample_coeffs(301, 150, I.LANCZOS)
    assert k == 15 and count.max() <= k
    assert (np.abs(kk.sum(1) - (1 << 22)) <= 8).all()


def test_descriptor_and_table_layout_reproduce_pillow_chain():
    """every golden sample, all in ONE packed batch per (W, H, C), through a NumPy emulation of the two kernels"""
    frames, boxes, z = _frames(), _boxes(), _npz("cases.npz")
    groups = {}
    for i in range(int(z["n"])):
        c = _case(z, i)
        groups.setdefault((c["W"], c["H"], c["u8"].shape[2]), []).append(c)
    for (W, H, C), cs in groups.items():
        geoms = [_geom(c, frames, boxes) for c in cs]
        wins = [I.crop_window(frames[c["name"]], g) for c, g in zip(cs, geoms)]
        p = I.pack_layout(geoms, [w.nbytes for w in wins], 0)
        buf = np.zeros(p.nbytes, np.uint8)
        I.pack_batch(buf, p, geoms, wins)
        got = _emulate(buf, p, C, H, W)
        for b, c in enumerate(cs):
            assert np.array_equal(got[b], np.moveaxis(c["u8"], -1, 0)), (c["name"], c["ts"], c["patch"], W, H)


def test_window_is_one_patch_of_pixels_not_the_frame():
    g = I.sample_geometry(1920, 1080, 416, 416, True, 0.5, 3)
    x, y, w, h = g.window
    assert w <= 2 * 416 + 16 and h <= 2 * 416 + 16 and (w, h) != (1920, 1080)
    g = I.sample_geometry(1920, 1080, 416, 416, True, 1.5, 0)
    assert g.window[2] <= 416 / 1.5 + 8 and g.window[3] <= 416 / 1.5 + 8


def test_labels_equal_the_reference_helpers_bitwise():
    frames, boxes, z = _frames(), _boxes(), _npz("cases.npz")
    T = int(z["T"])
    seen_empty_flip = False
    for i in range(int(z["n"])):
        c = _case(z, i)
        got = I.sample_labels(boxes[c["name"]], _geom(c, frames, boxes), T)
        assert got.dtype == np.float32 and got.shape == (T, 5)
        assert np.array_equal(got.view(np.uint32), c["labels"].view(np.uint32)), (i, got, c["labels"])
        seen_empty_flip |= bool((c["labels"][:, 1] == 1.0).any())
    assert seen_empty_flip            # a patch with no surviving label, flipped: rows with cx == 1.0, as the reference makes them


def test_filter_and_offset_mixed_precision_cases():
    f32 = np.float32
    lab = np.array([[0, 10.3, 20.7, 80.1, 90.9], [0, 500, 500, 510, 510]], f32)
    got = I.filter_and_offset_labels(lab, (32.5, 0.0, 96.5, 64))
    assert got.shape == (1, 5) and got.dtype == f32
    assert got[0, 1] == f32(0.0) and got[0, 2] == f32(20.7) and got[0, 3] == f32(f32(80.1) - f32(32.5)) and got[0, 4] == f32(64.0)
    none = I.filter_and_offset_labels(lab[1:], (0, 0, 64, 64))
    assert none.shape == (1, 5) and not none.any()


def test_csv_parse_skip_subset_targets_and_length():
    csvp = os.path.join(G, "dataset.csv")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        rows = I.read_label_csv(csvp, "/data")
    assert any("negative bounding box" in str(x.message) and "line 5" in str(x.message) for x in w)
    assert [os.path.basename(r[0]) for r in rows] == ["f0.png", "f1.png", "f2.png", "f3.png"]
    assert rows[0][0] == "/data/f0.png" and rows[0][1:4] == (301, 173, 0.5)
    assert rows[0][4].dtype == np.float32 and rows[0][4].shape == (4, 4) and rows[3][4].shape == (0, 4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ld = I.ImageLabelBatches(csvp, "", 64, 64, num_images=-1, bw=False, lr_flip=True, ts=True, batch_size=4)
        n = [I.n_patches(w, h, s, 64, 64) for _, w, h, s, _ in rows]
        assert n == [6, 2, 1, 2]
        assert len(ld.dataset) == 11 and len(ld) == 3 and ld.num_targets_per_image == 4
        assert ld.img_files == ["f0.png"] * 6 + ["f1.png"] * 2 + ["f2.png"] + ["f3.png"] * 2
        for k in (0, 1):                                       # random.sample of 0 or 1 keeps the whole list (len > 1 quirk)
            assert len(I.ImageLabelBatches(csvp, "", 64, 64, num_images=k, ts=True).dataset) == 11
        sub = I.ImageLabelBatches(csvp, "", 64, 64, num_images=3, ts=True, batch_size=2)
        idx = random.Random(0).sample(range(11), k=3)            # train.py seeds Python's random with 0 before its loaders
        assert sub.img_files == [ld.img_files[i] for i in idx] and len(sub) == 2
        assert sub.num_targets_per_image == max(len(ld.labels[i]) for i in idx)
        pad = I.ImageLabelBatches(csvp, "", 96, 64, ts=False, batch_size=3)
        assert len(pad.dataset) == 4 and len(pad) == 2


def test_draws_follow_the_reference_order_and_are_reproducible():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ld = I.ImageLabelBatches(os.path.join(G, "dataset.csv"), "", 64, 64, bw=False, lr_flip=True, ts=True, batch_size=4, seed=5)
    for index in range(11):
        rng = random.Random(f"5/2/{index}")
        patch = rng.randint(0, I.n_patches(*ld.sizes[index], ld.scales[index], 64, 64) - 1)
        flip = len(ld.labels[index]) > 0 and rng.random() > 0.5
        g = ld.plan(index, epoch=2)
        assert (g.patch_index, g.flip) == (patch, flip)
    assert ld.order(0) != ld.order(1) and sorted(ld.order(0)) == list(range(11))
    ld.shuffle = False
    assert ld.order(3) == list(range(11))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dbg = I.ImageLabelBatches(os.path.join(G, "dataset.csv"), "", 64, 64, lr_flip=True, ts=True, seed=5, debug_mode=True)
    for index in range(11):                     # debug_mode: patch 0, but the patch draw is still made before the flip draw
        g, d = ld.plan(index, epoch=2), dbg.plan(index, epoch=2)
        assert d.patch_index == 0 and d.flip == g.flip


def test_forced_draws_give_the_golden_targets():
    frames = _frames()
    for name in ("loader_ts.npz", "loader_pad.npz"):
        z = _npz(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ld = I.ImageLabelBatches(os.path.join(G, "dataset.csv"), "", int(z["W"]), int(z["H"]), ts=name == "loader_ts.npz",
                                     lr_flip=True, batch_size=int(z["B"]), shuffle=False,
                                     draws=lambda e, i: tuple(int(v) for v in z[f"e{e}_draws"][i]))
        assert [os.path.splitext(f)[0] for f in ld.img_files] == list(z["files"])
        for e in range(3):
            for i, f in enumerate(ld.img_files):
                g = ld.plan(i, e, frames[os.path.splitext(f)[0]].shape[1::-1])
                assert np.array_equal(g.labels.view(np.uint32), z[f"e{e}_targets"][i].view(np.uint32)), (name, e, i)


def test_unsupported_options_raise():
    csvp = os.path.join(G, "dataset.csv")
    for opt in I.UNSUPPORTED:
        with pytest.raises(ValueError, match=opt):
            I.ImageLabelBatches(csvp, "", 64, 64, ts=True, **{opt: True})
    with pytest.raises(TypeError):
        I.ImageLabelBatches(csvp, "", 64, 64, ts=True, colour=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        I.ImageLabelBatches(csvp, "", 64, 64, ts=True, ud_flip=True, augment_hsv=False, data_aug=False)   # False is accepted


def test_odd_patch_with_half_offset_is_rejected():
    # width 194 -> 3 patches of 65 with offset 0.5: patch 1 spans 64.5 .. 129.5, which Image.crop rounds to 66 columns
    with pytest.raises(ValueError, match="rounds"):
        I.sample_geometry(194, 65, 65, 65, True, 1.0, 1)
    I.sample_geometry(194, 65, 64, 64, True, 1.0, 1)
