"""Augmented real-image loader, host half (no GPU): the NumPy restatement of Pillow's blend / HSV / affine arithmetic against the golden
images and against Pillow itself (both colour conversions on all 2^24 inputs), the draw order, the boxes against the reference's
`affine_labels`, and the untouched path.  Golden data: tests/golden/imgaug (tests/golden/make_golden_imgaug.py: Pillow 12.2 and the
reference's own label code)."""
import json
import os
import random
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imgaug_cases as K  # noqa: E402
import imgaug_numpy as N  # noqa: E402
from mdcv.data import images as I  # noqa: E402

CSV = os.path.join(K.GL, "dataset.csv")
# Box tolerance, in pixels before the division by W / H.  The reference's float32 affine_labels sits at most 8.9e-5 px from a float64
# evaluation (2000 random 416x416 cases); twice that covers a torch build that sums the 3-term products of its matmuls in another order.
BOX_TOL_PX = 2e-4


def _boxes():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows = I.read_label_csv(CSV, "")
    return {os.path.splitext(os.path.basename(r[0]))[0]: r[4] for r in rows}


def _loader(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return I.ImageLabelBatches(CSV, "", **kw)


def _all_rgb():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_fixture_provenance():
    meta = json.load(open(os.path.join(K.G, "meta.json")))
    assert meta["pillow"] == "12.2.0" and "torch" in meta and "numpy" in meta


def test_numpy_restatement_equals_the_golden_images():
    cs, _ = K.cases()
    kinds = set()
    for c in cs:
        jit, aff = (None, None) if c["empty"] else (c["jitter"], c["affine"])
        m = N.inverse_affine_matrix(c["W"], c["H"], *aff) if aff else None
        got = N.augment(c["patch_u8"], jit, m, c["bw"] and not c["empty"], c["flip"] and not c["empty"])
        assert got.shape == c["u8"].shape and int((got != c["u8"]).sum()) == 0, (c["i"], int((got != c["u8"]).sum()))
        kinds.add((jit is not None, aff is not None))
        if jit:
            kinds.add(("contrast at", jit[0].index(N.CONTRAST)))
    assert {(True, False), (False, True), (True, True), (False, False)} <= kinds
    assert {("contrast at", 0), ("contrast at", 3)} <= kinds and kinds & {("contrast at", 1), ("contrast at", 2)}


def test_matrix_equals_the_helper_and_identity_for_no_motion():
    m = I.inverse_affine_matrix(96, 64, 7.3, (12.5, -20.25), 1.05, 2.0)
    assert m == N.inverse_affine_matrix(96, 64, 7.3, (12.5, -20.25), 1.05, 2.0)
    assert np.allclose(I.inverse_affine_matrix(64, 64, 0.0, (0.0, 0.0), 1.0, 0.0), [1, 0, 0, 0, 1, 0], atol=1e-12)


def test_rgb_to_hsv_equals_pillow_on_every_rgb_value():
    Image = pytest.importorskip("PIL.Image")
    a = _all_rgb()
    want = np.asarray(Image.fromarray(a, "RGB").convert("HSV"))
    got = N.rgb_to_hsv(a)
    assert int((got != want).sum()) == 0


def test_hsv_to_rgb_equals_pillow_on_every_hsv_value():
    Image = pytest.importorskip("PIL.Image")
    a = _all_rgb()
    want = np.asarray(Image.fromarray(a, "HSV").convert("RGB"))
    got = N.hsv_to_rgb(a)
    assert int((got != want).sum()) == 0


def test_blends_equal_pillow_over_the_factor_range():
    pytest.importorskip("PIL.Image")
    from PIL import Image, ImageEnhance
    rng = np.random.default_rng(3)
    factors = [0.75, 0.8, 0.9, 0.97, 0.999999, 1.0, 1.000001, 1.03, 1.1, 1.2, 1.25] + [random.Random(5).uniform(0.75, 1.25) for _ in range(6)]
    for k, f in enumerate(factors):
        a = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
        if k % 3 == 0:
            a[:24] = a[:24] // 8 + (0 if k % 2 else 224)         # dark / bright halves: both clip branches of the blend
        im = Image.fromarray(a, "RGB")
        assert np.array_equal(N.brightness(a, f), np.asarray(ImageEnhance.Brightness(im).enhance(f))), f
        assert np.array_equal(N.contrast(a, f), np.asarray(ImageEnhance.Contrast(im).enhance(f))), f
        assert np.array_equal(N.saturation(a, f), np.asarray(ImageEnhance.Color(im).enhance(f))), f


def test_affine_equals_pillow_on_random_transforms():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    for t in range(12):
        W, H = ((96, 64), (123, 77), (64, 128))[t % 3]
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        r = random.Random(t)
        m = N.inverse_affine_matrix(W, H, r.uniform(-10, 10), (r.uniform(-40, 40), r.uniform(-40, 40)), r.uniform(.9, 1.1), r.uniform(-3, 3))
        want = np.asarray(Image.fromarray(a).transform((W, H), Image.AFFINE, m, Image.BILINEAR, fillcolor=(127, 127, 127)))
        assert np.array_equal(N.affine(a, m), want), t


def test_hue_shift_truncates_toward_zero_and_wraps():
    assert [I.hue_shift(h) for h in (0.04, 0.0039, 0.0, -0.0039, -0.004, -0.04)] == [10, 0, 0, 0, 255, 246]
    assert all(I.hue_shift(h) == N.hue_shift(h) for h in np.linspace(-0.04, 0.04, 101))


@pytest.mark.parametrize("opts", [dict(data_aug=True), dict(augment_hsv=True), dict(augment_affine=True),
                                  dict(augment_hsv=True, augment_affine=True)])
def test_draws_follow_the_reference_order(opts):
    ld = _loader(width=64, height=64, lr_flip=True, ts=True, batch_size=4, seed=11, **opts)
    jit_on = opts.get("data_aug") or opts.get("augment_hsv")
    aff_on = opts.get("data_aug") or opts.get("augment_affine")
    seen = set()
    for epoch in (0, 3):
        for index in range(len(ld.img_files)):
            rng = random.Random(f"11/{epoch}/{index}")
            patch = rng.randint(0, I.n_patches(*ld.sizes[index], ld.scales[index], 64, 64) - 1)
            jitter = affine = None
            flip = False
            if len(ld.labels[index]) > 0:
                if jit_on and rng.random() > 0.5:
                    b, c, s = rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25), rng.uniform(0.75, 1.25)
                    h = rng.uniform(-0.04, 0.04)
                    order = [0, 1, 2, 3]
                    rng.shuffle(order)
                    jitter = (tuple(order), (b, c, s), h)
                if aff_on and rng.random() > 0:
                    angle = rng.uniform(-10, 10)
                    tr = (rng.uniform(-40, 40), rng.uniform(-40, 40))
                    affine = (angle, tr, rng.uniform(0.9, 1.1), rng.uniform(-3, 3))
                flip = rng.random() > 0.5
            g = ld.plan(index, epoch)
            assert (g.patch_index, g.flip) == (patch, flip)
            if jitter is None and affine is None:
                assert g.aug is None
            else:
                assert g.aug.jitter == jitter and g.aug.affine == affine
                if affine:
                    assert g.aug.matrix == N.inverse_affine_matrix(64, 64, *affine)
                if jitter:
                    assert g.aug.hue_shift == int(jitter[2] * 255) % 256
            seen.add((len(ld.labels[index]) > 0, jitter is not None, affine is not None))
    assert (False, False, False) in seen and (True, bool(jit_on), bool(aff_on)) in seen


def _check_boxes(got, want, changed, W, H, what):
    """the rows affine_labels replaced must be the same rows; coordinates within BOX_TOL_PX (divided by W / H like the boxes)"""
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(got[:, 0], want[:, 0]), what
    tol = BOX_TOL_PX * np.array([1 / W, 1 / H, 1 / W, 1 / H])
    err = np.abs(got[:, 1:].astype(np.float64) - want[:, 1:])
    assert (err <= tol).all(), (what, err.max())
    return err.max()


def test_case_boxes_equal_affine_labels_of_the_reference():
    cs, T = K.cases()
    boxes, frs = _boxes(), K.frames()
    changed_rows = 0
    for c in cs:
        g = K.geometry(I, c, frs)
        got = I.sample_labels(boxes[c["name"]], g, T, g.aug)
        plain = I.sample_labels(boxes[c["name"]], g, T)
        _check_boxes(got, c["labels"], c["changed"], c["W"], c["H"], c["i"])
        moved = (got != plain).any(1)                            # the rows this implementation replaced
        assert np.array_equal(moved, c["changed"]), (c["i"], moved, c["changed"])
        changed_rows += int(moved.sum())
    assert changed_rows >= 8


@pytest.mark.parametrize("name", ["loader_ts.npz", "loader_pad.npz"])
def test_plan_reproduces_the_golden_draws_and_boxes(name):
    z = K.npz(name)
    W, H = int(z["W"]), int(z["H"])
    ld = _loader(width=W, height=H, ts=name == "loader_ts.npz", lr_flip=True, batch_size=int(z["B"]), shuffle=False,
                 seed=int(z["seed"]), data_aug=True)
    off = _loader(width=W, height=H, ts=name == "loader_ts.npz", lr_flip=True, batch_size=int(z["B"]), shuffle=False,
                  draws=lambda e, i: tuple(int(v) for v in z[f"e{e}_draws"][i]))
    assert [os.path.splitext(f)[0] for f in ld.img_files] == list(z["files"])
    frs = K.frames()
    n_changed = 0
    for e in range(3):
        for i, f in enumerate(ld.img_files):
            size = frs[os.path.splitext(f)[0]].shape[1::-1]
            g = ld.plan(i, e, size)
            assert (g.patch_index, int(g.flip)) == tuple(int(v) for v in z[f"e{e}_draws"][i]), (e, i)
            jitter, affine = K.unpack_aug(z[f"e{e}_aug"][i])
            assert (g.aug.jitter if g.aug else None) == jitter and (g.aug.affine if g.aug else None) == affine, (e, i)
            _check_boxes(g.labels, z[f"e{e}_targets"][i], z[f"e{e}_changed"][i], W, H, (name, e, i))
            moved = (g.labels != off.plan(i, e, size).labels).any(1)
            assert np.array_equal(moved, z[f"e{e}_changed"][i]), (name, e, i)
            n_changed += int(moved.sum())
    assert n_changed > 10


def test_options_off_leave_plan_and_staging_buffer_as_they_were():
    """no option: no `aug`, the golden targets of tests/golden/imgload bit for bit, and a staging buffer without an augmentation region
    that equals the one packed from bare geometries (the layout of the two-launch path)"""
    frs = K.frames()
    z = np.load(os.path.join(K.GL, "loader_ts.npz"))
    draws = lambda e, i: tuple(int(v) for v in z[f"e{e}_draws"][i])          # noqa: E731
    ld = _loader(width=64, height=64, ts=True, lr_flip=True, batch_size=4, shuffle=False, draws=draws,
                 augment_hsv=False, augment_affine=False, data_aug=False)
    geoms, wins, bare = [], [], []
    for i, f in enumerate(ld.img_files):
        fr = frs[os.path.splitext(f)[0]]
        g = ld.plan(i, 1, fr.shape[1::-1])
        assert g.aug is None
        assert np.array_equal(g.labels.view(np.uint32), z["e1_targets"][i].view(np.uint32))
        geoms.append(g)
        wins.append(I.crop_window(fr, g))
        bare.append(I.sample_geometry(fr.shape[1], fr.shape[0], 64, 64, True, ld.scales[i], g.patch_index, g.flip))
    p = I.pack_layout(geoms, [w.nbytes for w in wins], ld.num_targets_per_image)
    q = I.pack_layout(bare, [w.nbytes for w in wins], ld.num_targets_per_image)
    assert not p.aug and not hasattr(p, "aug_off")
    assert (p.desc_off, p.lab_off, p.coef_off, p.pix_off, p.nbytes) == (q.desc_off, q.lab_off, q.coef_off, q.pix_off, q.nbytes)
    assert p.nbytes == I._align(p.pix_off + p.src_bytes)
    a, b = np.zeros(p.nbytes, np.uint8), np.zeros(q.nbytes, np.uint8)
    I.pack_batch(a, p, geoms, wins, [g.labels for g in geoms])
    I.pack_batch(b, q, bare, wins, [g.labels for g in geoms])
    assert np.array_equal(a, b)
    # seeds without options: not one extra draw (the flip is the second draw of a boxed sample)
    plain = _loader(width=64, height=64, ts=True, lr_flip=True, seed=5)
    for i in range(len(plain.img_files)):
        rng = random.Random(f"5/0/{i}")
        patch = rng.randint(0, I.n_patches(*plain.sizes[i], plain.scales[i], 64, 64) - 1)
        flip = len(plain.labels[i]) > 0 and rng.random() > 0.5
        g = plain.plan(i, 0)
        assert (g.patch_index, g.flip, g.aug) == (patch, flip, None)


def test_augmented_batch_carries_its_descriptors_behind_the_pixels():
    cs, _ = K.cases()
    frs = K.frames()
    cs = [c for c in cs if (c["W"], c["H"]) == (64, 64) and not c["bw"]]
    geoms = [K.geometry(I, c, frs) for c in cs]
    wins = [I.crop_window(frs[c["name"]], g) for c, g in zip(cs, geoms)]
    p = I.pack_layout(geoms, [w.nbytes for w in wins], 0)
    assert p.aug and p.aug_off == I._align(p.pix_off + p.src_bytes) and p.nbytes == I._align(p.aug_off + len(cs) * I.AUG_DESC * 4)
    buf = np.zeros(p.nbytes, np.uint8)
    I.pack_batch(buf, p, geoms, wins)
    d = buf[p.aug_off:p.aug_off + len(cs) * I.AUG_DESC * 4].view(np.int32).reshape(len(cs), I.AUG_DESC)
    for row, c, g in zip(d, cs, geoms):
        assert row[12] == int(g.aug is not None and g.aug.jitter is not None) and row[21] == int(g.aug is not None and g.aug.affine is not None)
        assert sorted(row[13:17]) == [0, 1, 2, 3] and row[22] == row[23] == 0
        m = row[0:12].view(np.float64)
        if row[21]:
            assert list(m) == N.inverse_affine_matrix(64, 64, *c["affine"])
        else:
            assert list(m) == [1, 0, 0, 0, 1, 0]
        if row[12]:
            assert tuple(row[13:17]) == c["jitter"][0] and row[20] == N.hue_shift(c["jitter"][2])
            assert np.array_equal(row[17:20].view(np.float32), np.array(c["jitter"][1], np.float32))
    with pytest.raises(ValueError, match="permutation"):
        I.Augmentation(((0, 1, 2, 2), (1, 1, 1), 0.0), None)
