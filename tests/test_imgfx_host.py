"""The loader's blur / noise / contrast / sharpen options, host half (no GPU): the NumPy restatement of csrc/imgfx.hip
(tests/helpers/imgfx_numpy.py) against independent references (a float64 Gaussian filter, the float64 sigmoid, exact rationals, the
normal distribution's moments), the host tables of mdcv/data/images.py against the restatement, the draw order against the reference's own
`ImageLabelDataset.__getitem__` (tests/golden/imgfx/draws.npz, written by tests/golden/make_golden_imgfx.py), and the untouched paths."""
import math
import os
import random
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imgaug_cases as K  # noqa: E402
import imgfx_numpy as N  # noqa: E402
from mdcv.data import images as I  # noqa: E402

CSV = os.path.join(K.GL, "dataset.csv")
DRAWS = os.path.join(K.GOLDEN, "imgfx", "draws.npz")
SIGMAS = [0.0011, 0.01, 0.3, 0.5, 0.77, 1.0, 1.6, 2.0, 2.5, 2.99, 3.0, 3.7, 4.2, 4.9]


def _loader(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return I.ImageLabelBatches(CSV, "", **kw)


def _image(H, W, seed):
    """random bytes with runs of 0 and 255 on the borders"""
    a = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[:3, : W // 2], a[-2:, W // 3:], a[:, :2], a[H // 2:, -3:] = 0, 255, 255, 0
    return a


# ------------------------------------------------------------------------------------------------------------------------ blur
def test_kernel_size_rule():
    assert [N.blur_ksize(s) for s in (0.0005, 0.5, 1.6, 2.99, 4.9)] == [None, 5, 5, 9, 15]
    assert [I.blur_radius(s) for s in (0.0005, 0.5, 1.6, 2.99, 4.9)] == [0, 2, 2, 4, 7]
    assert I.blur_radius(1e-3) == 0 and I.blur_radius(5.0) == 13 // 2 and I.blur_radius(4.99999) == 7
    with pytest.raises(ValueError, match="sigma"):
        I.ImageFx(blur=5.0)


def test_every_table_is_symmetric_non_negative_and_sums_to_256():
    for s in SIGMAS + [random.Random(1).uniform(0, 5) for _ in range(200)]:
        if N.blur_ksize(s) is None:
            continue
        r, q = N.blur_table(s)
        assert len(q) == 2 * r + 1 == N.blur_ksize(s) and 1 <= r <= 7
        assert (q >= 0).all() and q.sum() == 256 and np.array_equal(q, q[::-1]), (s, q)
        assert I.blur_table(s) == (r, tuple(int(v) for v in q[r:])), s              # the loader's half table, centre first


def test_blur_stays_within_the_derived_bound_of_the_float64_filter():
    """Each pass replaces w by q / 256: |sum (q/256 - w) x| <= 255 * sum |q/256 - w| per pass, the second pass's weights sum to 1 so the
    first pass's error goes through undiminished at most, and the one rounding at the end adds 0.5."""
    ndimage = pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for k, s in enumerate(s for s in SIGMAS if N.blur_ksize(s) is not None):
        r, q = N.blur_table(s)
        a = _image(40, 52, k)
        ref = ndimage.gaussian_filter1d(a.astype(np.float64), s, axis=1, radius=r, mode="mirror")
        ref = ndimage.gaussian_filter1d(ref, s, axis=0, radius=r, mode="mirror")
        bound = 0.5 + 2 * 255 * np.abs(q / 256.0 - N.gauss_weights(s, r)).sum()
        dev = np.abs(N.blur(a, s).astype(np.float64) - ref).max()
        print(f"sigma {s}: r {r}, deviation {dev:.4f}, bound {bound:.4f}")
        assert dev <= bound, (s, dev, bound)
        worst = max(worst, dev)
    print(f"largest deviation {worst:.4f}")
    assert np.array_equal(N.blur(a, 0.0005), a)                  # skipped


# -------------------------------------------------------------------------------------------------------------------- contrast
@pytest.mark.parametrize("cutoff", [0.45, 0.6, 0.75])
def test_contrast_table(cutoff):
    for gain in range(5, 11):
        v = np.linspace(0, 1, 256, dtype=np.float32)
        f32 = np.float32(255) / (np.float32(1) + np.exp(np.float32(gain) * (np.float32(cutoff) - v)))
        assert f32.dtype == np.float32
        want = np.clip(f32, 0, 255).astype(np.uint8)
        for t in (N.sigmoid_table(gain, cutoff), I.sigmoid_table(gain, cutoff)):
            assert t.dtype == np.uint8 and t.shape == (256,) and np.array_equal(t, want), (gain, cutoff)
        assert (np.diff(want.astype(np.int64)) >= 0).all()
        f64 = 255.0 / (1.0 + np.exp(float(gain) * (float(cutoff) - np.linspace(0, 1, 256))))
        assert np.abs(want.astype(np.int64) - np.floor(f64).astype(np.int64)).max() <= 1


# --------------------------------------------------------------------------------------------------------------------- sharpen
def test_sharpen_alpha_zero_is_the_identity():
    a = _image(16, 16, 3)
    assert np.array_equal(N.sharpen(a, 0.0), a)
    kc, kn = I.sharpen_coefficients(0.0)
    assert (kc, kn) == (1.0, 0.0) and kc.dtype == np.float32


@pytest.mark.parametrize("alpha", [0.37, 0.5, 0.0625, 0.123456789])
def test_sharpen_equals_the_exact_rational_rounded_half_even(alpha):
    a = _image(16, 16, 5)
    m = N.sharpen_matrix(alpha)
    assert m.dtype == np.float32 and len({float(m[i, j]) for i in range(3) for j in range(3) if (i, j) != (1, 1)}) == 1
    kc, kn = I.sharpen_coefficients(alpha)
    assert (kc, kn) == (m[1, 1], m[0, 0]) and kc.dtype == kn.dtype == np.float32
    fc, fn = Fraction(float(kc)), Fraction(float(kn))
    got = N.sharpen(a, alpha)
    for y in range(16):
        for x in range(16):
            ys = [abs(y - 1), y, y + 1 if y + 1 < 16 else 14]
            xs = [abs(x - 1), x, x + 1 if x + 1 < 16 else 14]
            for c in range(3):
                s8 = sum(int(a[yy, xx, c]) for yy in ys for xx in xs) - int(a[y, x, c])
                exact = fc * int(a[y, x, c]) + fn * s8
                assert got[y, x, c] == min(255, max(0, round(exact))), (y, x, c)     # round(Fraction) rounds half to even


# ----------------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("per_channel", [False, True])
def test_noise_has_the_moments_of_the_rounded_normal(per_channel):
    a = np.full((64, 64, 3), 128, np.uint8)
    s = 5.0
    d = N.noise(a, s, per_channel, 20261019).astype(np.int64) - 128
    assert np.array_equal(d, N.noise_values(64, 64, s, per_channel, 20261019)) and np.abs(d).max() < 127        # nothing clipped
    if per_channel:
        assert not np.array_equal(d[..., 0], d[..., 1])
        x = d.reshape(-1)
    else:
        assert np.array_equal(d[..., 0], d[..., 1]) and np.array_equal(d[..., 0], d[..., 2])
        x = d[..., 0].reshape(-1)
    n = x.size
    assert n == 64 * 64 * (3 if per_channel else 1)
    sd = math.sqrt(s * s + 1 / 12)
    print(f"per_channel {per_channel}: mean {x.mean():.5f} (limit {5 * sd / math.sqrt(n):.5f}), std {x.std():.5f} vs {sd:.5f} "
          f"(limit {5 * sd / math.sqrt(2 * n):.5f})")
    assert abs(x.mean()) < 5 * sd / math.sqrt(n)
    assert abs(x.std() - sd) < 5 * sd / math.sqrt(2 * n)


def test_noise_sum_is_the_documented_irwin_hall():
    S = N.noise_sum(99, np.arange(1 << 16))
    assert S.min() >= 0 and S.max() <= 12 * 65535
    z = (S - 393210) / 65536.0
    assert abs(z.mean()) < 5 / 256 and abs(z.std() - 1) < 5 / math.sqrt(2 * 65536)
    assert np.array_equal(N.noise(np.zeros((16, 16, 3), np.uint8), 0.0, True, 1), np.zeros((16, 16, 3), np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- loader
def _configs():
    z = np.load(DRAWS)
    for name in ("ts_plain", "ts_aug", "pad_plain", "pad_aug"):
        yield z, name


def test_golden_draw_logs_end_in_the_reference_order():
    """behind the flip the recorder logged, per op, the gate `random()` and, when it opened, the op's draws in the reference's order
    (the unused uniform(40, -40) of the blur included); the recorded imgaug arguments are those draws"""
    boxed = 0
    for z, name in _configs():
        for e in range(int(z["epochs"])):
            kinds, values, params = z[f"{name}_e{e}_kinds"], z[f"{name}_e{e}_values"], z[f"{name}_e{e}_params"]
            for i in range(len(kinds)):
                n = int((kinds[i] >= 0).sum())
                p = params[i]
                if n <= 1:                                       # a box-free sample: the patch draw at most
                    assert not p.any() and (n == 0 or kinds[i, 0] == 2)
                    continue
                boxed += 1
                want_k, want_v = [], []
                for on, gate, draws in ((p[0], 0.2, [(1, None), (1, p[1])]), (p[2], 0.3, [(1, p[3])]), (p[4], 0.5, [(1, p[6]), (2, p[5])]),
                                        (p[7], 0.3, [(1, p[8])])):
                    want_k.append(0)
                    want_v.append(("gate", gate, bool(on)))
                    for k, v in (draws if on else []):
                        want_k.append(k)
                        want_v.append(v)
                tail_k, tail_v = kinds[i, n - len(want_k):n], values[i, n - len(want_k):n]
                assert list(tail_k) == want_k, (name, e, i)
                assert kinds[i, n - len(want_k) - 1] == 0                                   # the flip draw
                for got, want in zip(tail_v, want_v):
                    if isinstance(want, tuple):
                        assert (got > want[1]) == want[2]
                    elif want is None:
                        assert -40 <= got <= 40
                    else:
                        assert got == want
    assert boxed > 50


@pytest.mark.parametrize("name", ["ts_plain", "ts_aug", "pad_plain", "pad_aug"])
def test_plan_reproduces_the_reference_gates_and_parameters(name):
    z = np.load(DRAWS)
    W, H = (int(v) for v in z[f"{name}_size"])
    ld = _loader(width=W, height=H, ts=name.startswith("ts"), lr_flip=True, shuffle=False, seed=int(z["seed"]), data_aug=name.endswith("aug"),
                 blur=True, noise=True, contrast=True, sharpen=True)
    assert [os.path.basename(f) for f in ld.img_files] == list(z[f"{name}_files"])
    seen, closed_blur = set(), 0
    for e in range(int(z["epochs"])):
        for i in range(len(ld.img_files)):
            want = z[f"{name}_e{e}_params"][i]
            g = ld.plan(i, e)
            fx = g.fx
            closed_blur += int(len(ld.labels[i]) > 0 and want[0] == 0)
            if not want[[0, 2, 4, 7]].any():
                assert fx is None, (e, i)
                seen.add("none" if len(ld.labels[i]) else "box-free")
                continue
            assert (fx.blur is not None, fx.noise is not None, fx.contrast is not None, fx.sharpen is not None) == tuple(want[[0, 2, 4, 7]] > 0)
            if fx.blur is not None:
                assert fx.blur == want[1]
            if fx.noise is not None:
                r2 = random.Random(f"{int(z['seed'])}/{e}/{i}/imgaug")
                assert fx.noise == (want[3], r2.random() < 0.5, r2.getrandbits(32))
            if fx.contrast is not None:
                assert fx.contrast == (int(want[5]), want[6])
            if fx.sharpen is not None:
                assert fx.sharpen == want[8]
            seen.add((fx.blur is not None, fx.noise is not None))
            # the flip is the draw in front of the blur gate: the log's last random() before the recorded parameters
            kinds, values = z[f"{name}_e{e}_kinds"][i], z[f"{name}_e{e}_values"][i]
            n_fx = 3 * int(want[0]) + 2 * int(want[2]) + 3 * int(want[4]) + 2 * int(want[7]) + int((want[[0, 2, 4, 7]] == 0).sum())
            flip_at = int((kinds >= 0).sum()) - n_fx - 1
            assert kinds[flip_at] == 0 and g.flip == (values[flip_at] > 0.5), (e, i)
    assert closed_blur > 0 and "box-free" in seen                # a closed blur gate: the discarded uniform(40, -40) is then not drawn


def test_salt_warns_and_changes_nothing():
    with pytest.warns(UserWarning, match="salt"):
        salted = I.ImageLabelBatches(CSV, "", 64, 64, ts=True, lr_flip=True, seed=3, salt=True)
    plain = _loader(width=64, height=64, ts=True, lr_flip=True, seed=3)
    for i in range(len(plain.img_files)):
        a, b = salted.plan(i, 0), plain.plan(i, 0)
        assert a.desc == b.desc and a.flip == b.flip and a.fx is None and a.aug is None and np.array_equal(a.labels, b.labels)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        I.ImageLabelBatches(CSV, "", 64, 64, ts=True, salt=False, blur=False, noise=False, contrast=False, sharpen=False)
    assert not any("salt" in str(w.message) for w in caught)


@pytest.mark.parametrize("opt", ["blur", "noise", "contrast", "sharpen"])
def test_bw_with_an_imgaug_option_raises(opt):
    with pytest.raises(ValueError, match="bw"):
        _loader(width=64, height=64, ts=True, bw=True, **{opt: True})
    _loader(width=64, height=64, ts=True, bw=False, **{opt: True})
    _loader(width=64, height=64, ts=True, bw=True, **{opt: False})


@pytest.mark.parametrize("name", ["loader_ts.npz", "loader_pad.npz"])
def test_options_off_leave_draws_descriptors_and_layout_as_they_were(name):
    """tests/golden/imgaug's loader fixtures were drawn before the options existed: with the four off the plan is still theirs (patch,
    augmentation and flip, so not one more draw in front of the flip), no sample carries `fx`, and the staging layout has no fx region"""
    z = K.npz(name)
    W, H = int(z["W"]), int(z["H"])
    ld = _loader(width=W, height=H, ts=name == "loader_ts.npz", lr_flip=True, batch_size=int(z["B"]), shuffle=False, seed=int(z["seed"]),
                 data_aug=True, blur=False, noise=False, contrast=False, sharpen=False)
    frs = K.frames()
    for e in range(3):
        geoms, wins = [], []
        for i, f in enumerate(ld.img_files):
            fr = frs[os.path.splitext(f)[0]]
            g = ld.plan(i, e, fr.shape[1::-1])
            assert (g.patch_index, int(g.flip)) == tuple(int(v) for v in z[f"e{e}_draws"][i]) and g.fx is None
            assert ((g.aug.jitter, g.aug.affine) if g.aug else (None, None)) == K.unpack_aug(z[f"e{e}_aug"][i])
            geoms.append(g)
            wins.append(I.crop_window(fr, g))
        p = I.pack_layout(geoms, [w.nbytes for w in wins], ld.num_targets_per_image)
        assert not p.fx and not hasattr(p, "fx_off") and p.aug
        assert p.nbytes == I._align(p.aug_off + len(geoms) * I.AUG_DESC * 4)
        a = np.zeros(p.nbytes, np.uint8)
        I.pack_batch(a, p, geoms, wins, [g.labels for g in geoms])
        for g in geoms:
            del g.fx                                             # geometries as they were before the options existed
        q = I.pack_layout(geoms, [w.nbytes for w in wins], ld.num_targets_per_image)
        b = np.zeros(q.nbytes, np.uint8)
        I.pack_batch(b, q, geoms, wins, [g.labels for g in geoms])
        assert p.nbytes == q.nbytes and np.array_equal(a, b)


def test_fx_descriptors_and_tables_ride_behind_everything_else():
    ld = _loader(width=64, height=64, ts=True, lr_flip=True, shuffle=False, seed=7, blur=True, noise=True, contrast=True, sharpen=True,
                 draws=lambda e, i: (0, i % 2, None, dict(blur=0.5 + i, noise=(2.5, i % 2, 2 ** 32 - 1 - i), contrast=(5 + i % 6, 0.5),
                                                          sharpen=0.25) if i % 3 else (dict(sharpen=0.5) if i else None)))
    frs = K.frames()
    n = 5
    geoms = [ld.plan(i, 0) for i in range(n)]
    assert geoms[0].fx is None and geoms[3].fx.blur is None and geoms[1].fx.blur == 1.5
    wins = [I.crop_window(frs[os.path.splitext(os.path.basename(g.uri))[0]], g) for g in geoms]
    p = I.pack_layout(geoms, [w.nbytes for w in wins], 0)
    assert p.fx and not p.aug and p.fx_off == I._align(p.pix_off + p.src_bytes) and p.n_luts == 3
    assert p.lut_off == I._align(p.fx_off + n * I.FX_DESC * 4) and p.nbytes == I._align(p.lut_off + 3 * 256)
    buf = np.zeros(p.nbytes, np.uint8)
    I.pack_batch(buf, p, geoms, wins)
    d = buf[p.fx_off:p.fx_off + n * I.FX_DESC * 4].view(np.int32).reshape(n, I.FX_DESC)
    luts = buf[p.lut_off:p.lut_off + 3 * 256].reshape(3, 256)
    k = 0
    for row, g in zip(d, geoms):
        fx = g.fx
        assert (row[20:] == 0).all() and row[2] + 2 * row[3:10].sum() == 256 and 1 <= row[1] <= 7
        if fx is None:
            assert list(row[[0, 10, 15, 17]]) == [0, 0, 0, 0]
            continue
        assert list(row[[0, 10, 15, 17]]) == [int(v is not None) for v in (fx.blur, fx.noise, fx.contrast, fx.sharpen)]
        if fx.blur is not None:
            r, q = N.blur_table(fx.blur)
            assert row[1] == r and list(row[2:3 + r]) == list(q[r:]) and (row[3 + r:10] == 0).all()
        if fx.noise is not None:
            assert row[11] == int(fx.noise[1]) and int(row[12:13].view(np.uint32)[0]) == fx.noise[2] and row[13:15].view(np.float64)[0] == 2.5
        if fx.contrast is not None:
            assert row[16] == k and np.array_equal(luts[k], N.sigmoid_table(*fx.contrast))
            k += 1
        if fx.sharpen is not None:
            m = N.sharpen_matrix(fx.sharpen)
            assert tuple(row[18:20].view(np.float32)) == (m[1, 1], m[0, 0])
    assert k == 3
    with pytest.raises(ValueError, match="sigma"):
        _loader(width=64, height=64, ts=True, blur=True, draws=lambda e, i: (0, 0, None, dict(blur=5.5))).plan(0, 0)
    # shorter tuples keep working, and leave the drawn fx in place
    short = _loader(width=64, height=64, ts=True, lr_flip=True, seed=7, blur=True, sharpen=True, draws=lambda e, i: (0, 1))
    drawn = _loader(width=64, height=64, ts=True, lr_flip=True, seed=7, blur=True, sharpen=True)
    for i in range(4):
        a, b = short.plan(i, 0), drawn.plan(i, 0)
        assert (a.fx is None) == (b.fx is None) and (a.fx is None or (a.fx.blur, a.fx.sharpen) == (b.fx.blur, b.fx.sharpen))
