"""Key-point augmentation, host half (no GPU): the entry's argument check through the built libmdcv_kptaug.so, the draws of
`KeypointAugBatches`, properties of the NumPy restatement of csrc/kptaug.hip (tests/kptaug_ref.py), the loop's default."""
import inspect
import math
import re
import subprocess

import numpy as np
import pytest

import kptaug_ref as R
from mdcv import _lib
from mdcv.data import kptaug as KA

F = np.float32
ARGS = ["desc_host", "desc", "B", "C", "S", "K", "imgs", "hm", "pts", "imgs_out", "hm_out", "pts_out", "stats", "stream"]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ header and library
def test_the_header_declares_the_entry_and_the_library_exports_it():
    protos = _lib.parse_header(_lib.KPTAUG_HEADER)
    assert list(protos) == ["mdcv_kptaug_batch"] and protos["mdcv_kptaug_batch"][2] == ARGS
    assert "mdcv_kptaug_batch" not in _lib.parse_header() and "mdcv_kptaug_batch" not in _lib.parse_header(_lib.AUG_HEADER)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.KPTAUG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(protos)                 # the library exports exactly its header
    K = _lib.kptaug_lib()
    assert K is _lib.kptaug_lib() and K is not _lib.aug_lib() and K is not _lib.lib() and callable(K.kptaug_batch)
    assert KA.DESC == R.DESC == 24 and KA.PERM == R.PERM


# ------------------------------------------------------------------------------------------------------------ the argument check
class _Call:
    """a call of the entry whose every argument is good, over host arrays standing in for the device buffers (a bad argument returns
    before anything is dereferenced but desc_host)"""

    def __init__(self, B=3, C=3, S=16):
        self.kw = dict(B=B, C=C, S=S, K=7, stream=None)
        self.desc_host = np.stack([R.row()] * B)
        self.buf = {"desc": np.zeros((B, 24), np.int32), "imgs": np.zeros((B, C, S, S), F), "hm": np.zeros((B, 7, S, S), F),
                    "pts": np.zeros((B, 7, 2), F), "imgs_out": np.zeros((B, C, S, S), F), "hm_out": np.zeros((B, 7, S, S), F),
                    "pts_out": np.zeros((B, 7, 2), F), "stats": np.zeros(4, np.int32)}

    def __call__(self, **over):
        a = dict(self.kw, desc_host=self.desc_host.ctypes.data, **{k: v.ctypes.data for k, v in self.buf.items()})
        a.update(over)
        return _lib.kptaug_lib().kptaug_batch(*[a[k] for k in ARGS])


def test_every_bad_argument_is_reported_without_a_gpu():
    c = _Call()
    for name in ("desc_host", "desc", "imgs", "hm", "pts", "imgs_out", "hm_out", "pts_out", "stats"):
        assert c(**{name: None}) == -1, name
    assert c(B=0) == -1 and c(B=-2) == -1 and c(B=65536) == -1
    assert c(C=0) == -1 and c(C=4) == -1 and c(C=-1) == -1
    assert c(S=15) == -1 and c(S=257) == -1 and c(S=0) == -1 and c(S=-16) == -1
    assert c(K=6) == -1 and c(K=8) == -1 and c(K=0) == -1
    # an output overlapping its input: the same buffer, and one word into its end; an output overlapping another input or output
    for o, i in (("imgs_out", "imgs"), ("hm_out", "hm"), ("pts_out", "pts")):
        assert c(**{o: c.buf[i].ctypes.data}) == -1, o
        assert c(**{o: c.buf[i].ctypes.data + c.buf[i].nbytes - 4}) == -1, o
        assert c(**{i: c.buf[o].ctypes.data + c.buf[o].nbytes - 4}) == -1, o
    assert c(imgs_out=c.buf["hm"].ctypes.data) == -1 and c(hm_out=c.buf["imgs_out"].ctypes.data) == -1
    assert c(pts_out=c.buf["stats"].ctypes.data) == -1


BAD_WORDS = [(0, 4), (0, -1), (0, 1 << 30), (19, 1), (23, -7)] + \
            [(w, v) for w in (1, 6, 7, 12, 13, 15, 16, 18) for v in (0x7FC00000, 0x7F800000, -8388608)]      # NaN, +Inf, -Inf (0xFF800000)


@pytest.mark.parametrize("word,value", BAD_WORDS)
def test_a_bad_host_descriptor_row_is_reported(word, value):
    c = _Call()
    for apply in (1, 0):                                          # the check holds for a pass-through row as well
        c.desc_host[:] = R.row(apply=apply)
        c.desc_host[2, word] = value
        assert not R.row_ok(c.desc_host[2])
        assert c() == -1


def test_the_restatement_accepts_what_the_entry_documents():
    assert R.row_ok(R.row()) and R.row_ok(R.row(apply=0, swap=1)) and R.row_ok(R.row(I=(-1e30, 3, 2, 1, 0, 1e-40), gain=(-2, 0, 5)))
    for flags in (0, 1, 2, 3):
        assert R.row_ok(R.row(flags=flags))


# ------------------------------------------------------------------------------------------------------------ the draws
def test_the_draws_are_a_function_of_seed_epoch_and_batch():
    a = KA.draw_rows(5, 2, 7, 16, 80)
    assert a.dtype == np.int32 and a.shape == (16, 24)
    assert np.array_equal(a, KA.draw_rows(5, 2, 7, 16, 80))
    for other in ((6, 2, 7), (5, 3, 7), (5, 2, 8)):
        assert not np.array_equal(a, KA.draw_rows(*other, 16, 80))
    assert all(R.row_ok(r) for r in a) and (a[:, 0] & 1).all()


def test_p_changes_bit_0_and_nothing_else():
    """every image consumes the same draws whether or not it is applied: the rows under another p differ in the apply bit alone"""
    full, some, none = (KA.draw_rows(3, 1, 4, 64, 80, p=p) for p in (1.0, 0.4, 0.0))
    assert np.array_equal(full[:, 1:], some[:, 1:]) and np.array_equal(full[:, 1:], none[:, 1:])
    assert np.array_equal(full[:, 0] & ~1, some[:, 0] & ~1) and not (none[:, 0] & 1).any()
    assert 10 < int((some[:, 0] & 1).sum()) < 45
    a, b = KA.draw_params(3, 1, 4, 64, 80, p=1.0), KA.draw_params(3, 1, 4, 64, 80, p=0.4)
    assert all({k: v for k, v in x.items() if k != "apply"} == {k: v for k, v in y.items() if k != "apply"} for x, y in zip(a, b))


def test_the_two_maps_are_inverses_in_float64_and_the_words_their_float32():
    for S in (16, 18, 80, 256):
        for i, kw in enumerate(KA.draw_params(11, 1, S, 24, S, degrees=180.0, scale=(0.5, 2.0), translate=0.3)):
            Fm, Im = KA.affine_maps(S, kw["degrees"], kw["scale"], kw["tx"], kw["ty"], kw["flip"])
            h = lambda m: np.vstack([m, [0.0, 0.0, 1.0]])
            assert np.abs(h(Fm) @ h(Im) - np.eye(3)).max() < 1e-9 and np.abs(h(Im) @ h(Fm) - np.eye(3)).max() < 1e-9
            d = KA.descriptor(S, **kw)
            assert np.array_equal(u32(d[1:7]), u32(Im.ravel().astype(F))) and np.array_equal(u32(d[7:13]), u32(Fm.ravel().astype(F)))
            assert np.array_equal(u32(d[13:16]), u32(np.array(kw["gain"]).astype(F))) and np.array_equal(u32(d[16:19]), u32(np.array(kw["bias"]).astype(F)))
            assert not d[19:].any() and bool(d[0] & 2) == kw["flip"] and bool(d[0] & 1) == kw["apply"]
            # the composition: the centre goes to the centre plus the shift, and the flip mirrors x before the rotation
            c = (S - 1) / 2
            assert np.allclose(Fm @ [c, c, 1], [c + kw["tx"], c + kw["ty"]], atol=1e-9)
            assert np.sign(np.linalg.det(Fm[:, :2])) == (-1 if kw["flip"] else 1)
            assert math.isclose(abs(np.linalg.det(Fm[:, :2])), kw["scale"] ** 2, rel_tol=1e-12)


def test_a_flip_sets_swap_and_the_colour_rule():
    rows = KA.draw_rows(0, 1, 0, 200, 80, flip=1.0)
    assert (rows[:, 0] & 2).all() and not (KA.draw_rows(0, 1, 0, 200, 80, flip=0.0)[:, 0] & 2).any()
    frac = np.mean([(r[0] & 2) != 0 for r in KA.draw_rows(1, 1, 0, 400, 80)])
    assert 0.4 < frac < 0.6
    Fm, Im = KA.affine_maps(80, flip=True)
    assert np.allclose(Fm, [[-1, 0, 79], [0, 1, 0]], atol=1e-12) and np.allclose(Im, Fm, atol=1e-12)
    # gain_c = contrast * brightness * tint_c, bias_c = 0.5 * (1 - contrast): without brightness and tint the gain IS the contrast
    for kw in KA.draw_params(2, 1, 0, 50, 80, brightness=0.0, tint=0.0, contrast=0.3):
        ct = kw["gain"][0]
        assert 0.7 <= ct <= 1.3 and kw["gain"] == (ct, ct, ct) and kw["bias"] == (0.5 * (1.0 - ct),) * 3
    for kw in KA.draw_params(2, 1, 0, 50, 80, degrees=0.0, scale=(1.0, 1.0), translate=0.0, flip=0.0, brightness=0.0, contrast=0.0, tint=0.0):
        d = KA.descriptor(80, **kw)                                                   # nothing to draw from: the identity row (zeros of either sign)
        assert d[0] == 1 and np.array_equal(d[1:19].view(F), R.row()[1:19].view(F)) and not d[19:].any()


def test_the_wrapper_forwards_and_validates():
    class Loader(list):
        dataset = range(12)
        closed = False

        def close(self):
            self.closed = True
    ld = Loader([1, 2, 3])
    m = KA.KeypointAugBatches(ld, draws=lambda e, i, B: [R.row()] * B)
    assert len(m) == 3 and m.dataset is ld.dataset and m.active
    m.close()
    assert ld.closed
    m.active = False
    assert list(m) == [1, 2, 3] and m.epoch == 0                                  # handed through untouched, no epoch of draws consumed
    assert m.rows(1, 0, 2, 80).dtype == np.int32 and m.rows(1, 0, 2, 80).shape == (2, 24)
    with pytest.raises(ValueError):
        KA.KeypointAugBatches(ld, draws=lambda e, i, B: [[0] * 23] * B).rows(1, 0, 3, 80)
    for bad in (dict(p=1.5), dict(flip=-0.1), dict(scale=(1.2, 0.8)), dict(scale=(0.0, 1.0)), dict(degrees=-1.0), dict(translate=2.0),
                dict(brightness=1.0), dict(contrast=-0.2), dict(tint=1.5)):
        with pytest.raises(ValueError):
            KA.KeypointAugBatches(ld, **bad)
    assert m.stats() == dict(augmented=0, rejected=0, passed=0, errors=0, images=0)          # nothing launched: no device touched
    assert "augmentation off" in m.summary_line("train", 1)
    from mdcv.data import KeypointAugBatches
    assert KeypointAugBatches is KA.KeypointAugBatches
    sig = inspect.signature(KeypointAugBatches).parameters
    assert {k: v.default for k, v in sig.items() if k != "loader"} == dict(
        p=1.0, seed=0, degrees=15.0, scale=(0.85, 1.15), translate=0.08, flip=0.5, brightness=0.2, contrast=0.2, tint=0.05, draws=None)


def test_the_training_loop_defaults_to_off():
    from mdcv.rektnet.train import train_model
    assert inspect.signature(train_model).parameters["augment"].default is None


# ------------------------------------------------------------------------------------------------------------ the restatement
def _case(seed, B=3, C=3, S=18):
    g = np.random.default_rng(seed)
    imgs = g.random((B, C, S, S), dtype=F)
    hm = g.random((B, 7, S, S), dtype=F)
    pts = (g.integers(1, S - 1, (B, 7, 2)) / S).astype(F)
    return imgs, hm, pts


def test_the_identity_row_returns_the_input_pixels_and_points_as_bits():
    imgs, hm, pts = _case(1)
    pts[0, 3] = [1.0, 0.0]                                                        # a label of exactly 1.0 survives the identity
    oi, oh, op, stats = R.kptaug([R.row()] * 3, imgs, hm, pts)
    assert stats.tolist() == [3, 0, 0, 0]
    assert np.array_equal(u32(oi), u32(imgs)) and np.array_equal(u32(op), u32((pts * F(18)) / F(18)))
    # the maps are regenerated: each sums to 1, peaks at the point's pixel, and is not the input's
    assert not np.array_equal(oh, hm) and np.allclose(oh.sum((2, 3)), 1.0, atol=1e-6) and np.isfinite(oh).all()
    for b in range(3):
        for k in range(7):
            y, x = np.unravel_index(np.argmax(oh[b, k]), (18, 18))
            if (b, k) != (0, 3) and not (2 <= min(pts[b, k] * F(18)) and max(pts[b, k] * F(18)) < 16):
                continue                                                      # one pixel off a border the reflected taps move the peak onto it
            assert (x, y) == (min(int(pts[b, k, 0] * F(18)), 17), min(int(pts[b, k, 1] * F(18)), 17))      # (int) of the fp32 product


def test_apply_zero_and_a_rejected_image_pass_through_as_bits():
    imgs, hm, pts = _case(2)
    hm[1, 2, 3, 4] = np.nan
    shift = R.row(I=(1, 0, -30, 0, 1, 0), Fw=(1, 0, 30, 0, 1, 0))                # every point lands beyond Sf: rejected
    oi, oh, op, stats = R.kptaug([R.row(apply=0, swap=1, gain=(0, 0, 0)), shift, R.row(flags=8)], imgs, hm, pts)
    assert stats.tolist() == [0, 1, 2, 1]
    assert np.array_equal(u32(oi), u32(imgs)) and np.array_equal(u32(oh), u32(hm)) and np.array_equal(u32(op), u32(pts))


@pytest.mark.parametrize("S", [16, 18])
def test_quarter_turns_about_the_centre_are_rot90(S):
    imgs, hm, _ = _case(3, B=1, S=S)
    centre = np.full((1, 7, 2), 0.5, F)                                           # stays inside under every turn
    n = S - 1
    turns = {1: (0, -1, n, 1, 0, 0), 2: (-1, 0, n, 0, -1, n), 3: (0, 1, 0, -1, 0, n)}     # I of np.rot90(m, k): out[y, x] = m[sy, sx]
    for k, I in turns.items():
        fwd = np.round(np.linalg.inv(np.vstack([np.array(I, float).reshape(2, 3), [0, 0, 1]])))[:2].ravel()
        oi, _, _, stats = R.kptaug([R.row(I=I, Fw=fwd)], imgs, hm, centre)
        assert stats.tolist() == [1, 0, 0, 0]
        assert np.array_equal(u32(oi[0]), u32(np.rot90(imgs[0], k, axes=(1, 2))))


def test_a_flip_mirrors_the_pixels_and_permutes_the_points():
    S = 18
    imgs, hm, pts = _case(4, S=S)
    d = KA.descriptor(S, flip=True)
    assert d[0] == 3
    oi, oh, op, stats = R.kptaug([d] * 3, imgs, hm, pts)
    assert stats.tolist() == [3, 0, 0, 0]
    assert np.array_equal(u32(oi), u32(imgs[..., ::-1]))
    want = pts[:, list(R.PERM)].copy()
    want[..., 0] = (F(S - 1) - want[..., 0] * F(S)) / F(S)
    want[..., 1] = (want[..., 1] * F(S)) / F(S)
    assert np.array_equal(u32(op), u32(want))


def test_the_clamp_at_both_ends_and_the_half_pixel_blend():
    imgs = np.array([[[[0.25, 0.75], [0.5, 1.0]]]], F).repeat(8, 2).repeat(8, 3)          # [1,1,16,16]
    hm, pts = np.zeros((1, 7, 16, 16), F), np.full((1, 7, 2), 0.5, F)
    oi, _, _, _ = R.kptaug([R.row(gain=(4, 1, 1), bias=(-1.5, 0, 0))], imgs, hm, pts)
    assert set(np.unique(oi)) == {0.0, 0.5, 1.0} and oi[0, 0, 0, 0] == 0.0 and oi[0, 0, 15, 15] == 1.0
    oi, _, _, _ = R.kptaug([R.row(I=(1, 0, 0.5, 0, 1, 0))], imgs, hm, pts)                # half a pixel to the right: the mean at the seam
    assert oi[0, 0, 0, 7] == 0.5 and oi[0, 0, 0, 6] == 0.25 and oi[0, 0, 0, 15] == 0.75  # and the edge replicated
