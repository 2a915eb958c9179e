"""Mosaic augmentation, host half (no GPU): the second header and library (include/mdcv_aug.h, libmdcv_aug.so), the entry's argument check,
properties of the NumPy restatement of csrc/mosaic.hip (tests/helpers/mosaic_ref.py), the draws of `MosaicBatches`, the loop's defaults."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mosaic_ref as R  # noqa: E402
from mdcv import _lib  # noqa: E402
from mdcv.data import mosaic as M  # noqa: E402

ARGS = ["desc_host", "desc", "B", "C", "H", "W", "in", "out", "targets_in", "T", "targets_out", "T_out", "min_px", "min_visible", "stats",
        "stream"]


# ------------------------------------------------------------------------------------------------------------ header and library
def test_the_header_parses_and_names_the_arguments():
    protos = _lib.parse_header(_lib.AUG_HEADER)
    assert list(protos) == ["mdcv_mosaic_batch"]
    assert protos["mdcv_mosaic_batch"][2] == ARGS


def test_the_library_exports_exactly_the_header():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.AUG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\bT (mdcv_\w+)", out)) == set(_lib.parse_header(_lib.AUG_HEADER))
    A = _lib.aug_lib()
    assert A is _lib.aug_lib() and A is not _lib.lib() and callable(A.mosaic_batch)


def test_the_main_header_gained_no_prototype():
    main = _lib.parse_header()
    assert "mdcv_mosaic_batch" not in main and "mosaic_batch" not in open(_lib.HEADER).read()
    assert not set(main) & set(_lib.parse_header(_lib.AUG_HEADER))
    assert _lib.HEADER.endswith(os.path.join("include", "mdcv_hip.h")) and _lib.AUG_HEADER.endswith(os.path.join("include", "mdcv_aug.h"))


# ------------------------------------------------------------------------------------------------------------ the argument check
class _Call:
    """a call of the entry whose every argument is good, over host arrays standing in for the device buffers (a bad argument returns
    before anything is dereferenced but desc_host)"""

    def __init__(self, B=3, C=3, H=8, W=10, T=2, T_out=8):
        self.kw = dict(B=B, C=C, H=H, W=W, T=T, T_out=T_out, min_px=2.0, min_visible=0.25, stream=None)
        self.desc_host = np.array([[1, 4, 5, 0, 1, 2, 0, 0]] * B, np.int32)
        self.buf = {"desc": np.zeros((B, 8), np.int32), "in": np.zeros((B, C, H, W), np.float32), "out": np.zeros((B, C, H, W), np.float32),
                    "targets_in": np.zeros((B, T, 5), np.float32), "targets_out": np.zeros((B, T_out, 5), np.float32),
                    "stats": np.zeros(4, np.int32)}

    def __call__(self, **over):
        a = dict(self.kw, desc_host=self.desc_host.ctypes.data, **{k: v.ctypes.data for k, v in self.buf.items()})
        a.update(over)
        return _lib.aug_lib().mosaic_batch(*[a[k] for k in ARGS])


def test_every_bad_argument_is_reported_without_a_gpu():
    c = _Call()
    for name in ("desc_host", "desc", "in", "out", "targets_in", "targets_out", "stats"):
        assert c(**{name: None}) == -1, name
    for name in ("B", "H", "W", "T", "T_out"):
        assert c(**{name: 0}) == -1 and c(**{name: -3}) == -1, name
    assert c(C=0) == -1 and c(C=5) == -1
    assert c(B=65536) == -1 and c(T=65537) == -1 and c(T_out=65537) == -1                  # the header's own limits (32-bit row indices, the grid)
    assert c(H=4097) == -1 and c(W=4097) == -1
    assert c(min_px=0.5) == -1 and c(min_px=float("nan")) == -1
    assert c(min_visible=-0.01) == -1 and c(min_visible=1.01) == -1 and c(min_visible=float("nan")) == -1
    # out overlapping in, targets_out overlapping targets_in: the same buffer, and one word into it
    assert c(out=c.buf["in"].ctypes.data) == -1 and c(out=c.buf["in"].ctypes.data + c.buf["in"].nbytes - 4) == -1
    assert c(targets_out=c.buf["targets_in"].ctypes.data) == -1
    assert c(targets_in=c.buf["targets_out"].ctypes.data + c.buf["targets_out"].nbytes - 4) == -1


@pytest.mark.parametrize("word,value", [(0, 2), (0, -1), (1, 0), (1, 10), (2, 0), (2, 8), (3, 3), (4, -1), (5, 3), (6, 1 << 30), (7, 1)])
def test_a_bad_host_descriptor_row_is_reported(word, value):
    c = _Call()
    c.desc_host[2, word] = value
    assert not R.row_ok(c.desc_host[2], 3, 8, 10)
    assert c() == -1


def test_the_restatement_accepts_what_the_entry_documents():
    assert R.row_ok([0, 99, -5, 77, 77, 77, 77, 9], 3, 8, 10)                 # pass-through: the other words are free
    assert R.row_ok([1, 1, 1, 0, 0, 0, 0, 0], 3, 8, 10) and R.row_ok([1, 9, 7, 2, 2, 2, 2, 0], 3, 8, 10)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _random_case(seed, B=5, C=3, H=29, W=37, T=6, p_apply=0.8):
    g = np.random.default_rng(seed)
    imgs = g.random((B, C, H, W), dtype=np.float32)
    tg = np.zeros((B, T, 5), np.float32)
    for b in range(B):
        n = int(g.integers(0, T + 1))
        tg[b, :n, 0] = g.integers(0, 3, n)
        tg[b, :n, 1:3] = g.uniform(0.02, 0.98, (n, 2))
        tg[b, :n, 3:5] = g.uniform(0.02, 0.6, (n, 2))
    desc = np.array([[int(g.random() < p_apply), g.integers(1, W), g.integers(1, H), *g.integers(0, B, 4), 0] for _ in range(B)], np.int32)
    return desc, imgs, tg


def test_every_output_pixel_is_the_source_pixel_the_formula_names():
    for seed in range(4):
        desc, imgs, _ = _random_case(seed)
        B, C, H, W = imgs.shape
        out = R.pixels(desc, imgs)
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    s, sy, sx = R.source_of(desc[b], b, y, x, H, W)
                    assert 0 <= sy < H and 0 <= sx < W
                    assert np.array_equal(out[b, :, y, x].view(np.uint32), imgs[s, :, sy, sx].view(np.uint32)), (seed, b, y, x)


def test_apply_zero_is_the_identity():
    desc, imgs, tg = _random_case(7)
    desc[:, 0] = 0
    out, tout, stats = R.mosaic(desc, imgs, tg, tg.shape[1], 2.0, 0.25)
    assert np.array_equal(out.view(np.uint32), imgs.view(np.uint32)) and np.array_equal(tout.view(np.uint32), tg.view(np.uint32))
    assert stats.tolist() == [int((tg.sum(2) > 0).sum()), 0, 0, 0]


@pytest.mark.parametrize("min_px,min_visible", [(1.0, 0.0), (2.0, 0.25), (4.0, 1.0)])
def test_kept_rows_are_inside_the_grid_and_large_enough_and_every_candidate_is_counted(min_px, min_visible):
    for seed in range(6):
        desc, imgs, tg = _random_case(100 + seed, W=37 + 379 * (seed % 2), H=29 + 387 * (seed % 2))
        B, _, H, W = imgs.shape
        T = tg.shape[1]
        for T_out in (4 * T, 5):
            tout, stats = R.labels(desc, tg, T_out, min_px, min_visible, H, W)
            cands = sum(int((tg[b].sum(1) > 0).sum()) if d[0] == 0 else sum(int((tg[s].sum(1) > 0).sum()) for s in d[3:7])
                        for b, d in enumerate(desc))
            assert int(stats[:3].sum()) == cands and stats[3] == 0
            assert T_out == 5 or stats[2] == 0
            for b in range(B):
                rows = tout[b][tout[b].sum(1) > 0]
                assert np.array_equal(tout[b, :len(rows)], rows) and not tout[b, len(rows):].any()      # kept rows first, zeros behind
                if desc[b, 0] == 1 and len(rows):
                    assert (rows[:, 1] > 0).all() and (rows[:, 1] < 1).all() and (rows[:, 2] > 0).all() and (rows[:, 2] < 1).all()
                    # w' >= min_px exactly; w' / Wf and the product back each round once (2^-24 relative): 2^-22 covers both
                    assert (rows[:, 3] * np.float32(W) >= min_px * (1 - 2 ** -22)).all() and (rows[:, 4] * np.float32(H) >= min_px * (1 - 2 ** -22)).all()
            assert int(sum(len(tout[b][tout[b].sum(1) > 0]) for b in range(B))) == int(stats[0])


def test_the_row_order_is_quadrant_then_source_row():
    """every source row carries its own class id: the kept classes of an image must be increasing in (quadrant, source row)"""
    B, T, H, W = 4, 5, 64, 64
    g = np.random.default_rng(3)
    tg = np.zeros((B, T, 5), np.float32)
    tg[..., 0] = np.arange(B * T).reshape(B, T) + 1
    tg[..., 1:3] = g.uniform(0.1, 0.9, (B, T, 2))
    tg[..., 3:5] = 0.3
    desc = np.array([[1, 30, 34, 3, 1, 0, 2, 0], [1, 20, 40, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, 40, 20, 0, 3, 3, 0, 0]], np.int32)
    tout, stats = R.labels(desc, tg, 4 * T, 2.0, 0.05, H, W)
    assert stats[0] > 12
    for b in (0, 1, 3):
        cls = tout[b][tout[b].sum(1) > 0][:, 0].astype(int) - 1
        want = [(q, s * T + t) for q, s in enumerate(desc[b, 3:7]) for t in range(T)]
        at = 0
        for c in cls:                                                   # a subsequence of `want`, in order; a source may repeat over quadrants
            while at < len(want) and want[at][1] != c:
                at += 1
            assert at < len(want), (b, cls)
            at += 1


def test_the_label_arithmetic_on_hand_computed_rows():
    H = W = 100
    f = np.float32
    # a box in the top-left quadrant (source bottom-right corner): centre (90, 80), 10 x 20 px; centre at (50, 60): shifted by (-50, -40)
    o = R.label(np.array([2, 0.9, 0.8, 0.1, 0.2], f), 0, 0, 50, 60, H, W, 2.0, 0.25)
    assert o[0] == 2 and np.allclose(o[1:], [0.40, 0.40, 0.10, 0.20], atol=1e-6)
    # the same box straddling the source's cut at x = 50 for quadrant 1 (source bottom-left corner shows source x < 50): nothing visible
    assert R.label(np.array([2, 0.9, 0.8, 0.1, 0.2], f), 1, 0, 50, 60, H, W, 2.0, 0.25) is None
    # an edge exactly on the centre: source box x in [0, 20] shown in quadrant 1 starts at xc
    o = R.label(np.array([0, 0.1, 0.9, 0.2, 0.1], f), 1, 0, 50, 60, H, W, 2.0, 0.25)
    assert np.allclose(o[1:], [0.60, 0.50, 0.20, 0.10], atol=1e-6)
    # NaN anywhere drops the row
    for k in range(1, 5):
        r = np.array([0, 0.1, 0.9, 0.2, 0.1], f)
        r[k] = np.nan
        assert R.label(r, 1, 0, 50, 60, H, W, 2.0, 0.25) is None


# ------------------------------------------------------------------------------------------------------------ the draws
def test_the_draws_are_a_function_of_seed_epoch_and_batch():
    a = M.draw_rows(5, 2, 7, 16, 416, 416)
    assert a == M.draw_rows(5, 2, 7, 16, 416, 416)
    assert a != M.draw_rows(6, 2, 7, 16, 416, 416) and a != M.draw_rows(5, 3, 7, 16, 416, 416) and a != M.draw_rows(5, 2, 8, 16, 416, 416)
    for B, H, W in ((16, 416, 416), (1, 2, 2), (7, 29, 37)):
        for i in range(20):
            for b, row in enumerate(M.draw_rows(0, 1, i, B, H, W)):
                assert row[0] == 1 and b in row[3:7] and row[7] == 0 and R.row_ok(row, B, H, W)
                assert max(1, int(np.ceil(0.25 * W))) <= row[1] <= max(1, min(W - 1, int(np.floor(0.75 * W))))
    assert all(r[0] == 0 for i in range(10) for r in M.draw_rows(0, 1, i, 8, 64, 64, p=0.0))
    frac = np.mean([r[0] for i in range(200) for r in M.draw_rows(1, 1, i, 8, 64, 64, p=0.3)])
    assert 0.25 < frac < 0.35


def test_the_wrapper_forwards_and_validates():
    class Loader(list):
        dataset = range(12)
        closed = False

        def close(self):
            self.closed = True
    ld = Loader([1, 2, 3])
    m = M.MosaicBatches(ld, draws=lambda e, i, B: [[0] * 8] * B)
    assert len(m) == 3 and m.dataset is ld.dataset and m.active
    m.close()
    assert ld.closed
    m.active = False
    assert list(m) == [1, 2, 3] and m.epoch == 0                                  # handed through untouched, no epoch of draws consumed
    assert m.rows(1, 0, 2, 8, 8).dtype == np.int32 and m.rows(1, 0, 2, 8, 8).shape == (2, 8)
    with pytest.raises(ValueError):
        M.MosaicBatches(ld, draws=lambda e, i, B: [[0] * 7] * B).rows(1, 0, 3, 8, 8)
    for bad in (dict(p=1.5), dict(centre=(0.8, 0.2)), dict(min_px=0.5), dict(min_visible=2.0)):
        with pytest.raises(ValueError):
            M.MosaicBatches(ld, **bad)
    assert m.stats() == dict(kept=0, dropped=0, overflow=0, errors=0, images=0, composed=0)          # nothing launched: no device touched
    assert "mosaic off" in m.summary_line("train", 1)


def test_the_training_loop_defaults_to_off():
    from mdcv.yolo import train as T
    sig = inspect.signature(T.train).parameters
    assert sig["mosaic"].default == 0.0 and sig["mosaic_off_epochs"].default == 0
    opt = T._parser().parse_args(["--model_cfg", "x.cfg"])
    assert opt.mosaic == 0.0 and opt.mosaic_off_epochs == 0
    opt = T._parser().parse_args(["--model_cfg", "x.cfg", "--mosaic", "0.5", "--mosaic_off_epochs", "3"])
    assert opt.mosaic == 0.5 and opt.mosaic_off_epochs == 3
