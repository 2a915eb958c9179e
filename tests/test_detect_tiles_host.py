"""Tile-and-scale inference, the host half (no GPU): the NumPy restatement of mdcv_detect_merge_tiles against vectors of the reference's own
`nms` (tests/golden/detect_tiles, written by tests/golden/make_golden_detect_tiles.py), mdcv.yolo.detect.TiledBatchPlan against the
training pipeline's tile geometry, and the argument checks of the C entry point, which run before anything touches a device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detect_tiles_numpy as TN  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
EARG = -1


def test_restatement_equals_the_reference_nms():
    z = np.load(os.path.join(G, "detect_tiles", "cases.npz"))
    i, kept, cut, tiles_seen, lost = 0, 0, 0, 0, 0
    while f"boxes_{i}" in z.files:
        B, overlap, top_k = int(z[f"args_{i}"][0]), float(z[f"args_{i}"][1]), int(z[f"args_{i}"][2])
        boxes, prob, count, tiles = z[f"boxes_{i}"], z[f"prob_{i}"], z[f"count_{i}"], z[f"tiles_{i}"]
        assert TN.table_ok(tiles, B)
        out_boxes, out_prob, src, n = TN.merge_tiles(boxes, prob, count, tiles, B, overlap, -1.0, top_k)     # the seam rule off
        for b in range(B):
            want = z[f"keep_{i}_{b}"]
            assert n[b] == len(want) and np.array_equal(src[b, :n[b]], want), (i, b)
            for c, (t, k) in enumerate(want):                                 # and the kept rows are those candidates, offset once
                assert np.array_equal(out_boxes[b, c].view(np.int32), TN.offset_boxes(boxes[t, k], tiles[t, 1], tiles[t, 2])[0].view(np.int32))
                assert out_prob[b, c] == prob[t, k]
            assert not out_boxes[b, n[b]:].any() and not out_prob[b, n[b]:].any() and (src[b, n[b]:] == -1).all()
            total = int(count[tiles[:, 0] == b].sum())
            kept, cut = kept + int(n[b]), cut + (total > top_k)
            tiles_seen = max(tiles_seen, len(set(want[:, 0])))
            lost += min(total, top_k) - int(n[b])
        i += 1
    assert i >= 6 and kept >= 400 and cut >= 3 and tiles_seen >= 9 and lost >= 50       # not vacuous: duplicates are removed


def test_seam_rule_of_the_restatement():
    """a half box of tile 0 inside a whole box of tile 1: IoU 0.5 stays at overlap 0.6, inter / min(area) = 1 goes at 0.6"""
    boxes = np.array([[54, 20, 64, 40], [54, 20, 74, 40]], np.float32)
    tile = np.array([1, 0])                                                   # visiting order: the whole box (tile 1) first
    assert list(TN.greedy_scan(boxes[::-1], tile, 0.6, -1.0)) == [0, 1]
    assert list(TN.greedy_scan(boxes[::-1], tile, 0.6, 0.6)) == [0]
    assert list(TN.greedy_scan(boxes[::-1], np.array([1, 1]), 0.6, 0.6)) == [0, 1]


# --------------------------------------------------------------------------------------------------------------------- the batch plan
@pytest.fixture(scope="module")
def sizes():
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    s = [(z[k].shape[1], z[k].shape[0]) for k in sorted(z.files)]
    assert s == [(301, 173), (97, 211), (257, 129), (120, 90)]
    return s


def _per_frame(plan):
    return [plan.tile_frame.count(b) for b in range(plan.B)]


def test_tiled_plan_scale_one(sizes):
    from mdcv.data import images as I
    from mdcv.yolo.detect import TiledBatchPlan
    plan = TiledBatchPlan(sizes, 64, 64, 200, [1.0] * 4)
    assert tuple(_per_frame(plan)) == (15, 8, 15, 4) and plan.NT == 42 and plan.tile_table.shape == (42, 4)
    assert plan.tile_table.dtype == np.int32 and (np.diff(plan.tile_table[:, 0]) >= 0).all() and not plan.tile_table[:, 3].any()
    at = 0
    for b, (w, h) in enumerate(sizes):
        n = I.n_patches(w, h, 1.0, 64, 64)
        sw, sh = I.scaled_size(w, h, 1.0)
        covered = None
        for i in range(n):
            g, row = plan.geoms[at], plan.tile_table[at]
            want = I.sample_geometry(w, h, 64, 64, ts=True, scale=1.0, patch_index=i)
            assert g.desc == want.desc and np.array_equal(g.col, want.col) and np.array_equal(g.row, want.row)
            assert plan.frefs[at] == I.frame_reference(want, plan.offsets[b])   # read in place from the frame's pool bytes
            x0, y0 = int(round(want.boundary[0])), int(round(want.boundary[1]))
            assert tuple(row) == (b, x0 - want.hp, y0 - want.vp, 0)             # the rounded patch origin minus the border
            if covered is None:
                hp, vp = want.hp, want.vp
                covered = np.zeros((sh + 2 * vp, sw + 2 * hp), bool)
            covered[row[2] + vp:row[2] + vp + 64, row[1] + hp:row[1] + hp + 64] = True
            assert row[1] >= -hp and row[2] >= -vp and row[1] + 64 <= sw + hp and row[2] + 64 <= sh + vp
            at += 1
        assert covered.all()                                                  # the tiles cover [-hp, sw + hp) x [-vp, sh + vp)
    assert at == plan.NT
    # the layout: the tile table lies in the pinned input, in front of the pool; src behind the output tables
    assert plan.det_off + 4 * 6 * 8 <= plan.tile_off and plan.tile_off + 42 * 16 <= plan.pool_off and plan.tile_off % 16 == 0
    assert plan.src_off >= plan.skip_off + 4 * 4 and plan.nbytes >= plan.src_off + 4 * 200 * 8


def test_tiled_plan_bordered_tiles_and_descriptors(sizes):
    from mdcv.yolo.detect import TiledBatchPlan
    scale = 0.4
    plan = TiledBatchPlan(sizes, 64, 64, 200, [scale] * 4)
    per = _per_frame(plan)
    assert per[3] == 1 and per[1] == 2
    first = np.cumsum([0] + per)
    assert tuple(plan.tile_table[first[3]]) == (3, -8, -14, 0)                # 120 x 90 -> 48 x 36: ONE tile between borders of 8 and 14
    assert list(plan.tile_table[first[1]:first[2], 1]) == [-13, -13]          # 97 x 211 -> 38 x 84: two tiles, border 13
    for s in (scale, 1.0, 1.5, 0.1 + 0.2):
        d = TiledBatchPlan(sizes, 64, 64, 200, [s] * 4).desc
        assert d.dtype == np.int64 and d.shape == (4, 6)
        assert (d[:, 3] == np.array([s], np.float64).view(np.int64)[0]).all()  # ratio == scale, bit for bit
        assert not d[:, 4:].any()                                             # zero pads
        assert [tuple(r) for r in d[:, 1:3]] == sizes and list(d[:, 0]) == plan.offsets
    mixed = TiledBatchPlan(sizes, 64, 64, 200, [1.0, 0.4, 1.0, 0.4])
    assert _per_frame(mixed) == [15, 2, 15, 1]


def test_tiled_plan_errors_name_the_frame(sizes):
    from mdcv.data import images as I
    from mdcv.yolo.detect import TiledBatchPlan
    odd = None
    for w in range(70, 140):                                                  # an odd patch size with a .5 offset somewhere
        try:
            for i in range(I.n_patches(w, 50, 1.0, 63, 63)):
                I.sample_geometry(w, 50, 63, 63, ts=True, scale=1.0, patch_index=i)
        except ValueError:
            odd = w
            break
    assert odd is not None
    with pytest.raises(ValueError, match=r"^frame 8: .*odd patch size"):
        TiledBatchPlan([(64, 64), (odd, 50)], 63, 63, 200, [1.0, 1.0], first=7)
    with pytest.raises(ValueError, match=r"^frame 0: .*more than 64"):
        TiledBatchPlan([(640, 640)], 64, 64, 200, [1.0])
    with pytest.raises(ValueError, match="frame 1"):
        TiledBatchPlan(sizes[:2], 64, 64, 200, [1.0, 0.001])                  # nothing left of the frame
    with pytest.raises(ValueError):
        TiledBatchPlan(sizes, 64, 64, 200, [1.0])


# ------------------------------------------------------------------------------------------------- the entry point's argument checks
def test_argument_errors_need_no_device():
    """every rejected call returns before a pointer is read or anything is enqueued, so null device pointers are enough"""
    from mdcv import _lib
    L = _lib.lib()

    def call(tiles, B, K=8, top_k=16, T=None):
        tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 4)
        T = len(tiles) if T is None else T
        return L.detect_merge_tiles(None, None, None, tiles.ctypes.data if len(tiles) else None, None, T, K, B, 0.5, -1.0, top_k, None, None,
                                    None, None, None)

    good = [[0, 0, 0, 0], [0, 32, 0, 0], [1, -8, -14, 0]]
    assert TN.table_ok(good, 2)
    assert call(good, 2) == EARG                                              # a good table: the null pointers are what is wrong
    assert call([[1, 0, 0, 0], [0, 0, 0, 0]], 2) == EARG and not TN.table_ok([[1, 0, 0, 0], [0, 0, 0, 0]], 2)       # unsorted
    assert call([[0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]], 2) == EARG        # a frame's tiles not contiguous
    assert call([[0, 0, 0, 0], [2, 0, 0, 0]], 2) == EARG and call([[-1, 0, 0, 0]], 2) == EARG                         # frame out of range
    assert call(good, 2, top_k=513) == EARG and call(good, 2, top_k=0) == EARG and call(good, 2, K=513) == EARG
    assert call([[0, (1 << 24) + 1, 0, 0]], 1) == EARG and call([[0, 0, 0, 1]], 1) == EARG
    assert call([[0, i, 0, 0] for i in range(65)], 1) == EARG and not TN.table_ok([[0, i, 0, 0] for i in range(65)], 1)
    assert call(good, -1) == EARG and call(good, 2, T=-1) == EARG and call(good, 2, K=-1) == EARG
    # nothing to merge is not an error, and needs no pointer
    assert call(np.zeros((0, 4)), 0) == 0 and call(np.zeros((0, 4)), 3) == 0 and call(good, 2, K=0) == 0
