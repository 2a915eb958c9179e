"""Tile-and-scale inference on the device: mdcv_detect_merge_tiles (csrc/detect_tiles.hip) through the C ABI against its NumPy restatement
(tests/helpers/detect_tiles_numpy.py, itself pinned against the reference's `nms` by tests/test_detect_tiles_host.py), bit for bit and
with guard words around every output; then mdcv.yolo.detect's tiled detectors end to end against the same chain assembled from the
public pieces."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detect_draw_numpy as D  # noqa: E402
import detect_tiles_numpy as TN  # noqa: E402
import kpt_draw_numpy as KD  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
F = np.float32
GUARD, GW = 0x5A5A5A5A, 16                      # the guard word and how many lie in front of and behind every output
EARG = -1


# --------------------------------------------------------------------------------------------------------------- the kernel, raw ABI
def _guarded(words):
    return torch.full((GW + words + GW,), GUARD, dtype=torch.int32, device="cuda")


def _payload(t, words, dtype, shape):
    a = t.cpu().numpy()
    assert (a[:GW] == GUARD).all() and (a[GW + words:] == GUARD).all()          # nothing in front of or behind the output
    return a[GW:GW + words].view(dtype).reshape(shape)


def _merge(boxes, prob, count, tiles, B, overlap, contain, top_k, tiles_dev=None):
    """one mdcv_detect_merge_tiles call -> (rc, out_boxes, out_prob, out_src, out_count); untouched outputs read as GUARD words"""
    from mdcv import _lib
    L = _lib.lib()
    boxes = np.ascontiguousarray(boxes, F)
    T, K = boxes.shape[0], boxes.shape[1]
    tiles = np.ascontiguousarray(tiles, np.int32).reshape(T, 4)

    def dev(a, dtype):
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        return torch.from_numpy(a if a.size else np.zeros(1, dtype)).cuda()
    d_boxes, d_prob, d_count = dev(boxes, F), dev(prob, F), dev(count, np.int32)
    d_tiles = dev(tiles if tiles_dev is None else tiles_dev, np.int32)
    nb, npr, ns, nc = B * top_k * 4, B * top_k, B * top_k * 2, B
    ob, op, os_, oc = _guarded(nb), _guarded(npr), _guarded(ns), _guarded(nc)
    rc = L.detect_merge_tiles(d_boxes.data_ptr(), d_prob.data_ptr(), d_count.data_ptr(), tiles.ctypes.data if T else None, d_tiles.data_ptr(),
                              T, K, B, float(overlap), float(contain), top_k, ob.data_ptr() + 4 * GW, op.data_ptr() + 4 * GW,
                              os_.data_ptr() + 4 * GW, oc.data_ptr() + 4 * GW, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc, _payload(ob, nb, F, (B, top_k, 4)), _payload(op, npr, F, (B, top_k)), _payload(os_, ns, np.int32, (B, top_k, 2)),
            _payload(oc, nc, np.int32, (B,)))


def _check(boxes, prob, count, tiles, B, overlap, contain, top_k):
    """the launch equals the restatement: the bits of boxes and probabilities, out_src, the counts"""
    rc, ob, op, src, cnt = _merge(boxes, prob, count, tiles, B, overlap, contain, top_k)
    assert rc == 0
    wb, wp, wsrc, wcnt = TN.merge_tiles(boxes, prob, count, tiles, B, overlap, contain, top_k)
    assert np.array_equal(cnt, wcnt), (cnt, wcnt)
    assert np.array_equal(src, wsrc)
    assert np.array_equal(ob.view(np.int32), wb.view(np.int32)) and np.array_equal(op.view(np.int32), wp.view(np.int32))
    return ob, op, src, cnt


def _random_tiles(rng, T, K, patch=64, lo=4, hi=28):
    """boxes in tile coordinates in EVERY slot (slots past a tile's count must not be read as candidates), scores in (0, 1)"""
    c = rng.uniform(0, patch, (T, K, 2))
    s = rng.uniform(lo, hi, (T, K, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], axis=2).astype(F)
    prob = -np.sort(-rng.uniform(0.01, 0.99, (T, K)).astype(F), axis=1)        # a tile's slots are in descending confidence
    return boxes, prob


def test_merge_mixed_counts():
    """(a) B = 3, K = 8: frame 0 has 3 tiles with counts (8, 3, 0), frame 1 one tile with count 0, frame 2 two tiles; top_k = 16"""
    rng = np.random.default_rng(11)
    boxes, prob = _random_tiles(rng, 6, 8)
    count = np.array([8, 3, 0, 0, 5, 8], np.int32)
    tiles = np.array([[0, 0, 0, 0], [0, 40, 0, 0], [0, 80, 0, 0], [1, 0, 0, 0], [2, -5, -9, 0], [2, 35, -9, 0]], np.int32)
    prob[2], prob[3], prob[1, 3:] = 0.999, 0.999, 0.998                         # confident rows past the counts: never candidates
    for contain in (-1.0, 0.5):
        ob, op, src, cnt = _check(boxes, prob, count, tiles, 3, 0.45, contain, 16)
        assert cnt[1] == 0 and 0 < cnt[0] <= 11 and 0 < cnt[2] <= 13
        assert all((t == 0) or (t == 1 and k < 3) for t, k in src[0, :cnt[0]])      # nothing from past a count
        assert (np.diff(op[0, :cnt[0]]) <= 0).all() and (np.diff(op[2, :cnt[2]]) <= 0).all()
    assert len(set(src[0, :cnt[0], 0])) == 2 and len(set(src[2, :cnt[2], 0])) == 2


def test_merge_same_box_seen_by_two_tiles():
    """(b) offsets make the two merged boxes the same box: exactly one survives, out_src names the more confident"""
    boxes = np.zeros((2, 4, 4), F)
    boxes[0, 0], boxes[1, 0] = [40, 10, 60, 30], [8.25, 10, 28.25, 30]          # + (0, 0) and + (32, 0): IoU 0.975
    tiles = np.array([[0, 0, 0, 0], [0, 32, 0, 0]], np.int32)
    count = np.array([1, 1], np.int32)
    for p0, p1, who in ((0.9, 0.8, 0), (0.7, 0.8, 1)):
        prob = np.zeros((2, 4), F)
        prob[0, 0], prob[1, 0] = p0, p1
        ob, op, src, cnt = _check(boxes, prob, count, tiles, 1, 0.5, -1.0, 8)
        assert cnt[0] == 1 and tuple(src[0, 0]) == (who, 0) and op[0, 0] == F(max(p0, p1))
    assert tuple(ob[0, 0]) == (40.25, 10, 60.25, 30)                            # tile 1's box in scaled-frame pixels


def test_merge_tie_order():
    """(c) bit-equal scores across two tiles and inside one tile: ascending tile, then ascending slot -- also where the top_k cut falls"""
    T, K = 3, 4
    boxes = np.zeros((T, K, 4), F)
    for t in range(T):
        for k in range(K):
            boxes[t, k] = [10 * k, 20 * t, 10 * k + 8, 20 * t + 8]               # disjoint in the frame: nothing is removed
    tiles = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    prob = np.array([[0.75, 0.5, 0.5, 0.25], [0.75, 0.75, 0.5, 0.125], [0.875, 0.5, 0.25, 0.25]], F)
    count = np.array([4, 4, 4], np.int32)
    want = [(2, 0), (0, 0), (1, 0), (1, 1), (0, 1), (0, 2), (1, 2), (2, 1), (0, 3), (2, 2), (2, 3), (1, 3)]
    ob, op, src, cnt = _check(boxes, prob, count, tiles, 1, 0.5, -1.0, 16)
    assert cnt[0] == 12 and [tuple(s) for s in src[0, :12]] == want
    for top_k in (3, 6, 7, 10):                                                 # cuts inside runs of equal scores
        ob, op, src, cnt = _check(boxes, prob, count, tiles, 1, 0.5, -1.0, top_k)
        assert cnt[0] == top_k and [tuple(s) for s in src[0]] == want[:top_k]


def test_merge_cut_before_scan():
    """(d) 5 tiles x 8 candidates, top_k = 16: only the 16 most confident are scanned, so what they remove is not refilled from below"""
    rng = np.random.default_rng(4)
    T, K = 5, 8
    boxes, _ = _random_tiles(rng, T, K)
    tiles = np.array([[0, 30 * t, 0, 0] for t in range(T)], np.int32)
    scores = (0.1 + 0.8 * rng.permutation(T * K) / (T * K)).astype(F).reshape(T, K)
    prob = -np.sort(-scores, axis=1)
    top = np.argsort(-prob.reshape(-1))[:16]
    for n, i in enumerate(top[1:9]):                                            # eight of the top 16 are copies of the most confident box
        t, k = divmod(int(i), K)
        t0, k0 = divmod(int(top[0]), K)
        boxes[t, k] = boxes[t0, k0] + np.array([tiles[t0, 1] - tiles[t, 1], 0, tiles[t0, 1] - tiles[t, 1], 0], F)
    count = np.full(T, K, np.int32)
    ob, op, src, cnt = _check(boxes, prob, count, tiles, 1, 0.5, -1.0, 16)
    assert cnt[0] <= 8
    allowed = {divmod(int(i), K) for i in top}
    assert all(tuple(s) in allowed for s in src[0, :cnt[0]])
    _, _, _, more = _check(boxes, prob, count, tiles, 1, 0.5, -1.0, 40)
    assert more[0] > cnt[0]                                                     # without the cut, lower candidates would be kept


def test_merge_seam_rule():
    """(e) a half box in tile 0 inside a whole box of tile 1, IoU 0.5 < overlap 0.6: stays with contain_thres -1, goes with 0.6; the same
    pair inside ONE tile stays in both settings"""
    boxes = np.zeros((2, 2, 4), F)
    prob = np.zeros((2, 2), F)
    tiles = np.array([[0, 0, 0, 0], [0, 48, 0, 0]], np.int32)
    boxes[0, 0], prob[0, 0] = [54, 20, 64, 40], 0.6                             # cut off by tile 0's right edge at x = 64
    boxes[1, 0], prob[1, 0] = [6, 20, 26, 40], 0.9                              # (54, 20, 74, 40) in the frame: the whole cone
    count = np.array([1, 1], np.int32)
    _, _, src, cnt = _check(boxes, prob, count, tiles, 1, 0.6, -1.0, 8)
    assert cnt[0] == 2 and [tuple(s) for s in src[0, :2]] == [(1, 0), (0, 0)]
    _, _, src, cnt = _check(boxes, prob, count, tiles, 1, 0.6, 0.6, 8)
    assert cnt[0] == 1 and tuple(src[0, 0]) == (1, 0)
    _, _, src, cnt = _check(boxes, prob, count, tiles, 1, 0.6, 1.0, 8)           # inter / min(area) == 1 <= 1: stays
    assert cnt[0] == 2
    boxes[1, 1], prob[1, 1] = [6, 20, 16, 40], 0.6                              # the same pair, both seen by tile 1
    count = np.array([0, 2], np.int32)
    for contain in (-1.0, 0.6):
        _, _, src, cnt = _check(boxes, prob, count, tiles, 1, 0.6, contain, 8)
        assert cnt[0] == 2 and [tuple(s) for s in src[0, :2]] == [(1, 0), (1, 1)]


def test_merge_zero_area_and_negative_offsets():
    """(f) two zero-area boxes on one another: inter 0, union 0, IoU NaN -> the second leaves; a bordered tile's negative offsets"""
    boxes = np.zeros((2, 4, 4), F)
    prob = np.zeros((2, 4), F)
    tiles = np.array([[0, -8, -14, 0], [0, 24, -14, 0]], np.int32)
    boxes[0, 0], prob[0, 0] = [18, 24, 18, 44], 0.9                             # zero width
    boxes[0, 1], prob[0, 1] = [18, 24, 18, 44], 0.8                             # the same line: NaN
    boxes[0, 2], prob[0, 2] = [30.5, 20.25, 50.5, 40.75], 0.7
    boxes[1, 0], prob[1, 0] = [-14, 24, -14, 44], 0.85                          # the same line seen from tile 1: NaN across tiles
    boxes[1, 1], prob[1, 1] = [40, 50, 40, 50], 0.5                             # a point elsewhere: IoU 0 / area: stays
    count = np.array([3, 2], np.int32)
    for contain in (-1.0, 0.5):
        ob, _, src, cnt = _check(boxes, prob, count, tiles, 1, 0.5, contain, 8)
        kept = [tuple(s) for s in src[0, :cnt[0]]]
        assert (0, 0) in kept and (0, 1) not in kept and (1, 0) not in kept and (0, 2) in kept
        assert tuple(ob[0, 0]) == (10, 10, 10, 30) and tuple(ob[0, kept.index((0, 2))]) == (22.5, 6.25, 42.5, 26.75)


@pytest.mark.parametrize("K,top_k", [(200, 200), (512, 512)])
def test_merge_at_the_documented_limit(K, top_k):
    """(g) MDCV_TILE_MAX_PER_FRAME = 64 tiles of one frame, every slot a candidate, random boxes over an 8 x 8 grid of overlapping tiles;
    a second frame behind it; one tile more in a frame is MDCV_EARG and nothing is written"""
    rng = np.random.default_rng(K)
    T = TN.MAX_TILES_PER_FRAME + 3
    boxes, prob = _random_tiles(rng, T, K, lo=3, hi=14)
    count = rng.integers(K // 2, K + 1, T).astype(np.int32)
    count[:4] = K
    tiles = np.array([[0, 50 * (t % 8) - 7, 50 * (t // 8) - 7, 0] for t in range(64)] + [[1, 40 * i, 0, 0] for i in range(3)], np.int32)
    _, _, src, cnt = _check(boxes, prob, count, tiles, 2, 0.5, 0.7, top_k)
    assert cnt[0] > top_k // 2 and len(set(src[0, :cnt[0], 0])) > 32 and cnt[1] > 0
    over = np.concatenate([tiles[:64], [[0, 0, 0, 0]], tiles[64:]]).astype(np.int32)          # 65 tiles in frame 0
    assert not TN.table_ok(over, 2)
    rc, ob, op, src, cnt = _merge(np.concatenate([boxes, boxes[:1]]), np.concatenate([prob, prob[:1]]), np.append(count, 1), over, 2, 0.5, 0.7, top_k)
    assert rc == EARG
    for a in (ob, op, src, cnt):
        assert (a.view(np.int32) == GUARD).all()


def test_merge_empty_shapes_write_nothing():
    """(h) B = 0, T = 0 and K = 0: MDCV_OK, nothing enqueued or written"""
    rng = np.random.default_rng(2)
    boxes, prob = _random_tiles(rng, 2, 4)
    tiles = np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.int32)
    count = np.array([4, 4], np.int32)
    for b, p, c, t, B in ((boxes[:0], prob[:0], count[:0], tiles[:0], 0), (boxes[:0], prob[:0], count[:0], tiles[:0], 2),
                          (boxes[:, :0], prob[:, :0], count, tiles, 2)):
        rc, ob, op, src, cnt = _merge(b, p, c, t, B, 0.5, -1.0, 8)
        assert rc == 0
        for a in (ob, op, src, cnt):
            assert (a.view(np.int32) == GUARD).all()


def test_merge_checks_the_device_table_again():
    """a device copy that differs from the validated host copy: the frame whose tiles are not contiguous there, or carry an offset out of
    range, gets count 0 and empty slots; the other frames are merged as usual"""
    rng = np.random.default_rng(8)
    boxes, prob = _random_tiles(rng, 5, 6)
    count = np.full(5, 6, np.int32)
    tiles = np.array([[0, 0, 0, 0], [0, 30, 0, 0], [1, 0, 0, 0], [1, 30, 0, 0], [2, 0, 0, 0]], np.int32)
    want = TN.merge_tiles(boxes, prob, count, tiles, 3, 0.5, -1.0, 8)
    for bad_frame, bad in ((0, [[0, 0, 0, 0], [1, 30, 0, 0], [0, 0, 0, 0], [1, 30, 0, 0], [2, 0, 0, 0]]),
                           (1, [[0, 0, 0, 0], [0, 30, 0, 0], [1, 0, 0, 0], [1, 1 << 25, 0, 0], [2, 0, 0, 0]]),
                           (2, [[0, 0, 0, 0], [0, 30, 0, 0], [1, 0, 0, 0], [1, 30, 0, 0], [2, 0, 0, 7]])):
        bad = np.array(bad, np.int32)
        rc, ob, op, src, cnt = _merge(boxes, prob, count, tiles, 3, 0.5, -1.0, 8, tiles_dev=bad)
        assert rc == 0
        frames_bad = {bad_frame} | ({1} if bad_frame == 0 else set())           # case 0 scatters frame 1's tiles too
        for b in range(3):
            if b in frames_bad:
                assert cnt[b] == 0 and not ob[b].any() and not op[b].any() and (src[b] == -1).all()
            else:
                assert cnt[b] == want[3][b] and np.array_equal(src[b], want[2][b]) and np.array_equal(ob[b].view(np.int32), want[0][b].view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------ end to end
SCALE = 1.0


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
def frames():
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    fr = [np.ascontiguousarray(z[k]) for k in sorted(z.files)]
    assert len(fr) == 4 and len({f.shape for f in fr}) > 1
    return fr


def _const(s):
    return lambda w, h: s


def _by_size(w, h):
    return 0.4 if (w, h) == (120, 90) else 1.0                                  # 120 x 90 at 0.4: ONE bordered tile


def _tiles_of(fr, W, H, scale_of):
    """the ts=True geometries of every tile of every frame, the frame of each tile, the tile table and the scales"""
    from mdcv.data import images as I
    geoms, owner, table, scales = [], [], [], []
    for b, f in enumerate(fr):
        w, h = f.shape[1], f.shape[0]
        s = scale_of(w, h)
        scales.append(s)
        for i in range(I.n_patches(w, h, s, W, H)):
            g = I.sample_geometry(w, h, W, H, ts=True, scale=s, patch_index=i)
            geoms.append(g), owner.append(b)
            table.append((b, int(round(g.boundary[0])) - g.hp, int(round(g.boundary[1])) - g.vp, 0))
    return geoms, owner, np.array(table, np.int32), scales


def _reference(net, frames, conf, nms, groups, scale_of, max_boxes=200, contain=-1.0):
    """the chain from the public pieces, per batch of `groups`: transform_batch with the ts=True geometries -> model -> detect_postprocess
    -> the restatement's merge -> the NumPy draw with ratio = scale and zero pads"""
    from mdcv.data import images as I
    from mdcv.yolo.postprocess import detect_postprocess
    W, H = net.img_size()
    out, at, outputs = [], 0, []
    for n in groups:
        fr = frames[at:at + n]
        at += n
        geoms, owner, table, scales = _tiles_of(fr, W, H, scale_of)
        with torch.no_grad():
            pred = net(I.transform_batch([fr[b] for b in owner], geoms, bw=net.get_bw()))
            outputs.append(pred)
            if conf is None:
                continue
            det = detect_postprocess(pred, None, conf, nms, 0.5, W, H, 200)
        mb, mp, src, cnt = TN.merge_tiles(det.boxes.cpu().numpy(), det.prob.cpu().numpy(), det.count.cpu().numpy(), table, len(fr), nms, contain, 200)
        for b, f in enumerate(fr):
            k = min(int(cnt[b]), max_boxes)
            ann, fb, rects, skipped = D.draw_boxes(f, mb[b, :k], scales[b], 0, 0)
            out.append(dict(boxes=fb, prob=mp[b, :k], rects=rects, skipped=skipped, annotated=ann, src=src[b, :k]))
    return out, outputs


@pytest.fixture(scope="module")
def conf_thres(mini, frames):
    """from the model's own objectness over all tiles at SCALE: between the 3rd and the 4th highest of the tile where those are lowest,
    so that every tile keeps candidates"""
    _, outputs = _reference(mini, frames, None, None, [4], _const(SCALE))
    obj = outputs[0][..., 4].cpu().numpy()
    assert obj.shape[0] == 42
    s = -np.sort(-obj, axis=1)
    return float(((s[:, 2].astype(np.float64) + s[:, 3]) / 2).min())


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.boxes.dtype == np.float64 and np.array_equal(g.boxes.view(np.int64), w["boxes"].view(np.int64))
        assert np.array_equal(g.prob, w["prob"]) and np.array_equal(g.rects, w["rects"]) and g.skipped == w["skipped"]
        assert g.src.dtype == np.int32 and np.array_equal(g.src, w["src"])
        ann = g.annotated.cpu().numpy() if torch.is_tensor(g.annotated) else g.annotated
        assert ann.dtype == np.uint8 and np.array_equal(ann, w["annotated"])


def test_tiled_detect_frames_end_to_end(mini, frames, conf_thres):
    from mdcv.yolo.detect import FrameDetections, TiledFrameDetector
    nms = mini.get_threshs()[1]
    want, _ = _reference(mini, frames, conf_thres, nms, [4], _const(SCALE))
    det = TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres)
    assert det.nms_thres == nms and (det.width, det.height) == (64, 64) and det.contain_thres == -1.0
    got = list(det.detect_frames(frames))
    drawn = sum(int((r.rects[:, 2] >= 0).sum()) for r in got)
    tiles_named = [len(set(r.src[:, 0])) for r in got]
    print("conf_thres", conf_thres, "boxes per frame", [len(r.boxes) for r in got], "drawn", drawn, "tiles named per frame", tiles_named)
    assert drawn >= 4 and max(tiles_named) >= 2                                 # not vacuous: boxes of more than one tile of a frame
    assert all(isinstance(r, FrameDetections) and len(r.boxes) <= det.max_boxes for r in got)
    assert any((r.annotated != f).any() for r, f in zip(got, frames))
    for r in got:
        assert (np.diff(r.prob) <= 0).all()
    _same(got, want)
    # two batches (3 + 1): both staging slots, tile indices restart per batch; the same results as in one batch apart from them
    got3 = list(TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres, batch_size=3).detect_frames(iter(frames)))
    want3 = _reference(mini, frames, conf_thres, nms, [3, 1], _const(SCALE))[0]
    _same(got3, want3)
    for a, b in zip(got3, got):
        assert np.array_equal(a.boxes.view(np.int64), b.boxes.view(np.int64)) and np.array_equal(a.prob, b.prob) and np.array_equal(a.annotated, b.annotated)
    assert np.array_equal(got3[3].src[:, 0], got[3].src[:, 0] - 38)             # frame 3's tiles are 38..41 of one batch, 0..3 of its own
    # the pixels stay on the device
    kept = list(det.detect_frames(frames, keep_on_device=True))
    assert all(torch.is_tensor(r.annotated) and r.annotated.is_cuda and r.annotated.shape == f.shape for r, f in zip(kept, frames))
    _same(kept, want)
    # chunks of 7 tiles do not divide the 42
    _same(list(TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres, tile_batch=7).detect_frames(frames)), want)
    # max_boxes caps what is mapped and drawn; the seam rule on
    _same(list(TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres, max_boxes=1).detect_frames(frames)),
          _reference(mini, frames, conf_thres, nms, [4], _const(SCALE), max_boxes=1)[0])
    _same(list(TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres, contain_thres=0.5).detect_frames(frames)),
          _reference(mini, frames, conf_thres, nms, [4], _const(SCALE), contain=0.5)[0])


def test_tiled_scale_callable_and_bordered_tile(mini, frames, conf_thres):
    """a scale per frame size: 1.0, and 0.4 for the 120 x 90 frame, which then is ONE tile between borders (offsets (-8, -14))"""
    from mdcv.yolo.detect import TiledFrameDetector
    nms = mini.get_threshs()[1]
    thres = conf_thres * 0.5                                                    # lower: the bordered tile keeps candidates too
    want, _ = _reference(mini, frames, thres, nms, [4], _by_size)
    got = list(TiledFrameDetector(mini, scale=_by_size, conf_thres=thres).detect_frames(frames))
    print("boxes per frame", [len(r.boxes) for r in got])
    _same(got, want)
    assert len(got[3].boxes) >= 1 and set(got[3].src[:, 0]) == {38}             # the single tile of the last frame
    assert (got[3].boxes[:, 2] > got[3].boxes[:, 0]).all()


def test_tiled_one_synchronisation_per_batch(mini, frames, conf_thres, monkeypatch):
    from mdcv.yolo.detect import TiledFrameDetector
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
    det = TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres, batch_size=2, tile_batch=7)
    list(det.detect_frames(frames))
    calls.clear()
    res = list(det.detect_frames(frames))
    print("synchronisations", calls, "boxes", sum(len(r.boxes) for r in res))
    assert len(calls) <= 2 and sum(len(r.boxes) for r in res) >= 4              # two batches: one each


@pytest.fixture(scope="module")
def kpnet():
    from mdcv.rektnet.keypoint_net import KeypointNet
    torch.manual_seed(7)
    return KeypointNet(7, (80, 80), precision="fp32").cuda().eval()


def test_tiled_frame_cone_detector(mini, kpnet, frames, conf_thres):
    """the tiled front, then the crop -> key-point -> draw chain held to its restatements as tests/test_gpu_kpt_detect.py holds it"""
    from mdcv.yolo.detect import FrameCones, TiledFrameConeDetector
    nms = mini.get_threshs()[1]
    bucket = 8
    want = _reference(mini, frames, conf_thres, nms, [3, 1], _const(SCALE))[0]
    det = TiledFrameConeDetector(mini, kpnet, scale=SCALE, conf_thres=conf_thres, batch_size=3, bucket=bucket)
    got = list(det.detect_frames(frames, return_crops=True))
    print("boxes per frame", [len(r.boxes) for r in got], "with a crop", [int(r.has_crop.sum()) for r in got])
    assert sum(int(r.has_crop.sum()) for r in got) >= 4 and all(isinstance(r, FrameCones) for r in got)
    for g, w in zip(got, want):                                                 # stage 1: the boxes are the tiled assembly's, bit for bit
        assert np.array_equal(g.boxes.view(np.int64), w["boxes"].view(np.int64)) and np.array_equal(g.rects, w["rects"])
        assert np.array_equal(g.prob, w["prob"]) and g.skipped == w["skipped"] and np.array_equal(g.src, w["src"])
    for lo, hi in ((0, 3), (3, 4)):
        fr, res = frames[lo:hi], got[lo:hi]
        rects = np.zeros((len(fr), max(max(len(r.rects) for r in res), 1), 4), np.int32)
        for b, r in enumerate(res):
            rects[b, :len(r.rects)] = r.rects
        count = np.array([len(r.rects) for r in res], np.int32)
        crops, owner, window, M = KD.crop_frames(fr, rects, count, det.max_cones, 80)
        pts = np.zeros((0, 7, 2), F)
        if M:
            batch = np.zeros(((M + bucket - 1) // bucket * bucket, 3, 80, 80), F)
            batch[:M] = crops
            with torch.no_grad():
                pts = kpnet(torch.from_numpy(batch).cuda())[1][:M].cpu().numpy()
        for b, r in enumerate(res):
            rows = np.nonzero(owner[:, 0] == b)[0]
            n = len(r.rects)
            has = np.zeros(n, bool)
            has[owner[rows, 1]] = True
            assert np.array_equal(r.has_crop, has)
            assert np.array_equal(r.crops.view(np.int32), crops[rows].view(np.int32))          # stage 2: cut from the ORIGINAL frame
            np.testing.assert_allclose(r.keypoints[has], pts[rows], atol=2e-4)                   # stage 3
            drawn = fr[b].copy()                                                                 # stage 4: outlines, then discs
            for rect in r.rects:
                if tuple(rect) != D.SKIPPED_RECT:
                    D.draw_rect(drawn, rect)
            skipped = 0
            for m, k in zip(rows, owner[rows, 1]):
                for i in range(7):
                    c = KD.center(r.keypoints[k, i], window[m])
                    if c is None:
                        skipped += 1
                        continue
                    assert tuple(r.keypoints_frame[k, i]) == c
                    KD.draw_disc(drawn, c[0], c[1], KD.COLOURS_RGB[i])
            assert r.skipped_points == skipped and np.array_equal(r.annotated, drawn)


def test_tiled_file_round_trip(mini, frames, conf_thres, tmp_path):
    from PIL import Image
    from mdcv.yolo import detect as DT
    nms = mini.get_threshs()[1]
    src, out1, out2 = tmp_path / "in", tmp_path / "single", tmp_path / "dir"
    for d in (src, out1, out2):
        os.makedirs(d)
    names = [f"frame_{i}.png" for i in range(len(frames))]
    for n, f in zip(names, frames):
        Image.fromarray(f).save(src / n)
    whole = list(DT.TiledFrameDetector(mini, scale=SCALE, conf_thres=conf_thres).detect_frames(frames))
    assert sum(len(r.boxes) for r in whole) >= 4
    paths = DT.detect(str(src), str(out2), mini, "cuda:0", conf_thres, nms, tiles=True, scale=SCALE)
    assert paths == [os.path.join(str(out2), n) for n in names]
    for p, r in zip(paths, whole):
        assert np.array_equal(np.asarray(Image.open(p)), r.annotated)
    path = DT.single_img_detect(str(src / names[0]), str(out1), "image", mini, "cuda:0", conf_thres, nms, tiles=True, scale=SCALE)
    assert path == os.path.join(str(out1), names[0]) and np.array_equal(np.asarray(Image.open(path)), whole[0].annotated)
    # the defaults are the whole-frame detector's
    plain = list(DT.FrameDetector(mini, conf_thres=conf_thres, batch_size=1).detect_frames(frames[:1]))
    path = DT.single_img_detect(str(src / names[0]), str(out1), "image", mini, "cuda:0", conf_thres, nms)
    assert np.array_equal(np.asarray(Image.open(path)), plain[0].annotated)
