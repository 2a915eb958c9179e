"""mdcv_detect_merge_tiles_mc (csrc/detect_tiles_mc.hip) through the C ABI against the NumPy restatement of the agnostic merge
(tests/helpers/detect_tiles_numpy.py) used class by class, bit for bit, guard words around every output; then the tiled detector end to end."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_draw_numpy as D  # noqa: E402
import detect_tiles_numpy as TN  # noqa: E402
from test_gpu_detect_tiles import GW, _guarded, _payload, _tiles_of, frames, mini  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F, I32 = np.float32, np.int32
OUTS = (("boxes", (4,), F), ("prob", (), F), ("cls", (), I32), ("src", (2,), I32))
ROW = np.array([[0, 40 * i - 7, 0, 0] for i in range(4)], I32)             # one frame's tiles side by side, 24 px of overlap


def oracle(boxes, prob, cls, count, tiles, B, overlap, contain, top_k):
    """per frame: TN.merge_tiles's candidates and visiting order, TN.greedy_scan class by class, the union in visiting order"""
    out = {n: np.zeros((B, top_k) + w, t) for n, w, t in OUTS}
    out["src"], out["count"] = out["src"] - 1, np.zeros(B, I32)
    for b in range(B):
        ts = np.nonzero(tiles[:, 0] == b)[0]
        ns = [min(max(int(count[t]), 0), boxes.shape[1]) for t in ts]
        if not sum(ns):
            continue
        bx = np.concatenate([TN.offset_boxes(boxes[t, :n], tiles[t, 1], tiles[t, 2]) for t, n in zip(ts, ns)])
        pr, cl = (np.concatenate([a[t, :n] for t, n in zip(ts, ns)]) for a in (prob, cls))
        tile, slot = np.repeat(ts, ns), np.concatenate([np.arange(n) for n in ns])
        order = TN.visiting_order(pr, tile, slot, top_k)
        at = [np.nonzero(cl[order] == c)[0] for c in np.unique(cl[order])]
        keep = order[np.sort(np.concatenate([a[TN.greedy_scan(bx[order[a]], tile[order[a]], overlap, contain)] for a in at]))]
        n = out["count"][b] = len(keep)
        out["boxes"][b, :n], out["prob"][b, :n], out["cls"][b, :n], out["src"][b, :n] = bx[keep], pr[keep], cl[keep], np.stack([tile[keep], slot[keep]], 1)
    return out


def launch(boxes, prob, cls, count, tiles, B, overlap, contain, top_k, tiles_dev=None, agnostic=False):
    """one call on guarded outputs (tests/test_gpu_detect_tiles.py's) -> {name: array}; agnostic: mdcv_detect_merge_tiles on the same inputs"""
    from mdcv import _lib
    ins = [(boxes, F), (prob, F), (cls, I32), (count, I32), (tiles if tiles_dev is None else tiles_dev, I32)]
    dev = [torch.from_numpy(np.ascontiguousarray(a, t).reshape(-1)).cuda() for a, t in ins if not (agnostic and a is cls)]
    outs = [(n, (B, top_k) + w, t) for n, w, t in OUTS if not (agnostic and n == "cls")] + [("count", (B,), I32)]
    bufs = [_guarded(int(np.prod(shape))) for _, shape, _t in outs]
    fn = _lib.lib().detect_merge_tiles if agnostic else _lib.mctiles_lib().detect_merge_tiles_mc
    host = np.ascontiguousarray(tiles, I32)
    assert fn(*[d.data_ptr() for d in dev[:-1]], host.ctypes.data, dev[-1].data_ptr(), *boxes.shape[:2], B, float(overlap),
              float(contain), top_k, *[t.data_ptr() + 4 * GW for t in bufs], torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return {name: _payload(buf, int(np.prod(shape)), t, shape) for (name, shape, t), buf in zip(outs, bufs)}


def same(got, want, at=slice(None)):
    for name in want:
        assert np.array_equal(got[name][at].view(I32), want[name][at].view(I32)), (name, got["count"], want["count"])


def rand(rng, T, K, ncls, lo=4, hi=28, q=None):    # boxes in 64 x 64 tile coordinates in EVERY slot, scores descending per tile (q: with ties)
    c, s, p = rng.uniform(0, 64, (T, K, 2)), rng.uniform(lo, hi, (T, K, 2)), rng.uniform(0.05, 0.95, (T, K))
    p = -np.sort(-(p if q is None else np.round(p * q) / q).astype(F), axis=1)
    return np.concatenate([c - s / 2, c + s / 2], axis=2).astype(F), p, rng.integers(0, ncls, (T, K)).astype(I32)


def build(case, rng):                               # -> boxes, prob, cls, count, tiles, B, overlap, top_k, kept counts (seam rule off, on) or None
    if case == "mixed":                             # counts 0, above K and negative; confident rows past a count are no candidates
        b, p, c = rand(rng, 5, 8, 3, lo=16, hi=40)
        p[2], p[3] = 0.999, 0.999
        return b, p, c, [8, 11, 0, -3, 5], np.array([[0, 0, 0, 0], [0, 40, 0, 0], [0, 80, 0, 0], [1, -5, -9, 0], [1, 35, -9, 0]], I32), 2, 0.45, 16, None
    if case == "same_box":                          # the point: one box seen by two tiles, frame 0 with two classes, frame 1 with one
        b, p = np.zeros((4, 2, 4), F), np.zeros((4, 2), F)
        b[0::2, 0], b[1::2, 0], p[0::2, 0], p[1::2, 0] = [40, 10, 60, 30], [8.25, 10, 28.25, 30], 0.9, 0.8
        tiles = np.array([[0, 0, 0, 0], [0, 32, 0, 0], [1, 0, 0, 0], [1, 32, 0, 0]], I32)
        assert TN.merge_tiles(b, p, [1] * 4, tiles, 2, 0.5, -1.0, 8)[3].tolist() == [1, 1]       # the agnostic merge keeps fewer
        return b, p, np.array([[1, 0], [2, 0], [2, 0], [2, 0]], I32), [1] * 4, tiles, 2, 0.5, 8, ([2, 1], [2, 1])
    if case == "seam":                              # a cut-off half (IoU 0.5 < 0.6) inside the whole box another tile saw, per frame:
        b, p, c = np.zeros((6, 2, 4), F), np.zeros((6, 2), F), np.zeros((6, 2), I32)   # 0 same class, 1 other class, 2 same tile and class
        for t in (0, 2):
            b[t, 0], p[t, 0], b[t + 1, 0], p[t + 1, 0] = [54, 20, 64, 40], 0.6, [6, 20, 26, 40], 0.9
        b[5], p[5], c[2] = [[6, 20, 26, 40], [6, 20, 16, 40]], [0.9, 0.6], 4
        return b, p, c, [1, 1, 1, 1, 0, 2], np.array([[f, 48 * i, 0, 0] for f in range(3) for i in range(2)], I32), 3, 0.6, 8, ([2, 2, 2], [1, 2, 2])
    if case == "segments":                          # 256 candidates cut to 200, then 20 segments of lengths 70, 17 x 5, 44 and 1
        b, _, c = rand(rng, 4, 64, 3, lo=3, hi=14)
        p = -np.sort(-rng.permutation(256).reshape(4, 64).astype(F), axis=1) / F(256)  # distinct, so the 200 selected are known here
        sel = np.argsort(-p.reshape(-1), kind="stable")[:200]
        c.reshape(-1)[sel] = rng.permutation(np.repeat([-7] + list(range(1, 18)) + [100, 70000], [70] + [5] * 17 + [44, 1]).astype(I32))
        _, n = np.unique(c.reshape(-1)[sel], return_counts=True)
        assert len(n) > 16 and n.max() > 64 and n.min() == 1 and (((np.cumsum(n) - n) % 64 != 0) & (n > 1)).any() and c.min() < 0 and c.max() > 65535
        return b, p, c, [64] * 4, ROW, 1, 0.3, 200, None
    if case == "ties":                              # equal scores across tiles and slots in two classes; the cut falls inside a run
        return rand(rng, 3, 8, 2, lo=16, hi=40, q=32) + ([8, 8, 8], ROW[:3], 1, 0.5, 16, None)
    return rand(rng, 3, 512, 5, lo=3, hi=14) + ([512, 400, 512], ROW[:3], 1, 0.5, 512, None)        # "limit": 1536 candidates, 5 classes


@pytest.mark.parametrize("contain", [-1.0, 0.6])
@pytest.mark.parametrize("case", ["mixed", "same_box", "seam", "segments", "ties", "limit"])
def test_merge_mc_equals_the_class_by_class_restatement(case, contain):
    b, p, c, count, tiles, B, overlap, top_k, kept = build(case, np.random.default_rng(35))
    got = launch(b, p, c, count, tiles, B, overlap, contain, top_k)
    same(got, oracle(b, p, c, count, tiles, B, overlap, contain, top_k))
    assert kept is None or got["count"].tolist() == kept[contain >= 0]


@pytest.mark.parametrize("contain", [-1.0, 0.5])
def test_one_class_is_the_agnostic_merge(contain):
    b, p, _ = rand(np.random.default_rng(6), 5, 64, 1)
    args = (b, p, np.full((5, 64), -3, I32), [64, 30, 64, 0, 64], np.array([[0, 0, 0, 0], [0, 30, 0, 0], [0, 60, 0, 0], [1, 0, 0, 0], [1, 30, 0, 0]], I32), 2, 0.5, contain, 100)
    got, want = launch(*args), launch(*args, agnostic=True)
    same(got, want)
    assert want["count"].min() > 8 and all((got["cls"][f, :n] == -3).all() and not got["cls"][f, n:].any() for f, n in enumerate(got["count"]))


def test_the_device_table_is_checked_again():
    b, p, c = rand(np.random.default_rng(8), 5, 6, 3)
    count, tiles = [6] * 5, np.array([[0, 0, 0, 0], [0, 30, 0, 0], [1, 0, 0, 0], [1, 30, 0, 0], [2, 0, 0, 0]], I32)
    want, none = (oracle(b, p, c, n, tiles, 3, 0.5, -1.0, 8) for n in (count, [0] * 5))
    for empty, rows, words, values in (((0, 1), [1, 2], 0, [1, 0]), ((1,), 3, 1, 1 << 25), ((2,), 4, 3, 7)):      # scattered; offset; last word
        bad = tiles.copy()                          # a device copy that differs from the validated host copy: count 0, empty slots, out_cls too
        bad[rows, words] = values
        got = launch(b, p, c, count, tiles, 3, 0.5, -1.0, 8, tiles_dev=bad)
        same(got, none, list(empty))
        same(got, want, [f for f in range(3) if f not in empty])
    assert want["count"].min() > 0


def test_tiled_per_class_end_to_end(mini, frames, monkeypatch):
    """mini.cfg has one class, so this is plumbing: tiles -> detect_postprocess(class_aware=True) -> the restatement -> / scale; then whole frames"""
    from mdcv import _lib
    from mdcv.data import images as I
    from mdcv.yolo.detect import FrameDetector, TiledFrameDetector
    from mdcv.yolo.postprocess import detect_postprocess
    net, fr, (W, H), nms = mini, frames, mini.img_size(), mini.get_threshs()[1]

    def post(images, geoms):                        # -> a threshold that leaves every input three candidates, the detections at it
        with torch.no_grad():
            pred = net(I.transform_batch(images, geoms, bw=net.get_bw()))
        s = -np.sort(-(pred[..., 4] * pred[..., 5:].max(-1).values).cpu().numpy(), axis=1)
        conf = float(((s[:, 2].astype(np.float64) + s[:, 3]) / 2).min())
        return conf, detect_postprocess(pred, None, conf, nms, 0.5, W, H, 200, class_aware=True)
    geoms, own, tiles, _ = _tiles_of(fr, W, H, lambda w, h: 1.0)
    conf, det = post([fr[f] for f in own], geoms)
    want = oracle(*(t.cpu().numpy() for t in (det.boxes, det.prob, det.cls, det.count)), tiles, len(fr), nms, 0.5, 200)
    monkeypatch.setattr(_lib, "_mctiles", None)
    assert all(r.cls is None for r in TiledFrameDetector(net, 1.0, conf_thres=conf, contain_thres=0.5).detect_frames(fr)) and _lib._mctiles is None
    calls, fn = [], _lib.mctiles_lib().detect_merge_tiles_mc
    monkeypatch.setattr(_lib.mctiles_lib(), "detect_merge_tiles_mc", lambda *a: (calls.append(1), fn(*a))[1])
    got = list(TiledFrameDetector(net, 1.0, conf_thres=conf, contain_thres=0.5, class_aware=True, tile_merge="per_class").detect_frames(fr))
    assert calls == [1] and want["count"].sum() >= 4 and len(np.unique(want["src"][..., 0])) > 2
    for f, r in enumerate(got):
        n = want["count"][f]
        assert len(r.boxes) == n and r.cls.dtype == I32 and all(np.array_equal(getattr(r, k), want[k][f, :n]) for k in ("cls", "src", "prob"))
        assert np.array_equal(r.boxes.view(np.int64), D.draw_boxes(fr[f], want["boxes"][f, :n], 1.0, 0, 0)[1].view(np.int64))
    conf, det = post(fr, [I.sample_geometry(a.shape[1], a.shape[0], W, H, ts=False) for a in fr])
    cnt = det.count.cpu().numpy()
    for f, r in enumerate(FrameDetector(net, conf_thres=conf, class_aware=True).detect_frames(fr)):
        assert cnt[f] > 0 and len(r.boxes) == cnt[f] and r.cls.dtype == I32 and np.array_equal(r.cls, det.cls[f, :cnt[f]].cpu().numpy())
    assert all(r.cls is None for r in FrameDetector(net, conf_thres=conf).detect_frames(fr))
