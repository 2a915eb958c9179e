"""mdcv_detect_merge_tiles_soft (csrc/detect_tiles_soft.hip) through the C ABI: hard `==` the two existing merges, linear `==` the
float32 restatement (tests/helpers/softtiles_numpy.py), linear and Gaussian against float64 (order `==`, a score decayed d times within
2 d 2^-23, the restatement's own decisions clearing four times that); the named cases; the tiled detector end to end."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_draw_numpy as D  # noqa: E402
import softtiles_numpy as ST  # noqa: E402
from test_gpu_detect_tiles import GW, _guarded, _payload, _tiles_of, mini  # noqa: E402,F401
from test_gpu_mctiles import OUTS, launch as old_merge, same  # noqa: E402

pytestmark = pytest.mark.gpu
F, I32, NMS, SIGMA, STHRES = np.float32, np.int32, 0.3, 0.5, 0.05
METHODS = {"hard": 0, "linear": 1, "gaussian": 2}
GRIDS = ((0, 0), (1, 1), (2, 1), (2, 2), (3, 3))          # B = 5: frames of 0, 1, 2, 4 and 9 tiles (tiles 0 | 1, 2 | 3..6 | 7..15)
# K, top_k, edge: frame 1 has 7 + edge candidates, frame 2 63 + edge, frame 3 511 + edge (K = 200), frame 4 more than 512 (the select runs)
CASES = [(1, 1, 0), (1, 65, 1), (64, 1, 2), (64, 65, 0), (64, 512, 1), (200, 1, 2), (200, 65, 0), (200, 65, 1), (200, 65, 2), (200, 512, 0),
         (200, 512, 1), (200, 512, 2)]


def batch(K, edge):
    b, p, c, cnt, tiles = ST.tiled_scene(900, 38, GRIDS, K, centres=300)
    want = np.minimum([7 + edge, 40, 23 + edge, 128, 128, 128, 127 + edge], K)
    assert (cnt[:7] >= want).all() and (K < 200 or cnt[7:].sum() - cnt[8] - cnt[9] > 512 + K)
    cnt[:7], cnt[8], cnt[9], cnt[10] = want, 0, -3, K + 5                       # a tile at 0, a negative count, one above K (its last slots: zeros)
    return b, p, c, cnt, tiles


def soft(b, p, c, cnt, tiles, B, overlap, contain, top_k, method, aware, sthres=STHRES):
    from mdcv import _lib                                                       # one call on guarded outputs -> {name: array}
    dev = [torch.from_numpy(np.ascontiguousarray(a, t).reshape(-1)).cuda() for a, t in ((b, F), (p, F), (c, I32), (cnt, I32), (tiles, I32))]
    outs = [(n, (B, top_k) + w, t) for n, w, t in OUTS] + [("count", (B,), I32)]
    bufs = {n: _guarded(int(np.prod(shape))) for n, shape, _t in outs}
    ptr = {n: t.data_ptr() + 4 * GW for n, t in bufs.items()}
    host = np.ascontiguousarray(tiles, I32)
    assert _lib.softtiles_lib().detect_merge_tiles_soft(
        dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr() if aware else None, dev[3].data_ptr(), host.ctypes.data, dev[4].data_ptr(),
        *b.shape[:2], B, overlap, contain, top_k, ptr["boxes"], ptr["prob"], ptr["cls"] if aware else None, ptr["src"], ptr["count"],
        METHODS[method], SIGMA, sthres, int(aware), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = {n: _payload(bufs[n], int(np.prod(shape)), t, shape) for n, shape, t in outs}
    if not aware:
        assert (got["cls"] == 0x5A5A5A5A).all()                                 # out_cls is not touched
        got["cls"] = np.zeros_like(got["cls"])
    return got


def close(got, want, decays, margin):
    assert margin > 4, margin                                                   # the float64 restatement is free of near-ties
    same({k: got[k] for k in ("boxes", "cls", "src", "count")}, {k: want[k] for k in ("boxes", "cls", "src", "count")})
    err = np.abs(got["prob"].astype(np.float64) - want["prob"])
    print("largest fraction of the bound", np.max(err[decays > 0] / (2 * decays * ST.EPS * want["prob"])[decays > 0], initial=0.0))
    assert (err <= 2 * decays * ST.EPS * np.abs(want["prob"])).all()


@pytest.mark.parametrize("K,top_k,edge", CASES)
def test_soft_merge_equals_the_restatement(K, top_k, edge):
    b, p, c, cnt, tiles = batch(K, edge)
    for aware in (False, True):
        args = (b, p, c, cnt, tiles, 5, NMS, 0.6, top_k)
        old = old_merge(*args, agnostic=not aware)                              # hard: the existing merges, every output tensor
        same({k: v for k, v in soft(*args, "hard", aware).items() if k in old}, old)
        ref = (b, p, c if aware else None, cnt, tiles, 5, NMS, 0.6, top_k)
        got = soft(*args, "linear", aware)
        want = ST.merge(*ref, "linear", SIGMA, STHRES, F)[0]
        same(got, want)                                                         # linear, float32: every output tensor
        assert got["count"][0] == 0 and got["count"][1:].all() and (K < 200 or top_k < 512 or (got["count"][3:] > 64).all())
        for method in ("linear", "gaussian"):
            close(soft(*args, method, aware), *ST.merge(*ref, method, SIGMA, STHRES, np.float64))


def named():
    """six frames of two tiles 48 px apart: far cone inside near cone across tiles | in ONE tile | cut-off half | two classes | zero area | ties"""
    b, p, c = np.zeros((12, 2, 4), F), np.zeros((12, 2), F), np.zeros((12, 2), I32)
    b[0, 0], p[0, 0], b[1, 0], p[1, 0] = [100, 100, 160, 180], 0.95, [64, 100, 110, 160], 0.9
    b[2], p[2] = [[100, 100, 160, 180], [112, 100, 158, 160]], [0.95, 0.9]
    b[4, 0], p[4, 0], b[5, 0], p[5, 0] = [54, 20, 64, 40], 0.6, [6, 20, 26, 40], 0.9
    b[6, 0], p[6, 0], c[6, 0], b[7, 0], p[7, 0], c[7, 0] = [10, 10, 50, 60], 0.9, 1, [-38, 10, 2, 60], 0.8, 2
    b[8, 0], p[8, 0], b[9, 0], p[9, 0] = [30, 30, 30, 30], 0.9, [-18, 30, -18, 30], 0.8
    b[10], p[10], b[11], p[11] = [[0, 0, 8, 8], [20, 0, 28, 8]], 0.5, [[100, 0, 108, 8], [200, 0, 208, 8]], [0.5, 0.25]
    return b, p, c, np.array([1, 1, 2, 0, 1, 1, 1, 1, 1, 1, 2, 2], I32), np.array([[t // 2, 48 * (t % 2), 0, 0] for t in range(12)], I32)


@pytest.mark.parametrize("aware", (False, True))
@pytest.mark.parametrize("contain", (-1.0, 0.6))
def test_named_cases(contain, aware):
    b, p, c, cnt, tiles = named()
    got = {}
    for method in METHODS:
        for sthres in (STHRES, 0.7):
            g = got[method, sthres] = soft(b, p, c, cnt, tiles, 6, 0.55, contain, 4, method, aware, sthres)
            dt = np.float64 if method == "gaussian" else F
            want, decays, margin = ST.merge(b, p, c if aware else None, cnt, tiles, 6, 0.55, contain, 4, method, SIGMA, sthres, dt)
            close(g, want, decays, margin) if method == "gaussian" else same(g, want)
    seam, (h, l, g) = contain >= 0, (got[m, STHRES] for m in METHODS)
    assert h["count"].tolist() == [1, 1, 1 if seam else 2, 2 if aware else 1, 1, 4]                      # hard loses the far cone
    assert l["count"].tolist() == [1 if seam else 2, 2, 1 if seam else 2, 2 if aware else 1, 1 if seam else 2, 4]
    assert g["count"].tolist() == [1 if seam else 2, 2, 1 if seam else 2, 2 if aware or not seam else 1, 1 if seam else 2, 4]
    for s in (l, g):
        assert seam or (0.05 < s["prob"][0, 1] < 0.9 and s["src"][0, 1].tolist() == [1, 0])             # kept, with a decayed score
        assert s["prob"][1, :2].tolist() == [F(0.95), F(0.9)]                                           # ONE tile: not decayed again
        assert s["src"][5].tolist() == [[10, 0], [10, 1], [11, 0], [11, 1]] and (not aware or s["prob"][3, 1] == F(0.8))
    assert seam or (l["prob"][2, 1] == F(0.6) and g["prob"][2, 1] < F(0.6))                             # the half, kept without the seam rule
    assert got["linear", 0.7]["count"].tolist() == [1, 2, 1, 2 if aware else 1, 1 if seam else 2, 0]    # the scan stops midway


@pytest.mark.parametrize("aware", (False, True))
def test_tiled_soft_end_to_end(mini, aware, monkeypatch):
    from mdcv import _lib
    from mdcv.data import images as I
    from mdcv.yolo.detect import TiledFrameDetector
    from mdcv.yolo.postprocess import detect_postprocess
    rng = np.random.default_rng(37)
    net, (W, H), nms = mini, mini.img_size(), mini.get_threshs()[1]
    fr = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((100, 150, 3), (140, 90, 3))]
    geoms, own, tiles, _ = _tiles_of(fr, W, H, lambda w, h: 1.0)
    with torch.no_grad():
        pred = net(I.transform_batch([fr[f] for f in own], geoms, bw=net.get_bw()))
    s = -np.sort(-(pred[..., 4] * (pred[..., 5:].max(-1).values if aware else 1)).cpu().numpy(), axis=1)
    conf = float(((s[:, 2].astype(np.float64) + s[:, 3]) / 2).min())             # leaves every tile three candidates at least
    det = detect_postprocess(pred, None, conf, nms, 0.5, W, H, 200, class_aware=aware, nms="linear")
    boxes, prob, cls, count = (t.cpu().numpy() for t in (det.boxes, det.prob, det.cls, det.count))
    want = ST.merge(boxes, prob, cls if aware else None, count, tiles, 2, nms, 0.5, 200, "linear", 0.5, conf, F)[0]
    monkeypatch.setattr(_lib, "_softtiles", None)
    list(TiledFrameDetector(net, 1.0, conf_thres=conf, contain_thres=0.5).detect_frames(fr))
    assert _lib._softtiles is None                                              # the defaults never load the library
    calls, fn = [], _lib.softtiles_lib().detect_merge_tiles_soft
    monkeypatch.setattr(_lib.softtiles_lib(), "detect_merge_tiles_soft", lambda *a: (calls.append(a[17:21]), fn(*a))[1])
    got = list(TiledFrameDetector(net, 1.0, conf_thres=conf, contain_thres=0.5, nms="linear", class_aware=aware,
                                  tile_merge="soft_per_class" if aware else "soft").detect_frames(fr))
    assert calls == [(1, 0.5, conf, int(aware))] and want["count"].sum() >= 4 and len(np.unique(want["src"][..., 0])) > 2
    for f, r in enumerate(got):
        n = want["count"][f]
        assert len(r.boxes) == n and all(np.array_equal(getattr(r, k), want[k][f, :n]) for k in ("src", "prob"))
        assert (r.cls is None and not aware) or (r.cls.dtype == I32 and np.array_equal(r.cls, want["cls"][f, :n]))
        assert np.array_equal(r.boxes.view(np.int64), D.draw_boxes(fr[f], want["boxes"][f, :n], 1.0, 0, 0)[1].view(np.int64))
