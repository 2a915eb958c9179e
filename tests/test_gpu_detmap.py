"""Dataset-level AP on the device: mdcv_detmap_match and mdcv_detmap_finalize (csrc/detmap.hip) through the C ABI against their NumPy
restatement (tests/helpers/detmap_numpy.py, itself pinned by tests/test_detmap_host.py), every output between guard words and compared
with ==: status words, n_gt, q, tot and the AP bit pattern; then mdcv.yolo.evaluate's DatasetAP / evaluate end to end."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detmap_numpy as DM  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
F = np.float32
GUARD, GW = 0x5A5A5A5A, 16
INF = np.inf
RANGES3 = ((0, INF), (0, 200), (200, 1e9))


def _guarded(words, fill=None):
    t = torch.full((GW + words + GW,), GUARD, dtype=torch.int32, device="cuda")
    if fill is not None:
        t[GW:GW + words] = fill
    return t


def _payload(t, words, dtype, shape):
    a = t.cpu().numpy()
    assert (a[:GW] == GUARD).all() and (a[GW + words:] == GUARD).all()          # nothing in front of or behind the output
    return a[GW:GW + words].view(dtype).reshape(shape)


def _dev(a, dtype):
    a = np.ascontiguousarray(a, dtype).reshape(-1)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).cuda()


class Raw:
    """the dataset buffers of the C ABI between guard words"""

    def __init__(self, cap, K, J, S, C):
        self.cap, self.K, self.J, self.S, self.C = cap, K, J, S, C
        self.score, self.cls, self.count = _guarded(cap * K), _guarded(cap * K), _guarded(cap)
        self.status, self.n_gt = _guarded(S * cap * K), _guarded(2 * S * C, fill=0)

    def ptr(self, t):
        return t.data_ptr() + 4 * GW

    def read(self):
        cap, K, S, C = self.cap, self.K, self.S, self.C
        return (_payload(self.score, cap * K, F, (cap, K)), _payload(self.cls, cap * K, np.int32, (cap, K)),
                _payload(self.count, cap, np.int32, (cap,)), _payload(self.status, S * cap * K, np.uint32, (S, cap, K)),
                _payload(self.n_gt, 2 * S * C, np.int64, (S, C)))

    def match(self, first, thr, ranges, batch=None, labels=None, side=64, no_cls=False):
        from mdcv import _lib
        L = _lib.lib()
        thr, ranges = np.ascontiguousarray(thr, F), np.ascontiguousarray(ranges, F)
        b = batch
        B, K = b["boxes"].shape[:2]
        d = dict(boxes=_dev(b["boxes"], F), prob=_dev(b["prob"], F), cls=None if no_cls else _dev(b["cls"], np.int32), count=_dev(b["count"], np.int32))
        if labels is None:
            T = b["gt_boxes"].shape[1]
            g = (_dev(b["gt_boxes"], F), None if no_cls else _dev(b["gt_cls"], np.int32), _dev(b["gt_ignore"], np.uint8), _dev(b["gt_count"], np.int32))
            mode = 0
        else:
            T = labels.shape[1]
            g, mode = (_dev(labels, F), None, None, None), 1
        p = lambda t: None if t is None else t.data_ptr()     # noqa: E731
        rc = L.detmap_match(p(d["boxes"]), p(d["prob"]), p(d["cls"]), p(d["count"]), B, K, mode, p(g[0]), p(g[1]), p(g[2]), p(g[3]), T,
                            float(side), float(side), thr.ctypes.data, len(thr), ranges.ctypes.data, len(ranges), self.C, first, self.cap,
                            self.ptr(self.score), self.ptr(self.cls), self.ptr(self.count), self.ptr(self.status), self.ptr(self.n_gt),
                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc


def _finalize(score, cls, count, status, n_gt, n_images, cap, K, J, S, C):
    """mdcv_detmap_finalize on device copies of the given buffers -> (q, tot, ap bits, err)"""
    from mdcv import _lib
    L = _lib.lib()
    nb = int(L.detmap_finalize_workspace_bytes(cap, K))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    n = C * J * S
    q, tot, ap, err = _guarded(2 * n * 202), _guarded(2 * n * 3), _guarded(2 * n), _guarded(1)
    d = [_dev(score, F), _dev(cls, np.int32), _dev(count, np.int32), _dev(status, np.uint32), _dev(n_gt, np.int64)]
    rc = L.detmap_finalize(*[t.data_ptr() for t in d], n_images, cap, K, J, S, C, q.data_ptr() + 4 * GW, tot.data_ptr() + 4 * GW,
                           ap.data_ptr() + 4 * GW, err.data_ptr() + 4 * GW, ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    return (_payload(q, 2 * n * 202, np.int64, (C, J, S, 101, 2)), _payload(tot, 2 * n * 3, np.int64, (C, J, S, 3)),
            _payload(ap, 2 * n, np.int64, (C, J, S)), int(_payload(err, 1, np.int32, (1,))[0]))


def _same_curves(got, want):
    q, tot, ap, err = want
    assert got[3] == err
    assert np.array_equal(got[1], tot)
    assert np.array_equal(got[0], q)
    assert np.array_equal(got[2], ap.view(np.int64))                            # the AP, bit for bit


# ------------------------------------------------------------------------------------------------------------- the match kernel
MATCH_CASES = [  # K, T, J, S, C, B
    (1, 0, 1, 1, 1, 3), (1, 1, 10, 3, 1, 5), (64, 1, 1, 1, 5, 4), (64, 63, 10, 1, 1, 4), (65, 64, 1, 3, 5, 4), (65, 65, 10, 3, 5, 4),
    (200, 64, 10, 3, 5, 4), (200, 130, 1, 3, 1, 3), (512, 65, 1, 1, 5, 3), (512, 130, 10, 3, 5, 2), (64, 20, 10, 3, 5, 8),
]


_EXPECTED = {}


def _expected(case):
    """the random batch of a case and the restatement's datasets for both ground-truth forms, computed once"""
    if case not in _EXPECTED:
        K, T, J, S, C, B = case
        rng = np.random.default_rng(1000 * K + T)
        thr, ranges = DM.COCO_THRESHOLDS[:J], RANGES3[:S]
        batch = DM.random_batch(rng, B, K, max(T, 1), C)
        if T == 0:
            batch["gt_count"][:] = 0
        labels = DM.labels_of(batch) if T else np.zeros((B, 0, 5), F)
        if B > 3 and T:
            labels[3] = 0                                                       # an image whose labels are all padding
        pix, lab = DM.Dataset(K, thr, ranges, C), DM.Dataset(K, thr, ranges, C)
        pix.add_pixels(**batch)
        lab.add_labels(batch["boxes"], batch["prob"], batch["cls"], batch["count"], labels, 64, 64)
        _EXPECTED[case] = (batch, labels, pix, lab)
    return _EXPECTED[case]


@pytest.mark.parametrize("K,T,J,S,C,B", MATCH_CASES)
def test_match_equals_the_restatement_in_both_forms(K, T, J, S, C, B):
    thr, ranges = DM.COCO_THRESHOLDS[:J], RANGES3[:S]
    batch, labels, pix, lab = _expected((K, T, J, S, C, B))
    assert (batch["count"] == 0).any()                                          # images without a detection
    cap, first = B + 3, 2
    for form, want in (("pixels", pix), ("labels", lab)):
        raw = Raw(cap, K, J, S, C)
        rc = raw.match(first, thr, ranges, batch, labels=labels if (form == "labels" or T == 0) else None)
        assert rc == 0
        score, cls, count, status, n_gt = raw.read()
        w_score, w_cls, w_count, w_status, w_ngt = want.buffers()
        assert np.array_equal(n_gt, w_ngt), (form, n_gt, w_ngt)
        assert np.array_equal(count[first:first + B], w_count)
        assert np.array_equal(status[:, first:first + B], w_status), form
        assert np.array_equal(score[first:first + B].view(np.int32), w_score.view(np.int32)) and np.array_equal(cls[first:first + B], w_cls)
        for a in (score, cls, status.transpose(1, 0, 2)):                       # the other images' rows are not touched
            assert (a[:first].view(np.int32) == GUARD).all() and (a[first + B:].view(np.int32) == GUARD).all()
        assert (count[:first] == GUARD).all() and (count[first + B:] == GUARD).all()
        if C > 1:
            assert not n_gt[:, C - 1].any()                                     # the empty class
        # the curves of this dataset, from the kernel's own buffers
        got = _finalize(score[first:first + B], cls[first:first + B], count[first:first + B], status[:, first:first + B], n_gt, B, B, K, J, S, C)
        _same_curves(got, want.finalize())


def test_match_cases_are_not_vacuous():
    """over the random cases above (the restatement's own counts; the kernel equals it case by case): every outcome, the fall-back to an
    ignored ground truth and equal-IoU ties all occur"""
    seen = {}
    for case in MATCH_CASES:
        for ds in _expected(case)[2:]:
            for k, v in ds.stats.items():
                seen[k] = seen.get(k, 0) + v
    print("outcomes over the random cases", seen)
    assert seen["tp"] >= 50 and seen["fp"] >= 50 and seen["ignored"] >= 50 and seen["fallback"] >= 20 and seen["ties"] >= 10, seen


def test_match_without_class_arrays_is_class_zero():
    rng = np.random.default_rng(3)
    batch = DM.random_batch(rng, 4, 64, 9, 1)
    want = DM.Dataset(64, DM.COCO_THRESHOLDS, RANGES3, 1)
    want.add_pixels(batch["boxes"], batch["prob"], None, batch["count"], batch["gt_boxes"], None, batch["gt_count"], batch["gt_ignore"])
    raw = Raw(4, 64, 10, 3, 1)
    assert raw.match(0, DM.COCO_THRESHOLDS, RANGES3, batch, no_cls=True) == 0
    score, cls, count, status, n_gt = raw.read()
    assert np.array_equal(status, want.buffers()[3]) and np.array_equal(n_gt, want.n_gt) and not cls.any()


def test_match_rejected_calls_write_nothing():
    rng = np.random.default_rng(4)
    batch = DM.random_batch(rng, 2, 8, 4, 1)
    raw = Raw(3, 8, 1, 1, 1)
    assert raw.match(2, [0.5], [(0, INF)], batch) == -1                         # first + B > cap
    assert raw.match(0, [0.5], [(2, 1)], batch) == -1
    for a in raw.read()[:4]:
        assert (a.view(np.int32) == GUARD).all()
    assert not raw.read()[4].any()


# ------------------------------------------------------------------------------------------------------------------ the curves
def _synthetic_dataset(rng, lengths, K, J, S, n_gt_of, all_ignored=None):
    """dataset buffers built by hand: class c owns lengths[c] valid rows scattered over the images; scores are multiples of 1/64, so equal
    scores occur across images and inside them; statuses are random"""
    C, total = len(lengths), sum(lengths)
    n = (total + K - 1) // K + 1
    score, cls = np.zeros((n, K), F), np.full((n, K), C + 3, np.int32)          # a row of no class is left out
    count = np.full(n, K, np.int32)
    count[-1] = K // 2
    valid = [(i, k) for i in range(n) for k in range(int(count[i]))]
    assert len(valid) >= total
    order = rng.permutation(len(valid))[:total]
    labels = np.concatenate([np.full(l, c) for c, l in enumerate(lengths)]).astype(int)
    for o, c in zip(order, labels):
        cls[valid[o]] = c
    for i in range(n):
        score[i, :count[i]] = -np.sort(-rng.integers(1, 64, int(count[i]))) / F(64)
    status = np.zeros((S, n, K), np.uint32)
    for j in range(J):
        status |= rng.choice([DM.FP, DM.TP, DM.TP, DM.IGNORED], size=(S, n, K)).astype(np.uint32) << np.uint32(2 * j)
    if all_ignored is not None:
        status[:, cls == all_ignored] = sum(DM.IGNORED << (2 * j) for j in range(J))
    n_gt = np.array([[n_gt_of(c, s) for c in range(C)] for s in range(S)], np.int64)
    return score, cls, count, status, n_gt, n


def test_curves_around_the_chunk():
    """class segments of length 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1; n_gt of 3 (several recall levels share one true
    positive) and of 250 (true positives without a level); one segment all IGNORED; equal scores across images"""
    CH = DM.CHUNK
    lengths = [0, 1, CH - 1, CH, CH + 1, 2 * CH + 1, 40]
    rng = np.random.default_rng(9)
    K, J, S = 512, 2, 2
    score, cls, count, status, n_gt, n = _synthetic_dataset(rng, lengths, K, J, S, lambda c, s: (3, 250)[(c + s) % 2], all_ignored=6)
    assert len(set(score[0, :8]) & set(score[1, :count[1]])) > 0                # duplicated scores across images
    want = DM.finalize(score, cls, count, status, n_gt, J)
    assert [int((np.array(DM.sorted_slots(score, cls, count, len(lengths))[1]) == c).sum()) for c in range(len(lengths))] == lengths
    got = _finalize(score, cls, count, status, n_gt, n, n, K, J, S, len(lengths))
    _same_curves(got, want)
    tot = got[1]
    assert (tot[6, :, :, 1:] == 0).all() and (got[0][6, ..., 0] == 0).all()     # all IGNORED: no detection counts
    assert (tot[0, :, :, 1:] == 0).all() and tot[5, 0, 0, 2] > CH
    q = got[0][5, 0, 0]
    assert len({tuple(p) for p in q}) > 3                                       # a curve with several steps


def test_curves_small_n_gt_shares_levels_and_bad_scores_set_the_error_word():
    rng = np.random.default_rng(10)
    K, J, S = 8, 1, 1
    score, cls, count, status, n_gt, n = _synthetic_dataset(rng, [12, 5], K, J, S, lambda c, s: 3)
    _same_curves(_finalize(score, cls, count, status, n_gt, n, n, K, J, S, 2), DM.finalize(score, cls, count, status, n_gt, J))
    _same_curves(_finalize(score, cls, count, status, n_gt, 0, n, K, J, S, 2), DM.finalize(score[:0], cls[:0], count[:0], status[:, :0], n_gt, J))
    for bad in (0.0, -0.5, np.nan):
        s2 = score.copy()
        s2[0, 1] = bad
        got, want = _finalize(s2, cls, count, status, n_gt, n, n, K, J, S, 2), DM.finalize(s2, cls, count, status, n_gt, J)
        assert got[3] == 1 and want[3] == 1
        _same_curves(got, want)


# ------------------------------------------------------------------------------------------------------------------ whole path
def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def _add(acc, b, lo, hi):
    acc.add_boxes(_t(b["boxes"][lo:hi]), _t(b["prob"][lo:hi]), _t(b["cls"][lo:hi]), _t(b["count"][lo:hi]), _t(b["gt_boxes"][lo:hi]),
                  _t(b["gt_cls"][lo:hi]), _t(b["gt_count"][lo:hi]), _t(b["gt_ignore"][lo:hi]))


def _bits(r):
    return r.ap.view(np.int64).copy(), r.q.copy(), np.stack([r.tp, r.detections]), r.n_gt.copy()


def _same_result(a, b):
    for x, y in zip(_bits(a), _bits(b)):
        assert np.array_equal(x, y)


def test_dataset_ap_splits_reset_and_no_synchronisation():
    from mdcv.yolo import DatasetAP
    rng = np.random.default_rng(21)
    N, K, T, C = 21, 32, 9, 3
    b = DM.random_batch(rng, N, K, T, C)
    want = DM.Dataset(K, DM.COCO_THRESHOLDS, RANGES3, C)
    want.add_pixels(**b)
    q, tot, ap, _ = want.finalize()
    results = []
    for parts in (1, 3, 7):
        acc = DatasetAP(C, N + 1, top_k=K, area_ranges=RANGES3)
        step = N // parts
        for i in range(parts):
            _add(acc, b, i * step, (i + 1) * step)
        results.append(acc.result())
        assert acc.n_images == N
    for r in results:
        assert np.array_equal(r.ap.view(np.int64), ap.view(np.int64)) and np.array_equal(r.q, q)
        assert np.array_equal(r.tp, tot[..., 1]) and np.array_equal(r.detections, tot[..., 2]) and np.array_equal(r.n_gt, tot[:, 0, :, 0])
        _same_result(r, results[0])
    r = results[0]
    assert r.ap.shape == (C, 10, 3) and (r.ap[C - 1] == -1).all() and np.isnan(r.ap_per_class[C - 1]).all()
    have = tot[:C - 1, :, 0, 0] > 0
    assert have.all() and abs(r.AP - np.mean([ap[c, :, 0].mean() for c in range(C - 1)])) < 1e-12        # means over classes with ground truth
    assert abs(r.AP50 - np.mean(ap[:C - 1, 0, 0])) < 1e-12 and 0 < r.AP <= 1 and 0 < r.AP50 <= 1
    assert np.allclose(r.max_recall[:C - 1], tot[:C - 1, ..., 1] / tot[:C - 1, ..., 0]) and np.isnan(r.max_recall[C - 1]).all()
    assert r.precision.shape == (C, 10, 3, 101) and "AP50" in r.summary()
    # reset, then the same images again (other batch sizes): the same bits; and no add synchronises
    acc.reset()
    assert acc.n_images == 0
    staged = [(lo, min(lo + 5, N)) for lo in range(0, N, 5)]
    tensors = {k: _t(v) for k, v in b.items()}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for lo, hi in staged:
            acc.add_boxes(tensors["boxes"][lo:hi], tensors["prob"][lo:hi], tensors["cls"][lo:hi], tensors["count"][lo:hi],
                          tensors["gt_boxes"][lo:hi], tensors["gt_cls"][lo:hi], tensors["gt_count"][lo:hi], tensors["gt_ignore"][lo:hi])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same_result(acc.result(), results[0])
    with pytest.raises(ValueError, match="max_images"):
        _add(acc, b, 0, 2)                                                      # 21 + 2 > 22
    assert acc.n_images == N


def test_dataset_ap_add_takes_detect_postprocess_and_label_rows():
    """`add` (label form) under the sync debug mode, against the restatement fed with what detect_postprocess returned"""
    from mdcv.yolo import DatasetAP
    from mdcv.yolo.postprocess import detect_postprocess
    v = np.load(os.path.join(G, "post_validate_c.npz"))
    args = (float(v["conf_thres"]), float(v["nms_thres"]), float(v["iou_thres"]), float(v["width"]), float(v["height"]))
    out, tg = torch.from_numpy(v["out"]).cuda(), torch.from_numpy(v["targets"]).cuda()
    C = out.shape[2] - 5
    det = detect_postprocess(out, tg, *args)
    acc = DatasetAP(max(C, 1), out.shape[0], area_ranges=((0, INF), (0, 1024), (1024, INF)))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc.add(det, tg, args[3], args[4])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    r = acc.result()
    want = DM.Dataset(200, DM.COCO_THRESHOLDS, ((0, INF), (0, 1024), (1024, INF)), max(C, 1))
    want.add_labels(det.boxes.cpu().numpy(), det.prob.cpu().numpy(), det.cls.cpu().numpy(), det.count.cpu().numpy(), v["targets"], args[3], args[4])
    q, tot, ap, err = want.finalize()
    print("detections", int(det.count.sum()), "outcomes", want.stats, "AP", r.AP, "AP50", r.AP50)
    assert err == 0 and want.stats.get("tp", 0) > 0
    assert np.array_equal(r.ap.view(np.int64), ap.view(np.int64)) and np.array_equal(r.q, q) and np.array_equal(r.n_gt, tot[:, 0, :, 0])


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


def test_evaluate_returns_validates_tuple_and_the_assembled_dataset_ap(mini, monkeypatch):
    from mdcv.data.synth import SyntheticCones
    from mdcv.yolo import DatasetAP
    from mdcv.yolo.evaluate import evaluate
    from mdcv.yolo.postprocess import detect_postprocess
    from mdcv.yolo.validate import validate
    W, H = mini.img_size()
    loader = lambda: SyntheticCones(4, H, W, 8, 1, batches=3, seed=5)            # noqa: E731
    with torch.no_grad():                                                       # a threshold that leaves the first batch some candidates
        obj = mini(loader().batch(0)[1])[..., 4].flatten()
    monkeypatch.setattr(mini, "conf_thresh", float(obj.topk(40).values[-1]))
    with contextlib.redirect_stdout(io.StringIO()) as text:
        (m_ap, m_r, m_p, _), res = evaluate(dataloader=loader(), model=mini, device=torch.device("cuda"))
    lines = text.getvalue().strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("mAP:") and lines[1].startswith("AP@[0.50:0.95]") and "AP50" in lines[1]
    with contextlib.redirect_stdout(io.StringIO()):
        v_ap, v_r, v_p, _ = validate(dataloader=loader(), model=mini, device=torch.device("cuda"))
    same = lambda a, b: a == b or (a != a and b != b)                           # noqa: E731
    assert same(m_ap, v_ap) and same(m_r, v_r) and same(m_p, v_p)
    conf, nms, iou = mini.get_threshs()
    acc = DatasetAP(mini.get_num_classes(), 12, area_ranges=res.area_ranges)
    n_det = 0
    with torch.no_grad():
        for _, imgs, tg in loader():
            det = detect_postprocess(mini(imgs), tg, conf, nms, iou, W, H)
            acc.add(det, tg, W, H)
            n_det += int(det.count.sum())
    r = acc.result()
    print("detections", n_det, "n_gt", r.n_gt.tolist(), "AP", r.AP)
    assert res.n_images == 12 and r.n_gt[0, 0] > 0 and len(res.area_ranges) == 4 and n_det > 0
    _same_result(res, r)


def test_add_frames_equals_add_boxes_on_the_same_arrays(mini):
    from mdcv.yolo import DatasetAP
    from mdcv.yolo.detect import TiledFrameDetector
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    frames = [np.ascontiguousarray(z[k]) for k in sorted(z.files)]
    scale = 1.5
    for conf in (0.5, 0.3, 0.1, 0.03, 0.01, 0.003):                             # the first threshold that leaves boxes to score
        results = list(TiledFrameDetector(mini, scale=scale, conf_thres=conf).detect_frames(frames))
        n = [len(r.boxes) for r in results]
        if sum(n) >= 8:
            break
    assert sum(n) >= 8
    rng = np.random.default_rng(6)
    labels, ignore = [], []
    for r in results:                                                           # labels in FRAME pixels: some of the boxes, moved a little
        take = r.boxes[::2] / scale
        labels.append(take + rng.integers(-1, 2, take.shape))
        ignore.append(rng.random(len(take)) < 0.25)
    labels[1], ignore[1] = np.zeros((0, 4)), np.zeros(0, bool)                  # a frame without a label
    ranges = ((0, INF), (0, 400))
    a = DatasetAP(1, 4, area_ranges=ranges)
    a.add_frames(results[:3], labels[:3], scale=scale, ignore=ignore[:3])
    a.add_frames(results[3:], labels[3:], scale=scale, ignore=ignore[3:])
    ra = a.result()
    boxes, prob, count, gt, gt_count, gt_ignore = DatasetAP.pack_frames(results, labels, 200, scale, ignore)
    assert gt.dtype == F and np.array_equal(gt[0, :len(labels[0])], (labels[0] * scale).astype(F))          # float64 product, one rounding
    b = DatasetAP(1, 4, area_ranges=ranges)
    b.add_boxes(_t(boxes), _t(prob), None, _t(count), _t(gt), None, _t(gt_count), _t(gt_ignore))
    rb = b.result()
    _same_result(ra, rb)
    want = DM.Dataset(200, DM.COCO_THRESHOLDS, ranges, 1)
    want.add_pixels(boxes, prob, None, count, gt, None, gt_count, gt_ignore)
    q, tot, ap, _ = want.finalize()
    print("boxes per frame", n, "outcomes", want.stats, "AP50", ra.AP50)
    assert np.array_equal(ra.ap.view(np.int64), ap.view(np.int64)) and np.array_equal(ra.q, q) and want.stats.get("tp", 0) > 0


def test_command_line_scores_frames_against_a_csv(mini, tmp_path, monkeypatch, capsys):
    """python -m mdcv.yolo.evaluate --frames DIR --labels CSV --tiles: the CSV layout ImageLabelBatches reads (boxes x, y, h, w in frame
    pixels), scored as evaluate_frames scores the same frames and labels"""
    import csv
    import json
    from PIL import Image
    from mdcv.yolo import evaluate as E
    from mdcv.yolo.detect import TiledFrameDetector
    z = np.load(os.path.join(G, "imgload", "frames.npz"))
    frames = [np.ascontiguousarray(z[k]) for k in sorted(z.files)]
    scale = 1.5
    for conf in (0.5, 0.3, 0.1, 0.03, 0.01, 0.003):
        results = list(TiledFrameDetector(mini, scale=scale, conf_thres=conf).detect_frames(frames))
        if sum(len(r.boxes) for r in results) >= 8:
            break
    os.makedirs(tmp_path / "frames")
    rows, labels = [["anchors"], ["name", "", "width", "height", "scale"]], []
    for i, (f, r) in enumerate(zip(frames, results)):
        Image.fromarray(f).save(tmp_path / "frames" / f"f{i}.png")
        b = np.clip(np.round(r.boxes[::3] / scale), 0, None)                    # every third box, in frame pixels, whole numbers
        xyhw = [[float(x0), float(y0), float(y1 - y0), float(x1 - x0)] for x0, y0, x1, y1 in b]
        labels.append(np.array([[x, y, x + w, y + h] for x, y, h, w in xyhw], np.float64).reshape(-1, 4))
        rows.append([f"f{i}.png", "", f.shape[1], f.shape[0], 1.0] + [json.dumps(c) for c in xyhw])
    with open(tmp_path / "labels.csv", "w", newline="") as fh:
        csv.writer(fh).writerows(rows)
    monkeypatch.chdir(os.path.join(G, "mini"))
    res = E.main(["--model_cfg", "mini.cfg", "--weights_path", "mini.weights", "--frames", str(tmp_path / "frames"), "--labels",
                  str(tmp_path / "labels.csv"), "--tiles", "--scale", str(scale), "--conf_thres", str(conf), "--precision", "fp32"])
    out = capsys.readouterr().out
    assert out.strip().splitlines()[-1].startswith("AP@[0.50:0.95]") and res.n_images == 4 and res.n_gt[0, 0] == sum(len(l) for l in labels)
    want = E.evaluate_frames(frames, labels, TiledFrameDetector(mini, scale=scale, conf_thres=conf), scale=scale, area_ranges=res.area_ranges)
    _same_result(res, want)
    assert res.AP50 > 0
