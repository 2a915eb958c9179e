"""Dataset-level AP, the host half (no GPU): the NumPy restatement of csrc/detmap.hip (tests/helpers/detmap_numpy.py) pinned on cases
whose answers are written out here, the committed fixture (tests/golden/detmap, written by tests/golden/make_golden_detmap.py), the
argument checks of the two C entry points, which run before anything touches a device, and DatasetAP's own max_images check."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import detmap_numpy as DM  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
F = np.float32
EARG = -1
INF = np.inf
FP, TP, IG = DM.FP, DM.TP, DM.IGNORED


def _run(images, thresholds=(0.5,), ranges=((0, INF),), C=1, K=4):
    """images: [(dets [(box, score, cls)], gts [(box, cls, ignore)])] -> (Dataset, q, tot, ap)"""
    ds = DM.Dataset(K, thresholds, ranges, C)
    for dets, gts in images:
        boxes, prob, cls = np.zeros((1, K, 4), F), np.zeros((1, K), F), np.zeros((1, K), np.int32)
        for k, (bx, sc, c) in enumerate(dets):
            boxes[0, k], prob[0, k], cls[0, k] = bx, sc, c
        T = max(len(gts), 1)
        gb, gc, gi = np.zeros((1, T, 4), F), np.zeros((1, T), np.int32), np.zeros((1, T), np.uint8)
        for t, (bx, c, ig) in enumerate(gts):
            gb[0, t], gc[0, t], gi[0, t] = bx, c, ig
        ds.add_pixels(boxes, prob, cls, [len(dets)], gb, gc, [len(gts)], gi)
    q, tot, ap, err = ds.finalize()
    assert err == 0
    return ds, q, tot, ap


def _status(ds, image, j=0, s=0):
    st, n = ds.status[image], ds.count[image]
    return [int(st[s, k] >> (2 * j)) & 3 for k in range(n)]


A, B = (0, 0, 10, 10), (20, 0, 30, 10)


def test_perfect_none_and_no_ground_truth():
    _, q, tot, ap = _run([([(A, 0.9, 0), (B, 0.8, 0)], [(A, 0, 0), (B, 0, 0)])])
    assert ap[0, 0, 0] == 1.0 and tuple(tot[0, 0, 0]) == (2, 2, 2) and (q[0, 0, 0] == (1, 1)).all()
    _, q, tot, ap = _run([([((50, 50, 60, 60), 0.9, 0)], [(A, 0, 0)])])
    assert ap[0, 0, 0] == 0.0 and tuple(tot[0, 0, 0]) == (1, 0, 1) and (q[0, 0, 0] == (0, 1)).all()
    _, q, tot, ap = _run([([(A, 0.9, 0)], [])])
    assert ap[0, 0, 0] == -1.0 and tuple(tot[0, 0, 0]) == (0, 0, 1)
    _, q, tot, ap = _run([([], [(A, 0, 0)])])                                  # ground truth and not one detection
    assert ap[0, 0, 0] == 0.0 and tuple(tot[0, 0, 0]) == (1, 0, 0)


def test_hand_worked_example():
    """image 0: ground truth A, B; detections .9 on A (TP), .8 elsewhere (FP), .6 on B (TP), .3 on A again (FP, A is used up).
    image 1: ground truth C, D; detections .7 on C (TP), .5 elsewhere (FP), .4 on C again (FP); D is missed.  n_gt = 4.
    By score: TP FP TP TP FP FP FP -> tp 1 1 2 3 3 3 3 over nd 1..7; precision 1, 1/2, 2/3, 3/4, 3/5, 1/2, 3/7; envelope 1, 3/4, 3/4, 3/4, 3/5,
    1/2, 3/7.  Recall k/100 needs 100 tp >= 4 k: k <= 25 at the first row (envelope 1), k <= 50 at the third (3/4), k <= 75 at the fourth
    (3/4), beyond: never.  AP = (26 + 50 * 3/4) / 101 = 127 / 202."""
    z = np.load(os.path.join(G, "detmap", "cases.npz"))
    ds = DM.Dataset(4, [0.5], [(0, INF)], 1)
    ds.add_pixels(z["hand::boxes"], z["hand::prob"], None, z["hand::count"], z["hand::gt_boxes"], None, z["hand::gt_count"])
    assert _status(ds, 0) == [TP, FP, TP, FP] and _status(ds, 1) == [TP, FP, FP]
    slots, classes, err = DM.sorted_slots(*ds.buffers()[:3], 1)
    assert slots == [0, 1, 4, 2, 5, 6, 3] and err == 0
    q, tot, ap, _ = ds.finalize()
    want = [Fraction(1)] * 26 + [Fraction(3, 4)] * 50 + [Fraction(0)] * 25
    assert [Fraction(int(n), int(d)) for n, d in q[0, 0, 0]] == want
    assert [(int(n), int(d)) for n, d in q[0, 0, 0]] == [(f.numerator, f.denominator) for f in want]      # lowest terms, 0 as 0 / 1
    assert tuple(tot[0, 0, 0]) == (4, 3, 7)
    assert sum(want) / 101 == Fraction(127, 202)
    assert ap[0, 0, 0] == DM.ap_of(want, 4) and abs(ap[0, 0, 0] - 127 / 202) < 1e-15
    assert np.array_equal(q, z["hand::q"]) and np.array_equal(tot, z["hand::tot"])
    assert np.array_equal(ap.view(np.int64), z["hand::ap"].view(np.int64))
    assert np.array_equal(ds.buffers()[3], z["hand::status"])


def test_fixture_is_the_restatement():
    z = np.load(os.path.join(G, "detmap", "cases.npz"))
    b = {k: z["smoke::" + k] for k in ("boxes", "prob", "cls", "count", "gt_boxes", "gt_cls", "gt_ignore", "gt_count")}
    ds = DM.Dataset(16, z["smoke::thresholds"], z["smoke::ranges"], 3)
    ds.add_pixels(**b)
    q, tot, ap, err = ds.finalize()
    assert err == 0 and np.array_equal(ds.buffers()[3], z["smoke::status"]) and np.array_equal(ds.n_gt, z["smoke::n_gt"])
    assert np.array_equal(q, z["smoke::q"]) and np.array_equal(tot, z["smoke::tot"])
    assert np.array_equal(ap.view(np.int64), z["smoke::ap"].view(np.int64))
    assert np.array_equal(z["smoke::thresholds"], np.array(DM.COCO_THRESHOLDS, F)) and z["smoke::thresholds"][0] == F(0.5)
    assert os.path.getsize(os.path.join(G, "detmap", "cases.npz")) < 32768


def test_equal_iou_takes_the_higher_index():
    """the first detection overlaps G0 and G1 by the same 60 / 140: it takes G1, so the second, which sits on G1, finds it used up
    (its IoU with G0 is 20 / 180) and is a false positive; had the lower index won it would have been a second true positive"""
    G0, G1 = (0, 0, 10, 10), (8, 0, 18, 10)
    assert DM.iou32((4, 0, 14, 10), G0) == DM.iou32((4, 0, 14, 10), G1) == F(60) / F(140)
    ds, _, tot, _ = _run([([((4, 0, 14, 10), 0.9, 0), (G1, 0.8, 0)], [(G0, 0, 0), (G1, 0, 0)])], thresholds=(0.4,))
    assert _status(ds, 0) == [TP, FP] and tuple(tot[0, 0, 0]) == (2, 1, 2) and ds.stats["ties"] == 1


def test_equal_scores_are_ordered_by_image_then_row():
    hit, miss = ([(A, 0.5, 0)], [(A, 0, 0)]), ([((50, 50, 60, 60), 0.5, 0)], [])
    _, q, _, ap = _run([miss, hit])                                            # FP first: precision 1 / 2 at recall 1
    assert ap[0, 0, 0] == 0.5 and (q[0, 0, 0] == (1, 2)).all()
    _, q, _, ap = _run([hit, miss])
    assert ap[0, 0, 0] == 1.0
    _, _, _, ap = _run([([((50, 50, 60, 60), 0.5, 0), (A, 0.5, 0)], [(A, 0, 0)])])   # inside an image: by row
    assert ap[0, 0, 0] == 0.5


def test_ground_truth_ignored_by_flag():
    ds, _, tot, ap = _run([([(A, 0.9, 0)], [(A, 0, 1)])])
    assert _status(ds, 0) == [IG] and ap[0, 0, 0] == -1.0 and tuple(tot[0, 0, 0]) == (0, 0, 0)
    ds, _, tot, ap = _run([([(A, 0.9, 0), (B, 0.8, 0)], [(A, 0, 1), (B, 0, 0)])])
    assert _status(ds, 0) == [IG, TP] and ap[0, 0, 0] == 1.0 and tuple(tot[0, 0, 0]) == (1, 1, 1)


def test_ground_truth_ignored_by_area():
    """area 100 is outside [0, 50): in that range the ground truth does not count and its detection is neither TP nor FP"""
    ds, _, tot, ap = _run([([(A, 0.9, 0)], [(A, 0, 0)])], ranges=((0, INF), (0, 50), (100, 101), (50, 100)))
    assert [_status(ds, 0, s=s) for s in range(4)] == [[TP], [IG], [TP], [IG]]                # [lo, hi): 100 is in [100, 101), not in [50, 100)
    assert list(ap[0, 0]) == [1.0, -1.0, 1.0, -1.0] and list(tot[0, 0, :, 0]) == [1, 0, 1, 0]


def test_unmatched_detection_outside_the_range_is_ignored():
    small, big = (50, 50, 55, 55), (60, 60, 70, 70)                             # areas 25 and 100, both on nothing
    ds, _, tot, ap = _run([([(small, 0.9, 0), (big, 0.8, 0), ((0, 0, 4, 4), 0.7, 0)], [((0, 0, 4, 4), 0, 0)])], ranges=((0, INF), (0, 50)))
    assert _status(ds, 0, s=0) == [FP, FP, TP] and _status(ds, 0, s=1) == [FP, IG, TP]
    assert tuple(tot[0, 0, 0]) == (1, 1, 3) and tuple(tot[0, 0, 1]) == (1, 1, 2)
    assert ap[0, 0, 0] == DM.ap_of([Fraction(1, 3)] * 101, 1) and ap[0, 0, 1] == 0.5


def test_fall_back_to_an_ignored_ground_truth():
    """G0 and the flagged G1 are the same box: the first detection takes G0 although G1 has the higher index (a non-ignored ground truth
    goes first), the second finds only G1 and is IGNORED, the third finds nothing and is a false positive"""
    ds, _, tot, ap = _run([([(A, 0.9, 0), (A, 0.8, 0), (A, 0.7, 0)], [(A, 0, 0), (A, 0, 1)])])
    assert _status(ds, 0) == [TP, IG, FP] and tuple(tot[0, 0, 0]) == (1, 1, 2) and ap[0, 0, 0] == 1.0
    assert ds.stats["fallback"] == 1
    ds, *_ = _run([([(A, 0.9, 1)], [(A, 0, 0)])], C=2)                          # another class: no match at all
    assert _status(ds, 0) == [FP]


def test_true_positives_equal_a_sort_all_pairs_matcher():
    """J = 1, S = 1, one class, no ties: every (detection, ground truth) pair with IoU >= 0.5 from a float64 IoU, sorted by detection row
    and then descending IoU; a pair is taken when both ends are free"""
    rng = np.random.default_rng(5)
    n_tp = 0
    for _ in range(20):
        K, T = 24, 10
        c, s = rng.uniform(0, 64, (T, 2)), rng.uniform(8, 24, (T, 2))
        gt = np.concatenate([c - s / 2, c + s / 2], 1).astype(F)
        pick = rng.integers(0, T, K)
        det = (gt[pick] + rng.normal(0, 2.5, (K, 4))).astype(F)
        det[:, 2:] = np.maximum(det[:, 2:], det[:, :2] + 1)
        st, n_gt = DM.match_image(det, None, K, gt, None, None, [F(0.5)], [(F(0), F(INF))], 1)
        d64, g64 = det.astype(np.float64), gt.astype(np.float64)
        pairs = []
        for d in range(K):
            for t in range(T):
                iw = min(d64[d, 2], g64[t, 2]) - max(d64[d, 0], g64[t, 0])
                ih = min(d64[d, 3], g64[t, 3]) - max(d64[d, 1], g64[t, 1])
                inter = max(iw, 0) * max(ih, 0)
                iou = inter / ((d64[d, 2] - d64[d, 0]) * (d64[d, 3] - d64[d, 1]) + (g64[t, 2] - g64[t, 0]) * (g64[t, 3] - g64[t, 1]) - inter)
                if iou >= 0.5:
                    pairs.append((d, -iou, t))
        tp, used = np.zeros(K, bool), set()
        for d, _, t in sorted(pairs):
            if not tp[d] and t not in used:
                tp[d] = True
                used.add(t)
        assert np.array_equal((st[0] & 3) == TP, tp) and n_gt[0, 0] == T
        n_tp += int(tp.sum())
    assert n_tp >= 100


def test_restatement_alone_is_not_vacuous():
    """the random cases of tests/test_gpu_detmap.py, counted on the CPU: every outcome, the fall-back and equal-IoU ties all occur"""
    rng = np.random.default_rng(1)
    ds = DM.Dataset(64, DM.COCO_THRESHOLDS[:3], [(0, INF), (0, 200), (200, 1e9)], 5)
    ds.add_pixels(**DM.random_batch(rng, 8, 64, 20, 5))
    s = ds.stats
    assert s["tp"] >= 50 and s["fp"] >= 50 and s["ignored"] >= 50 and s["fallback"] >= 20 and s["ties"] >= 10, s


# ------------------------------------------------------------------------------------------------ the entry points' argument checks
def _match_rc(L, K=8, T=4, J=1, S=1, C=1, first=0, cap=4, B=2, thr=(0.5,), ranges=((0, INF),), mode=0, out=1, width=64.0):
    thr, ranges = np.ascontiguousarray(thr, F), np.ascontiguousarray(ranges, F)
    o = out if out else None
    return L.detmap_match(None, None, None, None, B, K, mode, None, None, None, None, T, width, 64.0, thr.ctypes.data if thr.size else None, J,
                          ranges.ctypes.data if ranges.size else None, S, C, first, cap, o, o, o, o, o, None)


def test_match_argument_errors_need_no_device():
    """every rejected call returns before a pointer is read or anything is enqueued, so null (or dummy) device pointers are enough"""
    from mdcv import _lib
    L = _lib.lib()
    assert _match_rc(L) == EARG                                                 # all in range: the null detections are what is wrong
    assert _match_rc(L, B=0) == 0                                               # nothing to add is not an error
    for bad in (dict(K=0), dict(K=513), dict(T=-1), dict(T=2049), dict(J=0), dict(J=11, thr=(0.5,) * 11), dict(S=0), dict(S=5, ranges=((0, 1),) * 5),
                dict(C=0), dict(C=1025), dict(first=-1), dict(cap=0), dict(cap=1 << 40), dict(B=-1), dict(mode=2),
                dict(thr=(0.0,)), dict(thr=(1.5,)), dict(thr=(np.nan,)), dict(thr=()), dict(ranges=((2, 1),)), dict(ranges=((np.nan, 1),)),
                dict(ranges=()), dict(out=0), dict(mode=1, width=0.0)):
        assert _match_rc(L, **{**bad, "B": bad.get("B", 0)}) == EARG, bad           # wrong even with nothing to add
    assert _match_rc(L, first=2, B=0) == 0 and _match_rc(L, first=2, cap=4, B=3) == EARG     # first + B <= cap
    assert _match_rc(L, ranges=((1, 1),), B=0) == 0                             # lo == hi: an empty range, not an error


def test_finalize_argument_errors_need_no_device():
    from mdcv import _lib
    L = _lib.lib()

    def rc(n=2, cap=4, K=8, J=1, S=1, C=1, p=8, ws=8, nbytes=1 << 20):
        q = p if p else None
        return L.detmap_finalize(q, q, q, q, q, n, cap, K, J, S, C, q, q, q, q, ws if ws else None, nbytes, None)

    for bad in (dict(n=-1), dict(n=5), dict(cap=0), dict(K=0), dict(K=513), dict(J=0), dict(J=11), dict(S=0), dict(S=5), dict(C=0), dict(C=1025),
                dict(p=0), dict(ws=0), dict(ws=12), dict(nbytes=16), dict(nbytes=-1), dict(cap=1 << 40)):
        assert rc(**bad) == EARG, bad
    for bad in ((0, 8), (4, 0), (4, 513), (1 << 40, 8), (-1, 8)):
        assert L.detmap_finalize_workspace_bytes(*bad) == EARG, bad


def test_max_images_is_checked_on_the_host():
    import torch
    from mdcv.yolo import DatasetAP
    acc = DatasetAP(1, 3, top_k=4)
    z = lambda *s, **k: torch.zeros(*s, **k)       # noqa: E731
    with pytest.raises(ValueError, match="max_images"):
        acc.add_boxes(z(4, 4, 4), z(4, 4), None, z(4, dtype=torch.int32), z(4, 1, 4), None, z(4, dtype=torch.int32))
    acc.n_images = 2                                                            # the counter lives on the host
    with pytest.raises(ValueError, match="2 \\+ 2 images exceed max_images = 3"):
        acc.add_boxes(z(2, 4, 4), z(2, 4), None, z(2, dtype=torch.int32), z(2, 1, 4), None, z(2, dtype=torch.int32))
    for bad in (dict(top_k=513), dict(iou_thresholds=(0.0,)), dict(area_ranges=((2, 1),)), dict(area_ranges=((0, 1),) * 5), dict(max_images=0)):
        with pytest.raises(ValueError):
            DatasetAP(**{**dict(num_classes=1, max_images=3), **bad})
