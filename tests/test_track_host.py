"""Tracker, host half (no GPU): the restatement's assignment against brute force, its block-form filter against a plain 7x7 Kalman filter,
the conditions the GPU cases rest on, the ValueErrors, and that a detector with `track=` loads nothing until it runs."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import track_numpy as TN  # noqa: E402
from mdcv import _lib  # noqa: E402
from mdcv.yolo import track as TR  # noqa: E402


class Kalman7:
    """SORT's filter as plain matrices: x' = F x, P' = F P F^T + Q; K = P H^T (H P H^T + R)^-1, x += K y, P = (I - K H) P"""

    def __init__(self, z):
        self.F, self.H = np.eye(7), np.eye(4, 7)
        self.F[0, 4] = self.F[1, 5] = self.F[2, 6] = 1.0
        self.Q, self.R = np.diag([1, 1, 1, 1, 1e-2, 1e-2, 1e-4]), np.diag([1.0, 1, 10, 10])
        self.x, self.P = np.r_[z, 0.0, 0.0, 0.0], np.diag([10.0, 10, 10, 10, 1e4, 1e4, 1e4])

    def predict(self):
        if self.x[2] + self.x[6] <= 0:
            self.x[6] = 0.0
        self.x, self.P = self.F @ self.x, self.F @ self.P @ self.F.T + self.Q

    def update(self, z):
        K = self.P @ self.H.T @ np.linalg.inv(self.H @ self.P @ self.H.T + self.R)
        self.x, self.P = self.x + K @ (z - self.H @ self.x), (np.eye(7) - K @ self.H) @ self.P


@functools.lru_cache(None)
def filter_yardstick(steps=50, seed=39):
    """d: the worst difference of the predicted box between the block form and the 7x7 filter over `steps` frames of one seeded cone that
    moves, grows and is missed every seventh frame (coordinates of the test scenes' size) -- the rounding of a different operation order"""
    rng = np.random.default_rng(seed)
    box = np.array([900.0, 500.0, 960.0, 590.0])
    x, P = TN.new_filter(TN.measurement(box))
    full, d = Kalman7(TN.measurement(box)), 0.0
    for k in range(steps):
        box = box + np.array([7.0, -3.0, 8.5, -1.5]) + rng.normal(0, 1.5, 4)
        TN.block_predict(x, P)
        full.predict()
        d = max(d, float(np.abs(TN.state_box(x) - TN.state_box(full.x)).max()))
        if k % 7 != 6:
            TN.block_update(x, P, TN.measurement(box))
            full.update(TN.measurement(box))
    return d


@pytest.mark.parametrize("nr,n", [(1, 1), (3, 3), (6, 6), (2, 5), (4, 6), (5, 2), (6, 3)])
def test_assignment_total_equals_brute_force(nr, n):
    rng = np.random.default_rng([nr, n])
    for _ in range(20):
        cost = rng.choice([0, 3, 3, 7, 65535], (nr, n))                     # few values: many ties
        col, _, _ = TN.assign(cost)
        m = max(nr, n)
        full = np.full((m, m), TN.DUMMY, np.int64)                            # dummy rows add the same 65535 to every permutation
        full[:nr, :n] = cost
        assert sorted(col) == sorted(set(col)) and len(col) == nr
        best = min(sum(full[r, c] for r, c in enumerate(perm)) for perm in itertools.permutations(range(m)))
        assert sum(full[r, c] for r, c in enumerate(col)) + (m - nr) * TN.DUMMY == best


def test_block_filter_equals_the_7x7_filter():
    d = filter_yardstick()
    print("d =", d)
    assert 0.0 <= d <= 1e-10            # 50 steps at coordinates near 1e3 (ulp 2.3e-13): some hundred ulps at the very most


def test_cases_hold_what_they_are_for():
    a, d = TN.case("a")[4][0].solves, TN.case("d")[4][0].solves
    assert any(p >= 3 for _, _, p in a) and any(p >= 3 for _, _, p in d)     # an augmentation that re-assigns two or more earlier rows
    assert any(nr > n >= 64 and nr > 128 for nr, n, _ in d)                  # dummy columns in a lane's second and third register
    assert any(n > 192 and nr > 128 for nr, n, _ in d) and any(n == 0 for _, n, _ in a)
    assert TN.case("c")[4][0].dropped > 0 and ((TN.case("e")[6] & TN.BAD_BOX) != 0).sum() == 5


def test_bad_arguments_and_a_tracking_detector_loads_nothing(monkeypatch):
    from mdcv.yolo import detect as DT
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    monkeypatch.setattr(_lib, "_track", None)
    for kw in (dict(iou_thres=0.0), dict(iou_thres=1.5), dict(iou_thres=float("nan")), dict(max_age=-1), dict(min_hits=-1), dict(min_hits=1.5),
               dict(max_tracks=0), dict(max_tracks=257)):
        with pytest.raises(ValueError, match="TrackConfig"):
            TR.TrackConfig(**kw)
    with pytest.raises(ValueError, match="256 boxes"):
        DT.FrameDetector(net, top_k=300, max_boxes=300, track=True)
    with pytest.raises(ValueError, match="TrackConfig"):
        DT.FrameDetector(net, track="yes")
    for bad in (dict(boxes=torch.zeros(1, 2, 3, 4)), dict(count=torch.zeros(1, 3, dtype=torch.int32)), dict(cls=torch.zeros(1, 2, 3)), dict(config=3)):
        args = {**dict(boxes=torch.zeros(1, 2, 3, 4, dtype=torch.float64), count=torch.zeros(1, 2, dtype=torch.int32)), **bad}
        with pytest.raises(ValueError, match="track_boxes"):
            TR.track_boxes(**args)
    det = DT.FrameDetector(net, track=TR.TrackConfig(max_age=2))
    assert det.track.max_age == 2 and DT.FrameDetector(net, track=True).track.min_hits == 3 and DT.FrameDetector(net).track is None
    assert DT.TiledFrameDetector(net, 1.0, track=True).track.max_tracks == 256
    plan = DT.BatchPlan([(64, 48)], 32, 32, 200)
    assert plan.tid_off is None
    assert _lib._track is None and not any("mdcv_track" in line for line in open("/proc/self/maps"))     # building detectors loads nothing
