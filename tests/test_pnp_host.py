"""Cone pose solver, host half (no GPU): the float64 restatement (tests/helpers/pnp_numpy.py) recovers every committed synthetic pose, the
model's ordering, the ValueErrors, and that a detector without a camera never loads the library."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pnp_numpy as PN  # noqa: E402
from mdcv import _lib  # noqa: E402
from mdcv.rektnet import pose as PO  # noqa: E402


@pytest.mark.parametrize("windows", (False, True))
def test_the_restatement_recovers_every_noise_free_case(windows):
    c, pose, info = PN.reference(0.0, windows)
    tilt = np.degrees(np.arccos(c["R"][:, 2, 2]))
    assert c["t"][:, 2].max() / c["t"][:, 2].min() > 3.9 and tilt.max() > 15 and (info[:, 0] == 0).all()      # a 4x span, tilts past 15 degrees
    rel = np.linalg.norm(pose[:, :3] - c["t"], axis=1) / np.linalg.norm(c["t"], axis=1)
    assert rel.max() <= PN.WORST_NOISE_FREE and 0 < info[:, 3].sum() < 257                                   # both starts are needed


def test_cone_model_ordering():
    m = PO.cone_model()
    assert m.shape == (7, 3) and m.dtype == np.float64 and (m[:, 2] == 0).all() and m[0, 0] == 0
    assert m[0, 1] == m[:, 1].min() and np.isclose(m[:, 1].max() - m[:, 1].min(), 0.325 * 0.9)   # the apex on top
    for left, right in ((1, 2), (3, 4), (5, 6)):
        assert m[left, 0] == -m[right, 0] < 0 and m[left, 1] == m[right, 1]                                  # level pairs, left then right
    assert (np.diff(m[[0, 1, 3, 5], 1]) > 0).all() and (np.diff(m[[1, 3, 5], 0]) < 0).all()                  # down the side, widening


def test_bad_arguments_and_a_default_detector_loads_nothing(monkeypatch):
    from mdcv.yolo import detect as DT
    from mdcv.yolo.models import Darknet
    monkeypatch.chdir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mini"))
    net = Darknet("mini.cfg", 2.0, 1.6, 25.0, 0.1, False, precision="fp32")
    kpt = type("Kpt", (), {"image_size": (80, 80), "num_kpt": 7})()
    monkeypatch.setattr(_lib, "_pnp", None)
    pts = torch.zeros(2, 7, 2)
    for make in (lambda **kw: DT.FrameConeDetector(net, kpt, **kw), lambda **kw: DT.TiledFrameConeDetector(net, kpt, 1.0, **kw),
                 lambda camera=None, cone_model=None, pnp_iters=30: PO.solve_cone_pnp(pts, camera, cone_model, max_iters=pnp_iters)):
        for match, kw in (("one per frame", dict(camera=np.ones((2, 3)))), ("positive", dict(camera=(0, 1, 0, 0))),
                          (r"\[7,3\]", dict(camera=(1, 1, 0, 0), cone_model=np.zeros((7, 2)))), ("iters", dict(camera=(1, 1, 0, 0), pnp_iters=0))):
            with pytest.raises(ValueError, match=match):
                make(**kw)
    with pytest.raises(ValueError, match="one per frame"):
        list(DT.FrameConeDetector(net, kpt, camera=np.ones((2, 4))).detect_frames([np.zeros((8, 8, 3), np.uint8)] * 3))
    assert DT.FrameConeDetector(net, kpt).camera is None and DT.FrameConeDetector(net, kpt, camera=(9, 9, 3, 2)).camera.shape == (1, 4)
    assert _lib._pnp is None and not any("mdcv_pnp" in line for line in open("/proc/self/maps"))     # building detectors loads nothing
