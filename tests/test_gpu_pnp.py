"""mdcv_cone_pnp (csrc/cone_pnp.hip) against the float64 restatement (tests/helpers/pnp_numpy.py) at the group (8 lanes a
cone), wave (8 cones) and workgroup (32 cones) boundaries, per-frame cameras, with and without windows, and at the default cap; the
degenerate kinds beside good cones; FrameConeDetector(camera=) end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pnp_numpy as PN  # noqa: E402
from test_gpu_kpt_detect import kpnet, mini, scene  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("M,windows,cap", [(M, w, PN.MAX_ITERS) for M in PN.SIZES for w in (False, True)] + [(257, True, 30)])
def test_against_truth_and_restatement(M, windows, cap):
    from mdcv.rektnet import solve_cone_pnp
    for noise in (0.0, 0.5):
        c, want, winfo = PN.reference(noise, windows, cap)
        want, winfo, win = want[:M], winfo[:M], c["window"]
        got = solve_cone_pnp(dev(c["pts"][:M]), c["cam"], c["model"], dev(win if win is None else win[:M]), dev(c["owner"][:M]), cap)
        t, start, status = (f.cpu().numpy() for f in (got.t, got.start, got.status))
        if noise == 0.0:                                                        # against the truth, where the restatement is not at the cap
            ok = winfo[:, 0] == 0
            rel = np.linalg.norm(t - c["t"][:M], axis=1) / np.linalg.norm(c["t"][:M], axis=1)
            print("noise-free: worst relative translation error", rel[ok].max(), "of the bound", rel[ok].max() / PN.NOISE_FREE_BOUND)
            assert rel[ok].max() <= PN.NOISE_FREE_BOUND and np.array_equal(start, winfo[:, 3]) and np.array_equal(status, winfo[:, 0])
            continue
        tie = np.abs(want[:, 13] - want[:, 14]) <= 1e-6 * np.maximum(want[:, 13], want[:, 14])
        assert np.nonzero(tie)[0].tolist() == [m for m in PN.NEAR_TIES[windows, cap] if m < M]            # the exact set, as recorded
        bound = np.array([max(4 * PN.CAP_CHANGE.get((windows, cap, m), 0.0), 1e-12) for m in range(M)])
        held = (winfo[:, 1:3] < cap).all(1) | np.array([(windows, cap, m) in PN.CAP_CHANGE for m in range(M)])   # below the cap, or recorded
        err = np.abs(t - want[:, :3]).max(1)
        print("noisy: largest fraction of the bound", (err / bound)[held].max(), "cones compared", int(held.sum()), "of", M)
        assert (err <= bound)[held].all() and np.array_equal(start[~tie], winfo[~tie, 3]) and np.array_equal(status[~tie], winfo[~tie, 0])


def test_degenerate_cones_beside_good_ones():
    from mdcv.rektnet import solve_cone_pnp
    c = {k: (v if k in ("cam", "model") else v[:17]) for k, v in PN.reference(0.5, True)[0].items()}
    pts, win, own, cam = c["pts"].copy(), c["window"].copy(), c["owner"].copy(), np.vstack([c["cam"], [[-1.0, 900.0, 0, 0]], [[900.0, 0.0, 0, 0]]])
    pts[1, 3, 0], pts[3, 6, 1], win[5, 2], win[7, 3] = np.nan, np.inf, 0, -5
    own[9, 0], own[11, 0], own[12, 0] = 3, 4, 5                                 # cameras with fx < 0, fy == 0, a row outside the table
    pts[14, :, 1] = pts[14, 0, 1]                                               # no v extent
    kinds = {1: PN.BAD_POINTS, 3: PN.BAD_POINTS, 5: PN.BAD_WINDOW, 7: PN.BAD_WINDOW, 9: PN.BAD_CAMERA, 11: PN.BAD_CAMERA, 12: PN.BAD_CAMERA,
             14: PN.ZERO_EXTENT}
    bad, good = list(kinds), [m for m in range(17) if m not in kinds]           # good: four in the first wave, three in the second, one in the third

    def run(pts, win, own, cam, model):                     # device tables pass unchecked, so cameras the Python front refuses reach the kernel
        return [f.cpu().numpy() for f in solve_cone_pnp(dev(pts), dev(cam), dev(model), dev(win), dev(own), PN.MAX_ITERS)]
    base, got = run(c["pts"], c["window"], c["owner"], c["cam"], c["model"]), run(pts, win, own, cam, c["model"])
    assert got[5].tolist() == [kinds.get(m, 0) for m in range(17)] and all(np.isnan(f[bad]).all() for f in got[:3]) and not got[4][bad].any()
    assert all(np.array_equal(g[good], b[good]) for g, b in zip(got, base))     # every field of the good cones, bit for bit
    line = run(c["pts"], c["window"], c["owner"], c["cam"], c["model"] * [0.0, 1.0, 0.0])     # a model on one line: J's yaw column is zero;
    assert (line[5] == PN.SINGULAR).all() and np.isnan(line[0]).all()           # the model is the call's, so this kind has a call of its own


def test_frame_cone_detector_with_a_camera(mini, kpnet, scene, monkeypatch):    # noqa: F811
    from mdcv import _lib
    from mdcv.rektnet import solve_cone_pnp
    from mdcv.yolo.detect import FrameConeDetector
    frames, thres = scene
    monkeypatch.setattr(_lib, "_pnp", None)
    plain = list(FrameConeDetector(mini, kpnet, conf_thres=thres, batch_size=2, bucket=8, max_cones=2).detect_frames(frames))
    assert _lib._pnp is None and all(r.position is r.rotation is r.reproj_rms is r.pose_ok is None for r in plain)
    cams = PN.CAMS * [[0.1, 0.1, 0.05, 0.05]]                                   # one per frame, scaled to the small frames
    got = list(FrameConeDetector(mini, kpnet, conf_thres=thres, batch_size=2, bucket=8, max_cones=2, camera=cams, pnp_iters=40).detect_frames(frames))
    assert _lib._pnp is not None and sum(int(r.has_crop.sum()) for r in got) >= 3 and any((~r.has_crop).any() for r in got)
    for f, (r, p) in enumerate(zip(got, plain)):
        has = r.has_crop
        assert np.array_equal(r.keypoints, p.keypoints, equal_nan=True) and np.array_equal(r.annotated, p.annotated) and not r.pose_ok[~has].any()
        assert all(np.isnan(a[~has]).all() for a in (r.position, r.rotation, r.reproj_rms)) and r.rotation.shape == (len(r.boxes), 3, 3)
        if has.any():
            want = solve_cone_pnp(dev(r.keypoints[has]), cams[f], windows=dev(r.windows[has]), max_iters=40)
            for mine, theirs in ((r.position, want.t), (r.rotation, want.R), (r.reproj_rms, want.rms), (r.pose_ok, (want.status & 31) == 0)):
                assert np.array_equal(mine[has], theirs.cpu().numpy(), equal_nan=True)
