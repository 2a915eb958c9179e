"""Cone positions from key points: the batched planar PnP of csrc/cone_pnp.hip (include/mdcv_pnp.h).

RektNet's seven key points exist for "depth estimation of traffic cones on the 3D map" (the reference's README); the reference itself
stops at the points, and a caller would loop `cv2.solvePnP` over them on the host.  `solve_cone_pnp` takes the points where the
detectors leave them -- on the device -- and returns every cone's position and orientation in the camera frame from one launch, without
a host read.  Pinhole camera without distortion: undistort the key points first if the lens needs it (out of scope here, as are
covariances, tracking and the map frame).
"""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib

NUM_KPT = 7
STATUS_BAD_POINTS, STATUS_BAD_WINDOW, STATUS_BAD_CAMERA, STATUS_ZERO_EXTENT, STATUS_SINGULAR, STATUS_ITER_CAP = 1, 2, 4, 8, 16, 32   # MDCV_PNP_*
STATUS_DEGENERATE = 31                   # any of these: the pose is NaN

ConePoses = namedtuple("ConePoses", "t R rms start iters status")
ConePoses.__doc__ = """Device tensors, one row per cone: t float64 [M,3] (metres, camera frame: x right, y down, z forward), R float64 [M,3,3]
(model to camera), rms float64 [M] (reprojection error in pixels), start int32 [M] (0: the frontal start won, 1: its mirror image), iters
int32 [M,2] (accepted steps of either start), status int32 [M] (STATUS_* bits; with any of STATUS_DEGENERATE t, R and rms are NaN): views
of the two tables of include/mdcv_pnp.h."""


def cone_model(height=0.325, base_width=0.228, top_width=0.046, levels=(0.34, 0.62, 0.90)):
    """The [7,3] float64 model table in metres, in the key-point order of cross_ratio_loss.py: point 0 the apex, 1 / 3 / 5 down the left
    side, 2 / 4 / 6 down the right side, (1,2), (3,4) and (5,6) level.  Planar (z = 0), y down, centred on the cone's axis and on half its
    height.  `levels`: the three pairs' depth below the apex as fractions of the height.  The defaults are nominal Formula Student
    small-cone dimensions; they have NOT been checked against the labels of the RektNet data set -- pass your own table if yours differ."""
    h, half_b, half_t = float(height), float(base_width) / 2.0, float(top_width) / 2.0
    lv = [float(f) for f in levels]
    if not (h > 0 and half_b > 0 and half_t >= 0 and len(lv) == 3 and all(0 < f <= 1 for f in lv) and lv == sorted(lv)):
        raise ValueError(f"cone_model: need height, base_width > 0, top_width >= 0 and three ascending levels in (0, 1], got "
                         f"{height!r}, {base_width!r}, {top_width!r}, {levels!r}")
    m = np.zeros((NUM_KPT, 3))
    m[0] = 0.0, -h / 2.0, 0.0
    for i, f in enumerate(lv):
        x = half_t + (half_b - half_t) * f
        m[1 + 2 * i] = -x, -h / 2.0 + h * f, 0.0
        m[2 + 2 * i] = x, -h / 2.0 + h * f, 0.0
    return m


def check_model(model):
    """None -> the default; anything else must be a finite [7,3] table"""
    m = cone_model() if model is None else np.asarray(model, np.float64)
    if m.shape != (NUM_KPT, 3) or not np.isfinite(m).all():
        raise ValueError(f"cone model must be a finite [{NUM_KPT},3] table in metres (see cone_model()), got shape {m.shape}")
    return np.ascontiguousarray(m)


def check_camera(camera, frames=None):
    """one (fx, fy, cx, cy), or one per frame -> float64 [n,4]; with `frames`, n must be 1 or `frames`"""
    c = np.asarray(camera, np.float64)
    if c.shape == (4,):
        c = c[None]
    if c.ndim != 2 or c.shape[1] != 4 or len(c) < 1 or (frames is not None and len(c) not in (1, int(frames))):
        raise ValueError(f"camera must be one (fx, fy, cx, cy) or one per frame" + (f" of the call ({frames})" if frames is not None else "")
                         + f", got shape {c.shape}")
    if not (np.isfinite(c).all() and (c[:, :2] > 0).all()):
        raise ValueError("camera: fx and fy must be positive and every word finite; pass focal lengths in pixels")
    return np.ascontiguousarray(c)


def _exp_so3(w):
    th = np.sqrt(w @ w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    a, b = (1.0 - th * th / 6.0, 0.5 - th * th / 24.0) if th < 1e-8 else (np.sin(th) / th, (1.0 - np.cos(th)) / (th * th))
    return np.eye(3) + a * K + b * (K @ K)


def synthetic_cones(M, cameras, seed=0, noise=0.0, windows=False, model=None, z_range=(2.5, 10.0), tilt=15.0):
    """M seeded poses of `model` seen by cameras [n,4] (a random one per cone), for tests and timing: tilts of +-`tilt` degrees about x and
    y, +-5 about z, depth in `z_range` metres, up to 0.3 z / 0.15 z off axis, Gaussian pixel noise -> dict: pts float32 [M,7,2], window
    int32 [M,4] or None, owner int32 [M,2], cam, model, R [M,3,3], t [M,3].  With `windows` the points are normalised in an integer window
    around the cone, as a detector's crop has them."""
    rng, model, cameras = np.random.default_rng([seed, int(windows), int(noise > 0)]), check_model(model), check_camera(cameras)
    owner = np.stack([rng.integers(0, len(cameras), M), np.arange(M)], 1).astype(np.int32)
    R, t, pts, win = np.zeros((M, 3, 3)), np.zeros((M, 3)), np.zeros((M, NUM_KPT, 2), np.float32), np.zeros((M, 4), np.int32)
    for m in range(M):
        w = np.radians(np.array([rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt), rng.uniform(-5, 5)]))
        R[m] = _exp_so3(np.array([0.0, 0.0, w[2]])) @ _exp_so3(np.array([0.0, w[1], 0.0])) @ _exp_so3(np.array([w[0], 0.0, 0.0]))
        z = rng.uniform(*z_range)
        t[m] = z * rng.uniform(-0.3, 0.3), z * rng.uniform(-0.15, 0.15), z
        P, cam = model @ R[m].T + t[m], cameras[owner[m, 0]]
        uv = np.stack([cam[0] * P[:, 0] / P[:, 2] + cam[2], cam[1] * P[:, 1] / P[:, 2] + cam[3]], 1) + noise * rng.standard_normal((NUM_KPT, 2))
        if windows:
            lo, hi = np.floor(uv.min(0)) - 2, np.ceil(uv.max(0)) + 2
            win[m] = lo[0], lo[1], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
            uv = (uv - win[m, :2]) / win[m, 2:]
        pts[m] = uv
    return dict(pts=pts, window=win if windows else None, owner=owner, cam=cameras, model=model, R=R, t=t)


def parse_camera(text):
    """the command line's "fx,fy,cx,cy" -> float64 [1,4]"""
    try:
        return check_camera([float(v) for v in str(text).split(",")])
    except ValueError as e:
        raise ValueError(f"--camera takes fx,fy,cx,cy in pixels, got {text!r}: {e}") from None


def _device_table(a, check, dev):
    """a float64 device tensor passes as it is (a caller's cached upload; the kernel flags bad rows); anything else is checked and uploaded"""
    if torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float64 and a.dim() == 2:
        return a.contiguous()
    return torch.from_numpy(check(a)).to(dev)


def solve_cone_pnp(points, camera, model=None, windows=None, owner=None, max_iters=30):
    """points: float32 device tensor [M,7,2] -- pixels, or with `windows` (int32 [M,4]: x0, y0, w, h) normalised in the window as
    KeypointNet returns them; camera: one (fx, fy, cx, cy) or [n,4] (or a float64 device tensor [n,4], used as it is), indexed by owner[:, 0] (int32 [M,2]: frame, slot -- the detectors'
    owner table); model: [7,3] metres (default `cone_model()`) -> `ConePoses`.  One launch on the current stream, no host read."""
    if points.dim() != 3 or tuple(points.shape[1:]) != (NUM_KPT, 2) or points.dtype != torch.float32:
        raise ValueError(f"solve_cone_pnp: points must be float32 [M,{NUM_KPT},2], got {tuple(points.shape)} {points.dtype}")
    if int(max_iters) < 1:
        raise ValueError(f"solve_cone_pnp: max_iters must be at least 1, got {max_iters!r}")
    M, dev = int(points.shape[0]), points.device
    cam, mod = _device_table(camera, check_camera, dev), _device_table(model, check_model, dev)
    if tuple(cam.shape[1:]) != (4,) or tuple(mod.shape) != (NUM_KPT, 3):
        raise ValueError(f"solve_cone_pnp: device tables must be camera [n,4] and model [{NUM_KPT},3], got {tuple(cam.shape)}, {tuple(mod.shape)}")
    if len(cam) > 1 and owner is None:
        raise ValueError(f"solve_cone_pnp: {len(cam)} cameras need an owner table [M,2] whose first column is the camera row")
    for name, tab, width in (("windows", windows, 4), ("owner", owner, 2)):
        if tab is not None and (tab.dtype != torch.int32 or tuple(tab.shape) != (M, width) or tab.device != dev):
            raise ValueError(f"solve_cone_pnp: {name} must be an int32 [M,{width}] tensor on the points' device")
    _lib.require_gpu(points)
    pts = points.detach().contiguous()
    win = None if windows is None else windows.contiguous()
    own = None if owner is None else owner.contiguous()
    pose = torch.empty(M, 16, dtype=torch.float64, device=dev)
    info = torch.empty(M, 4, dtype=torch.int32, device=dev)
    L = _lib.pnp_lib()
    with torch.cuda.device(dev):
        L.check(L.cone_pnp(pts.data_ptr(), None if win is None else win.data_ptr(), None if own is None else own.data_ptr(), cam.data_ptr(),
                           len(cam), mod.data_ptr(), M, int(max_iters), pose.data_ptr(), info.data_ptr(),
                           torch.cuda.current_stream(dev).cuda_stream), "cone_pnp")
    return ConePoses(pose[:, 0:3], pose[:, 3:12].view(M, 3, 3), pose[:, 12], info[:, 3], info[:, 1:3], info[:, 0])
