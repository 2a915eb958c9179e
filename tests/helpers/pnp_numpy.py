"""float64 NumPy restatement of mdcv_cone_pnp (include/mdcv_pnp.h, csrc/cone_pnp.hip): the definition the kernel follows.
One cone at a time, plain loops.  Also the synthetic cases of the tests with the restatement's result on them (`reference`) and their bounds."""
import functools

import numpy as np

from mdcv.rektnet.pose import synthetic_cones

BAD_POINTS, BAD_WINDOW, BAD_CAMERA, ZERO_EXTENT, SINGULAR, ITER_CAP = 1, 2, 4, 8, 16, 32     # MDCV_PNP_* status bits
LAMBDA0, LAMBDA_MIN, MAX_TRIALS = 1e-3, 1e-12, 12
COST_NOISE = 2.0 ** -36            # a step whose cost rises by less than COST_NOISE * sqrt(cost) has not risen: rounding of the residuals
STEP_TOL = 1e-10                   # stop when an accepted step moves the 14 projections by less than this many pixels (|J d|)
TIE = 2.0 ** -10                   # start B wins only when its cost is below (1 - TIE) * start A's

# measured on the CPU with this restatement on `reference`'s cases:
WORST_NOISE_FREE = 1.25e-6         # worst relative translation error, noise-free, at MAX_ITERS (1.2472e-06: the float32 pixels)
NOISE_FREE_BOUND = 4 * WORST_NOISE_FREE
# noisy: change of t (m) when the cap is doubled, {(windows, max_iters, case)}; exactly 0 for a cone whose starts both end below the cap
CAP_CHANGE = {(True, 100, 233): 9.21e-8}
# noisy cases whose two starts end within 1e-6 relative of each other (both reach ONE minimum), by (windows, max_iters)
NEAR_TIES = {(False, 100): (32, 57, 58, 82, 92, 98, 106, 113, 127, 143, 149, 167, 171, 178, 199, 204, 211, 212, 237),
             (True, 100): (6, 14, 23, 65, 114, 122, 127, 128, 145, 205, 229, 233, 241),
             (True, 30): (6, 23, 65, 114, 122, 127, 128, 205, 229, 233, 241)}


def rodrigues(w):
    """exp([w]x)"""
    th = np.sqrt(w @ w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def _normal(uv, cam, model, R, t):
    """-> in front, J^T J [6,6], J^T r [6], cost; unknowns (w, t), R <- exp([dw]x) R so d(RP + t)/dw = -[RP]x"""
    fx, fy, cx, cy = cam
    Q = model @ R.T
    X, Y, Z = (Q + t).T
    if not (Z > 0).all():
        return False, None, None, np.inf
    iz = 1.0 / Z
    x, y = X * iz, Y * iz
    r = np.concatenate([fx * x + cx - uv[:, 0], fy * y + cy - uv[:, 1]])
    a, b = fx * iz, fy * iz
    zero = np.zeros(7)
    # du = a (dX - x dZ), dv = b (dY - y dZ); dX = Qz wy - Qy wz + tx, dY = Qx wz - Qz wx + ty, dZ = Qy wx - Qx wy + tz
    Ju = np.stack([-a * x * Q[:, 1], a * (Q[:, 2] + x * Q[:, 0]), -a * Q[:, 1], a, zero, -a * x], 1)
    Jv = np.stack([-b * (Q[:, 2] + y * Q[:, 1]), b * y * Q[:, 0], b * Q[:, 0], zero, b, -b * y], 1)
    J = np.concatenate([Ju, Jv])
    return True, J.T @ J, J.T @ r, float(r @ r)


def _cholesky_solve(A, g, lam):
    """(A + lam diag A) d = -g by Cholesky; None when a pivot is not positive and finite"""
    try:
        L = np.linalg.cholesky(A + lam * np.diag(np.diag(A)))
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, -g)) if np.isfinite(L).all() else None


def refine(uv, cam, model, R, t, max_iters):
    """Levenberg-Marquardt from (R, t) -> R, t, cost, accepted steps, status bits (0, SINGULAR or ITER_CAP)"""
    ok, A, g, cost = _normal(uv, cam, model, R, t)
    if not ok:
        return R, t, np.inf, 0, SINGULAR                      # a start behind the camera
    lam, iters, trials = LAMBDA0, 0, 0
    while True:
        d = _cholesky_solve(A, g, lam)
        if d is None:
            return R, t, cost, iters, SINGULAR
        R2, t2 = rodrigues(d[:3]) @ R, t + d[3:]
        ok, A2, g2, cost2 = _normal(uv, cam, model, R2, t2)
        if ok and cost2 <= cost + COST_NOISE * np.sqrt(cost):
            moved = d @ A @ d                                  # |J d|^2
            R, t, A, g, cost = R2, t2, A2, g2, cost2
            lam, iters, trials = max(lam * 0.1, LAMBDA_MIN), iters + 1, 0
            if moved <= STEP_TOL * STEP_TOL:
                return R, t, cost, iters, 0
            if iters >= max_iters:
                return R, t, cost, iters, ITER_CAP
        else:
            lam, trials = lam * 10.0, trials + 1
            if trials >= MAX_TRIALS:
                return R, t, cost, iters, 0                    # no step of any length lowers the cost: a minimum, to rounding


def mirror(R, t, model):
    """start B: the plane normal n = R e_z mirrored about the line of sight s to the model centroid, by the minimal rotation"""
    n = R[:, 2]
    c = R @ model.mean(0) + t
    s = c / np.sqrt(c @ c)
    n2 = 2.0 * (n @ s) * s - n
    a, co = np.cross(n, n2), n @ n2
    if not 1.0 + co > 1e-12:
        return R                                               # the plane is seen edge-on: the mirror image is the pose itself
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return (np.eye(3) + K + (K @ K) / (1.0 + co)) @ R


def solve_one(pts, window, cam, model, max_iters=30):
    """-> pose [16] (t, R row-major, rms, cost A, cost B, 0), info [4] (status, iterations A, iterations B, start)"""
    pose, info = np.full(16, np.nan), np.zeros(4, np.int32)
    pts = np.asarray(pts, np.float32).astype(np.float64)
    status = BAD_POINTS * (not np.isfinite(pts).all()) | BAD_WINDOW * (window is not None and bool(window[2] <= 0 or window[3] <= 0))
    status |= BAD_CAMERA * (not (cam[0] > 0 and cam[1] > 0 and np.isfinite(cam).all()))
    if status == 0:
        uv = pts if window is None else np.stack([window[0] + pts[:, 0] * window[2], window[1] + pts[:, 1] * window[3]], 1)
        ext_v, ext_y = uv[:, 1].max() - uv[:, 1].min(), model[:, 1].max() - model[:, 1].min()
        if not (ext_v > 0 and ext_y > 0):
            status |= ZERO_EXTENT
    if status == 0:
        tz = cam[1] * ext_y / ext_v
        mc, ub, vb = model.mean(0), uv[:, 0].mean(), uv[:, 1].mean()
        tA = np.array([tz * (ub - cam[2]) / cam[0] - mc[0], tz * (vb - cam[3]) / cam[1] - mc[1], tz - mc[2]])
        RA, tA, cA, itA, sA = refine(uv, cam, model, np.eye(3), tA, max_iters)
        status |= sA & SINGULAR
    if status == 0:
        RB, tB, cB, itB, sB = refine(uv, cam, model, mirror(RA, tA, model), tA, max_iters)
        b = bool(not (sB & SINGULAR) and cB < (1.0 - TIE) * cA)
        R, t, c = (RB, tB, cB) if b else (RA, tA, cA)
        status |= (sB if b else sA) & ITER_CAP
        pose[:3], pose[3:12], pose[12], pose[13], pose[14], pose[15] = t, R.reshape(-1), np.sqrt(c / 7.0), cA, cB, 0.0
        info[1:] = itA, itB, int(b)
    info[0] = status
    return pose, info


CAMS = np.array([[1200.0, 1200.0, 640.0, 360.0], [1150.0, 1210.0, 600.0, 380.0], [900.0, 880.0, 512.0, 300.0]])
SEED, MAX_ITERS = 117, 100          # the first seed from 100 on whose 2 x 257 noise-free cases the restatement all recovers at this cap
SIZES = (1, 7, 8, 9, 65, 257)       # group, wave and workgroup boundaries of the kernel: the tests take the first M cases


@functools.lru_cache(None)
def reference(noise, windows, max_iters=MAX_ITERS, N=257):
    """the N fixed-seed cases (mdcv.rektnet.pose.synthetic_cones) and the restatement on them, computed once -> cases, pose [N,16], info [N,4]"""
    c = synthetic_cones(N, CAMS, SEED, noise, windows)
    out = [solve_one(c["pts"][m], c["window"][m] if windows else None, CAMS[c["owner"][m, 0]], c["model"], max_iters) for m in range(N)]
    return c, np.array([o[0] for o in out]), np.array([o[1] for o in out])
