"""Pin tests/helpers/kpt_eval_refs.py (the float64 references of tests/test_gpu_kpt_eval.py) to what the reference project itself computed
for tests/golden/kpt_eval.npz (tests/golden/make_golden_kpt_eval.py): CrossRatioLoss on every sample alone, and utils.calculate_distance.
CPU only.

The recorded values are fp32 results.  The float64 helper must reproduce them within head_refs.bound(e32, scale), with e32 the helper's own
float32 error on the column and scale the column's largest float64 magnitude; nothing is a constant.  Measured, float64 helper against
the recorded fp32 values: <= 3.0e-7 on the heat-map sums (of about 4), <= 3.9e-7 on the point losses, <= 2.5e-5 on the distances (of up
to 240 pixels, where the reference rounds the scaled points before it subtracts them)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_refs as hr  # noqa: E402
import kpt_eval_refs as kr  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
F64, F32 = torch.float64, torch.float32


def near_columns(got64, got32, want, what):
    want = torch.as_tensor(np.asarray(want)).double()
    for k in range(want.shape[1]):
        e32 = hr.maxabs(got32[:, k] - got64[:, k])
        tol = hr.bound(e32, hr.maxabs(got64[:, k]))
        for got in (got64, got32):
            err = hr.maxabs(got[:, k] - want[:, k])
            assert err <= tol, f"{what} column {k}: {err:.3e} > {tol:.3e}"


def test_per_sample_losses_reproduce_the_reference_at_batch_one():
    z = np.load(os.path.join(G, "kpt_eval.npz"))
    hm, thm, pts, tpts = T(z["hm"]), T(z["thm"]), T(z["pts"]), T(z["tpts"])
    gh, gv = (float(v) for v in z["gamma"])
    assert torch.equal(pts[2, 3], pts[2, 1])                       # the coincident pair is in the fixture
    for lt in hr.LOSS_TYPES:
        for geo in (False, True):
            tag = f"{lt}:{int(geo)}"
            r64 = kr.per_sample(hm, pts, thm, tpts, lt, geo, gh, gv, F64)
            r32 = kr.per_sample(hm, pts, thm, tpts, lt, geo, gh, gv, F32)
            near_columns(r64, r32, z[f"per::{tag}"], tag)
            if not geo:
                assert bool((r64[:, 1] == 0).all()) and torch.equal(r64[:, 0], r64[:, 2])


def test_distances_reproduce_calculate_distance():
    z = np.load(os.path.join(G, "kpt_eval.npz"))
    pts, tpts = T(z["pts"]), T(z["tpts"])
    sx, sy = (float(int(z["C"]) * s) for s in z["input_size"])
    assert (sx, sy) == kr.DIST_SCALE
    near_columns(kr.distances(pts, tpts, sx, sy, F64), kr.distances(pts, tpts, sx, sy, F32), z["dist"], "dist")
    rows = kr.rows(T(z["hm"]), pts, T(z["thm"]), tpts, "l1_softargmax", True, 0.05, 0.07, sx, sy, F64)
    assert rows.shape == (6, kr.ROW) and bool((rows[:, 10:] == 0).all())
    assert torch.equal(rows[:, 3:10], kr.distances(pts, tpts, sx, sy, F64))


def test_the_mean_of_batch_one_geo_losses_is_not_the_batched_geo_loss():
    """why mdcv_cross_ratio_loss on a validation batch cannot stand in for eval_model: the batched geometric term is the mean of a [B,B]
    all-pairs matrix.  The location term agrees to fp32 rounding; geo and total do not."""
    z = np.load(os.path.join(G, "kpt_eval.npz"))
    for lt in hr.LOSS_TYPES:
        ev, batched, per = z[f"eval::{lt}:1"], z[f"batched::{lt}:1"].astype(np.float64), z[f"per::{lt}:1"].astype(np.float64)
        assert abs(ev[0] - batched[0]) <= hr.bound(0.0, abs(ev[0]))
        assert abs(per[:, 1].mean() - ev[1]) <= hr.bound(0.0, abs(ev[1]))
        assert abs(ev[1] - batched[1]) > 0.05 * abs(ev[1])
        assert abs(ev[2] - batched[2]) > 0.05 * abs(ev[1])
    # the oracle's batched call says the same as the reference's
    hm, thm, pts, tpts = T(z["hm"]), T(z["thm"]), T(z["pts"]), T(z["tpts"])
    o64, _ = hr.cross_ratio(hm, pts, thm, tpts, "l1_softargmax", True, 0.05, 0.07, None, F64, want_grad=False)
    b = z["batched::l1_softargmax:1"]
    for k in range(3):
        assert abs(float(o64[k]) - float(b[k])) <= hr.bound(0.0, abs(float(b[k])))
