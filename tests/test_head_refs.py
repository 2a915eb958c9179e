"""Pin tests/helpers/head_refs.py (the float64 references of tests/test_gpu_heads.py) to the outputs the reference project itself
recorded in tests/golden/yolo_layer_*.npz and cross_ratio.npz.  CPU only.

The golden values are fp32 results; the float64 path must reproduce them to fp32 rounding, 32 u of the largest magnitude of the tensor
(u = 2^-24; head_refs.bound with e32 = 0), and its own fp32 evaluation must sit inside the same distance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_refs as hr  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy


def near(got, want, what):
    want = torch.as_tensor(np.asarray(want)).double()
    err, tol = hr.maxabs(got.double() - want), hr.bound(0.0, hr.maxabs(want))
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("name", ["yolo_layer_c1_g13.npz", "yolo_layer_c80_g13.npz", "yolo_layer_c1_g26.npz"])
@pytest.mark.parametrize("layer", [hr.yo.yolo_layer, hr.yolo_layer_bce], ids=["oracle", "bce"])
def test_yolo_refs_reproduce_the_golden_files(name, layer):
    z = np.load(os.path.join(G, name))
    anchors = [tuple(a) for a in z["anchors_px"].tolist()]
    C, cfg_h, s, tg = int(z["C"]), int(z["cfg_h"]), T(z["sample"]), T(z["targets"])
    for dtype in (torch.float64, torch.float32):
        loss, parts, ds = hr.yolo_train(s, anchors, C, cfg_h, tg, dtype, layer=layer)
        near(loss, z["loss"], "loss")
        for k in range(6):
            near(parts[k], z["parts"][k], f"part {k}")
        near(ds, z["dsample"], "dsample")
        assert np.array_equal(ds.numpy() != 0, z["dsample"] != 0)
        ev = hr.yolo_eval(s, anchors, C, cfg_h, dtype)
        for sl in (slice(0, 2), slice(2, 4), slice(4, None)):
            near(ev[..., sl], z["eval_out"][..., sl], "eval")
    B, _, Gh, Gw = s.shape
    pos, neg = hr.yolo_masks(tg, anchors, C, Gh, Gw, cfg_h / Gh)
    assert int(pos.sum()) > 0 and int(neg.sum()) > 0 and not bool((pos & neg).any())


def test_stable_sigmoid_is_torch_sigmoid_without_the_overflow():
    """same value (two fp32 roundings apart at most) and the same backward wherever exp(-x) is finite; the denormal true value below"""
    x = torch.linspace(-80, 80, 6401).requires_grad_(True)
    p, q = hr.stable_sigmoid(x), torch.sigmoid(x)
    assert float(((p - q).abs() / q).detach().max()) <= 4 * hr.U
    gp, = torch.autograd.grad(p.sum(), x)
    assert torch.equal(gp, (1 - p) * p)
    x64 = torch.tensor([-95.0, -30.0, 30.0, 95.0], dtype=torch.float64)
    assert torch.equal(hr.stable_sigmoid(x64.float()), torch.sigmoid(x64).float())
    assert 0 < float(hr.stable_sigmoid(torch.tensor(-95.0))) < 2.0 ** -126


def test_cross_ratio_ref_reproduces_the_golden_file():
    z = np.load(os.path.join(G, "cross_ratio.npz"))
    hm, thm, tpts, pts = T(z["hm"]), T(z["thm"]), T(z["tpts"]), T(z["pts"])
    for lt in hr.LOSS_TYPES:
        for geo in (False, True):
            tag = f"{lt}:{int(geo)}"
            for dtype in (torch.float64, torch.float32):
                out3, dp = hr.cross_ratio(hm, pts, thm, tpts, lt, geo, 0.05, 0.07, None, dtype)
                for k in range(3):
                    near(out3[k], z[f"loss::{tag}"][k], f"{tag} out3[{k}]")
                near(dp, z[f"dpts::{tag}"], f"{tag} dpts")
    # upstream gradients of the two parts: d(a loc + b geo) = a d(loc) + b d(geo)
    _, d_loc = hr.cross_ratio(hm, pts, thm, tpts, "l2_softargmax", False, 0.05, 0.07, None, torch.float64)
    _, d_all = hr.cross_ratio(hm, pts, thm, tpts, "l2_softargmax", True, 0.05, 0.07, None, torch.float64)
    _, d_sc = hr.cross_ratio(hm, pts, thm, tpts, "l2_softargmax", True, 0.05, 0.07, (0.5, 2.0), torch.float64)
    near(d_sc, (0.5 * d_loc + 2.0 * (d_all - d_loc)).numpy(), "gscale")


def test_softargmax_ref_is_the_oracles_head():
    """head_refs.softargmax is keypoint_forward's tail: the heat-map rows of cross_ratio.npz are softmax outputs, so softmax(log hm) = hm"""
    z = np.load(os.path.join(G, "cross_ratio.npz"))
    hm = T(z["hm"])[:2]
    got, pts = hr.softargmax(torch.log(hm.double()), torch.float64)
    near(got, hm.numpy(), "hm")
    vy, vx = torch.arange(80).double() / 80, torch.arange(80).double() / 80
    want = torch.stack([(hm.double().sum(2) * vx).sum(-1), (hm.double().sum(3) * vy).sum(-1)], -1)
    near(pts, want.numpy(), "pts")
    d = hr.softargmax_bwd(torch.log(hm.double()), torch.ones(2, 7, 2), None, torch.float64)
    assert hr.maxabs(d.sum((2, 3))) < 1e-12                  # a softmax Jacobian maps onto zero-sum rows
