"""No GPU: the exact-equality convolution tests (tests/test_gpu_conv_exact.py) stand on three things that are proved here on the CPU --
  1. at EVERY shape of every case table the float64 reference alone satisfies the conditions under which `==` is the right comparison
     (bf16 outputs representable, fp32 sums and per-row statistics below 2^24 quanta: helpers/conv_exact.py check_exact_preconditions);
  2. the torch float64 reference agrees with an independent direct-loop int64 numpy implementation (forward, data gradient, weight gradient);
  3. the comparison would notice the mistakes the suite is there for: four mutations of the reference each change at least one element of every
     output channel they touch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_exact as X  # noqa: E402

torch.set_num_threads(16)


def s2(t):
    B, Ci, H, W, Co = t
    return (B, Ci, H, W, Co, 3, 2, 1, 1, False)


def s2d(t):
    B, Cdy, Hd, Wd, Cdx = t
    return (B, Cdx, 2 * Hd, 2 * Wd, Cdy, 3, 2, 1, 1, False)


def stream10(t):
    B, Ci, Co, H, W, dil = t
    return (B, Ci, H, W, Co, 3, 1, dil, dil, False)


def ws2(t):
    B, Ci, Co, Ho, Wo, _ = t
    return (B, Ci, 2 * Ho, 2 * Wo, Co, 3, 2, 1, 1, False)


def fuse10(t):
    B, Ci, H, W, Co, k, s, p = t
    return (B, Ci, H, W, Co, k, s, p, 2 if (k == 3 and p == 2) else 1, False)


# every 10-tuple the GPU file runs forward / data gradient / weight gradient on, with what it runs
PLAIN = ([(c, "fdw") for c in X.CONV_CASES + X.VARIANT_CASES + X.NARROW_CASES] +
         [(X.c3(c, bias=c == X.SHIFT_CASES[0]), "fd") for c in X.SHIFT_CASES] + [(X.c3(c), "fd") for c in X.SHIFT_2D + [X.SHIFT_W70]] +
         [(X.c3(c, dil=2), "fd") for c in X.SHIFT_DIL2] + [(X.c3(X.SHIFT_CASES[3]), "f"), (X.c3(X.SHIFT_2D[0]), "f")] +
         [(c, "w") for c in [(3, 64, 26, 20, 64, 3, 1, 1, 1, False)] + [X.c3(c) for c in X.WGRAD_SHIFT_CASES + X.WGRAD_KWSHARED_CASES]] +
         [(pc["geom"], pc["run"].replace("b", "")) for pc in X.PROD_CASES if pc["run"] != "b"] +
         [(stream10(c), "w") for c in X.WGRAD_STREAM_CASES + X.WGRAD_DIRECT_CASES + X.WGRAD_STREAM_PROD] + [(ws2(c), "w") for c in X.WGRAD_S2_CASES] +
         [((B, 3, H, W, 16, 7, 1, 3, 1, False), "w") for B, H, W in X.STEM_CASES] + [(X.c3(c), "d") for c in X.SHIFT_WIDE_DGRAD])
FUSED = ([(s2(c), (1,)) for c in X.S2_CASES] + [(s2d(c), (1,)) for c in X.S2D_CASES] + [(X.FUSE1X1_CASE, (1,))] + [(fuse10(c), (0, 1, 2)) for c in X.FUSE_CASES] +
         [(pc["geom"], (1,)) for pc in X.PROD_CASES if "b" in pc["run"]])
# the dense grids (helpers/conv_exact.py DENSE_CASES, under their own cap): forward of the two forward cases, data gradient plain / + addsrc / fused of the third
DENSE = [(X.DENSE_FWD, "f"), (X.DENSE_FWD256, "f"), (X.DENSE_DGRAD, "d")]


@pytest.mark.parametrize("case,what", PLAIN, ids=str)
def test_preconditions_plain(case, what):
    B, Ci, H, W, Co, k, s, p, d, bias = case
    c = X.gen_case(X.seed_of(case), B, Ci, H, W, Co, k, s, p, d, bias)
    X.check_exact_preconditions(X.conv_conditions(c, fwd="f" in what, dgrad="d" in what, wgrad="w" in what))


@pytest.mark.parametrize("case,what", DENSE, ids=str)
def test_preconditions_dense(case, what):
    assert X.MACS_CAP < X.macs(X.c3(case)) <= X.DENSE_MACS_CAP and [c for c, _ in DENSE] == X.DENSE_CASES
    c = X.dense_refs(case)
    X.check_exact_preconditions(X.conv_conditions(c, fwd="f" in what, dgrad="d" in what, wgrad=False))
    if what == "d":
        X.check_exact_preconditions(X.fused_dgrad_conditions(c, codes=(1,), adds=(True,)))
        X.check_exact_preconditions({"dx": ("bf16", c["_dx"])})


@pytest.mark.parametrize("case,codes", FUSED, ids=str)
def test_preconditions_fused_dgrad(case, codes):
    c = X.conv_case(case)
    X.check_exact_preconditions(X.fused_dgrad_conditions(c, codes))


@pytest.mark.parametrize("case", X.BNAPPLY_CASES, ids=str)
def test_preconditions_wgrad_bnapply(case):
    X.check_exact_preconditions(X.bnapply_conditions(case))


@pytest.mark.parametrize("table,case", [(t, c) for t in ("PW_CASES", "PW_PROD_CASES", "PWB_CASES", "PWB_PROD_CASES", "FIRST_CASES", "AFFINE_CASES") for c in getattr(X, t)] +
                         [("AFFINE_PROD_CASES", c) for c, _ in X.AFFINE_PROD_CASES], ids=str)
def test_preconditions_block_forms(table, case):
    refs = {"PW_CASES": X.pw_refs, "PW_PROD_CASES": X.pw_refs, "PWB_CASES": X.pwb_refs, "PWB_PROD_CASES": X.pwb_refs, "AFFINE_PROD_CASES": X.affine_refs, "FIRST_CASES": X.first_refs, "AFFINE_CASES": X.affine_refs}[table]
    X.check_exact_preconditions(refs(case)["cond"])


def test_reference_cap_and_generator_rules():
    for case, _ in PLAIN:
        if case in [pc["geom"] for pc in X.PROD_CASES if pc.get("dense")]:
            continue
        listed = case in [stream10(X.WGRAD_DIRECT_CASES[1]), X.c3(X.SHIFT_WIDE_DGRAD[0])]        # the two 512 -> 1024 layers at 13 x 13 (3.2e9)
        assert X.macs(case) <= X.MACS_CAP or listed, case
    for pc in X.PROD_CASES:                                  # the dense 128-wide grids sit under their own, named cap; everything else under MACS_CAP
        assert X.prod_macs_ok(pc) and (not pc.get("dense") or X.macs(pc["geom"]) > X.MACS_CAP), pc["id"]
    c = X.conv_case(X.CONV_CASES[9])
    assert set(c["x"].unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0} and set(c["w"].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert float(c["addsrc"].abs().max()) == 4.0
    bn = c["bn_in"]
    pre = bn["scale"].view(1, -1, 1, 1) * bn["y"] + bn["shift"].view(1, -1, 1, 1)
    assert bool((pre != 0).all()) and bool((bn["scale"] < 0).any()) and set(bn["scale"].abs().unique().tolist()) == {0.5, 1.0, 2.0}
    assert set(bn["cA"].unique().tolist()) <= {0.5, 1.0, 2.0} and set(bn["cB"].unique().tolist()) <= {0.0, 0.5, -0.5}


@pytest.mark.parametrize("geom", [(2, 3, 7, 7, 5, 3, 1, 1, 1), (2, 5, 7, 8, 3, 3, 2, 1, 1), (2, 3, 7, 7, 5, 7, 1, 3, 1)], ids=str)
def test_reference_against_direct_loops(geom):
    B, Ci, H, W, Co, k, s, p, d = geom
    c = X.gen_case(11, B, Ci, H, W, Co, k, s, p, d, budget=1e9)
    assert np.array_equal(X.ref_fwd(c).numpy(), X.conv_np_int(c["x"].numpy(), c["w"].numpy(), s, p, d))
    assert np.array_equal(X.ref_dgrad(c, False).numpy(), X.dgrad_np_int(c["dy"].numpy(), c["w"].numpy(), (B, Ci, H, W), s, p, d))
    assert np.array_equal(X.ref_wgrad(c).numpy(), X.wgrad_np_int(c["x"].numpy(), c["dy"].numpy(), k, s, p, d))


def test_assert_same_places_the_differences():
    want = torch.zeros(2, 5, 6, 16, dtype=torch.float64)
    got = want.clone()
    got[1, 4, 5, 15] = 1.0
    got[1, 0, 2, 8] = -2.0
    with pytest.raises(AssertionError) as e:
        X.assert_same(got, want, "probe", "nhwc", tile=30)
    m = str(e.value)
    assert "2 of 960" in m and "image 1..1" in m and "2 on image borders" in m and "2 in the last 8-channel chunk" in m and "(1, 0, 2, 8): got -2.0 want 0.0" in m
    assert "1 on first/last pixels of 30-pixel tiles" in m
    X.assert_same(want, want.clone(), "same")


MUTATION_CASES = [X.CONV_CASES[8], X.CONV_CASES[9], X.CONV_CASES[3], X.CONV_CASES[1]]       # 13^2 256->512, 26x20 64->128, 1x1 64->255 + bias, stride-2 17x19


def differs_in_every(a, b, touched, dim, what):
    """a != b somewhere in every index of `dim` listed in `touched`"""
    diff = (a != b)
    other = tuple(i for i in range(a.dim()) if i != dim)
    per = diff.sum(other) > 0
    assert int(touched.sum()) > 0, f"{what}: the mutation touches nothing"
    assert bool(per[touched].all()), f"{what}: unchanged in channels {(touched & ~per).nonzero().flatten().tolist()[:8]}"


@pytest.mark.parametrize("case", MUTATION_CASES, ids=str)
def test_mutations_are_detected(case):
    c = X.conv_case(case)
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    y, dx, dw = X.ref_fwd(c), X.ref_dgrad(c), X.ref_wgrad(c)
    tu, tv = k - 1, k // 2                                    # the tap the mutations act on
    # (a) the last 8-channel chunk of one tap zeroed: forward (outputs whose weights there are not all zero) and data gradient (the chunk's channels)
    lo = (Ci - 1) // 8 * 8
    w = c["w"].clone()
    w[:, lo:, tu, tv] = 0
    differs_in_every(y, X.ref_fwd(c, w=w), c["w"][:, lo:, tu, tv].abs().sum(1) > 0, 1, "(a) forward")
    touched = torch.zeros(Ci, dtype=torch.bool)
    touched[lo:] = c["w"][:, lo:, tu, tv].abs().sum(0) > 0
    differs_in_every(dx, X.ref_dgrad(c, w=w), touched, 1, "(a) data gradient")
    # (b) one tap reads its neighbour column at the right image border only
    wt = torch.zeros_like(c["w"])
    wt[:, :, tu, tv] = c["w"][:, :, tu, tv]
    nobias = dict(c, bias=None)
    t_true = X.ref_fwd(nobias, w=wt)
    t_shift = X.ref_fwd(nobias, x=torch.roll(c["x"], 1, 3), w=wt)
    ym = y.clone()
    ym[..., -1] += t_shift[..., -1] - t_true[..., -1]
    differs_in_every(y, ym, wt.abs().sum((1, 2, 3)) > 0, 1, "(b) forward")
    # (c) the last output pixel of the tensor dropped from the weight gradient
    dy = c["dy"].clone()
    dy[-1, :, -1, -1] = 0
    differs_in_every(dw, X.ref_wgrad(c, dy=dy), c["dy"][-1, :, -1, -1] != 0, 0, "(c) weight gradient")
    # (d) one pad channel of the input holds 1 instead of 0 and the kernel treats it as live: modelled as an extra input channel of ones whose weight
    #     slot aliases channel 0's (a pad slot is only harmless while BOTH operands keep it zero)
    xm = torch.cat((c["x"], torch.ones(B, 1, H, W, dtype=torch.float64)), 1)
    wm = torch.cat((c["w"], c["w"][:, :1]), 1)
    ym = F.conv2d(xm, wm, c["bias"], stride=s, padding=p, dilation=d)
    differs_in_every(y, ym, c["w"][:, 0].abs().sum((1, 2)) > 0, 1, "(d) forward")
    #     ... and in the weight gradient: a pad channel of dy holding 1 whose row of dW lands on output channel 0
    dym = torch.cat((c["dy"], torch.ones(B, 1, c["Ho"], c["Wo"], dtype=torch.float64)), 1)
    row = torch.nn.grad.conv2d_weight(c["x"], (Co + 1, Ci, k, k), dym, stride=s, padding=p, dilation=d)[Co]
    dwm = dw.clone()
    dwm[0] += row
    touched = torch.zeros(Co, dtype=torch.bool)
    touched[0] = True
    differs_in_every(dw, dwm, touched, 0, "(d) weight gradient")
