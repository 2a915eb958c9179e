"""Pin tests/helpers/datamove_refs.py (the references of tests/test_gpu_datamove.py) to torch.nn.functional with autograd.  CPU only.

Every reference runs at the small shapes of the device test, on its inputs (helpers/datamove_refs has none of its own: the generators live
here in POOL_KINDS and the device test imports them), and is compared with `==` on bit patterns:
max_pool2d(return_indices=True) with the flat indices converted to window positions, interpolate(mode="nearest"), permute, and the
autograd gradient of each.  The one place where torch and the references part on purpose is a window of only -inf: torch points at the
first element inside the image, the references (and the kernels) keep idx = 0; idx is not compared there, and where position 0 of such a
window is padding its gradient goes nowhere instead of to that element, so the comparison of dx drops those windows' dy."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import datamove_refs as R  # noqa: E402

NAN, NINF = float("nan"), float("-inf")
POOL2_SHAPES = [(2, 13, 13), (2, 7, 9), (1, 13, 13), (1, 6, 9)]                                  # stride, H, W
POOL_KS = [(2, 2), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (5, 1), (13, 1), (2, 3), (1, 1)]       # k, stride; pad = (k - 1) // 2
POOL_HW = (13, 17)
UPS_CASES = [(1, 4, 6), (2, 5, 7), (3, 5, 7), (4, 3, 5)]                                         # scale, H, W
POOL_KINDS = ["randn", "plateau", "negative", "zeros", "neginf", "nan"]


def nan_codes(C, H, W):
    """[C, H // 2, W // 2]: which of the eight NaN patterns of pool_input("nan") each 2x2 block of each channel holds"""
    H2, W2 = H // 2, W // 2
    return (torch.arange(H2).view(1, H2, 1) * W2 + torch.arange(W2).view(1, 1, W2) + torch.arange(C).view(C, 1, 1)) % 8


NAN_IDX = torch.tensor([0, 1, 2, 3, 3, 2, 3])                      # the last NaN of patterns 0..6 in scan order


def pool_input(kind, B, C, H, W, seed=0):
    """float32 NCHW whose values are bf16 numbers (so both element types hold them, and randn ties often)"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * H + W)
    x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16).float()
    if kind == "plateau":                                          # a block of equal values and one whole constant channel
        x[:, :, 1:H - 1, 2:W - 1] = 0.5
        x[:, 1] = -1.25
    elif kind == "negative":                                       # stride 1: the zero padding wins on the last row and column
        x = -x.abs() - 0.25
    elif kind == "zeros":                                          # -0.0 against +0.0, a few negative values among them
        sign = torch.randint(0, 2, x.shape, generator=g).bool()
        x = torch.where(x < -1.0, x, torch.where(sign, torch.tensor(-0.0), torch.tensor(0.0)))
    elif kind == "neginf":                                         # scattered, and blocks that fill whole windows (top-left and bottom-right corners)
        x[torch.rand(x.shape, generator=g) < 0.3] = NINF
        x[:, :, :H // 2, :W // 2] = NINF
        x[:, 0::2, H - 3:, W - 4:] = NINF
    elif kind == "nan":
        # by 2x2 block (the windows of the stride-2 pool), eight patterns in turn, shifted by one per channel: one NaN at each of the four
        # positions, two NaN (0 and 3, 1 and 2), only NaN, none; then NaN on the last row / column of some channels and in the corner
        H2, W2 = H // 2, W // 2
        code = nan_codes(C, H, W)
        for cd, positions in enumerate([(0,), (1,), (2,), (3,), (0, 3), (1, 2), (0, 1, 2, 3)]):
            for p in positions:
                block = x[:, :, p // 2:2 * H2:2, p % 2:2 * W2:2]
                block[(code == cd).expand_as(block)] = NAN
        x[:, 0::3, H - 1, :] = NAN
        x[:, 1::3, :, W - 1] = NAN
        x[:, :, H - 1, W - 1] = NAN
    else:
        assert kind == "randn"
    return x.to(torch.bfloat16).float()


def int_grad(shape, n, seed):
    """integer-valued gradients with |d| <= 256 // n (at least 1): n of them sum exactly in bf16"""
    m = max(1, 256 // n)
    return torch.randint(-m, m + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def same(a, b):
    return torch.equal(R.bits(a), R.bits(b))


def torch_pool(x, k, s, pad, br_pad):
    """F.max_pool2d with autograd: y, idx as window positions (pad_pos where torch points into the bottom / right zero padding), dx of a given dy"""
    B, C, H, W = x.shape
    xr = x.clone().requires_grad_(True)
    xin = F.pad(xr, (0, 1, 0, 1)) if br_pad else xr
    y, ind = F.max_pool2d(xin, k, s, pad, return_indices=True)
    Wi = W + (1 if br_pad else 0)
    h, w = ind // Wi, ind % Wi
    Ho, Wo = y.shape[2:]
    oh = torch.arange(Ho).view(1, 1, Ho, 1) * s - pad
    ow = torch.arange(Wo).view(1, 1, 1, Wo) * s - pad
    pos = (h - oh) * k + (w - ow)
    pos = torch.where((h >= H) | (w >= W), torch.full_like(pos, 4), pos)
    return xr, y, pos.to(torch.uint8)


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("stride,H,W", POOL2_SHAPES)
def test_maxpool2x2_ref_is_torch(stride, H, W, kind):
    x = pool_input(kind, 2, 5, H, W)
    y, idx = R.maxpool2x2_ref(x, stride)
    xr, ty, tpos = torch_pool(x, 2, stride, 0, stride == 1)
    assert same(y, ty.detach())
    live = ty.detach() != NINF                                     # (a 2x2 window of only -inf: possible at stride 2 alone, the zero padding beats it at stride 1)
    assert torch.equal(idx[live], tpos[live])
    assert int(idx.max()) <= 4 and (stride == 1 or int(idx.max()) <= 3)
    dy = int_grad(y.shape, 4 if stride == 1 else 1, H)
    ty.backward(dy)
    dx = R.maxpool_bwd_ref(dy, idx, H, W, 2, stride, 0)
    assert torch.equal(dx, xr.grad.double())                       # position 0 of a 2x2 window is never padding: the -inf windows agree too
    if kind == "negative" and stride == 1:
        assert bool((idx[:, :, H - 1, :] == 4).all()) and bool((idx[:, :, :, W - 1] == 4).all()) and bool((idx[:, :, :H - 1, :W - 1] < 4).all())
    if kind == "nan" and stride == 2 and H % 2 and W % 2:          # (odd sizes: the NaN of the last row / column are in no window)
        code = nan_codes(5, H, W).expand(2, -1, -1, -1)
        assert torch.equal(torch.isnan(y), code < 7)
        assert torch.equal(idx[code < 7], NAN_IDX[code[code < 7]].to(torch.uint8))
        assert torch.equal(y[code == 7], F.max_pool2d(pool_input("randn", 2, 5, H, W), 2, 2)[code == 7])   # windows without a NaN are unchanged


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("k,s", POOL_KS)
def test_maxpool_ref_is_torch(k, s, kind):
    H, W = POOL_HW
    pad = (k - 1) // 2
    x = pool_input(kind, 2, 5, H, W)
    y, idx = R.maxpool_ref(x, k, s, pad)
    xr, ty, tpos = torch_pool(x, k, s, pad, False)
    assert y.shape == ty.shape and same(y, ty.detach())
    live = ty.detach() != NINF
    assert torch.equal(idx[live], tpos[live])
    assert bool((idx[~live] == 0).all())
    n = -(-k // s) ** 2
    dy = int_grad(y.shape, n, k * 10 + s) * live                   # (see the module docstring: the windows of only -inf)
    ty.backward(dy)
    assert torch.equal(R.maxpool_bwd_ref(dy, idx, H, W, k, s, pad), xr.grad.double())
    if kind == "neginf" and k <= 5:                                # (the 13-wide window always reaches a finite value)
        assert not bool(live.all())


def test_nan_rule_by_hand():
    """one 2x2 window per case, written out: NaN at each position, two NaN (the last one wins), only NaN, a NaN against the zero padding"""
    for where, want in [((0,), 0), ((1,), 1), ((2,), 2), ((3,), 3), ((0, 3), 3), ((1, 2), 2), ((0, 1, 2, 3), 3)]:
        x = torch.tensor([5.0, 7.0, -1.0, 6.0])
        x[list(where)] = NAN
        y, idx = R.maxpool2x2_ref(x.view(1, 1, 2, 2), 2)
        assert bool(torch.isnan(y).all()) and int(idx) == want
        y, idx = R.maxpool_ref(x.view(1, 1, 2, 2), 2, 2, 0)
        assert bool(torch.isnan(y).all()) and int(idx) == want
    y, idx = R.maxpool2x2_ref(torch.tensor([[1.0, 2.0], [3.0, NAN]]).view(1, 1, 2, 2), 1)
    assert torch.isnan(y).view(-1).tolist() == [True, True, True, True] and idx.view(-1).tolist() == [3, 2, 1, 0]
    y, idx = R.maxpool2x2_ref(torch.tensor([[1.0, 1.0], [1.0, 1.0]]).view(1, 1, 2, 2), 2)
    assert int(idx) == 0 and int(R.maxpool2x2_ref(torch.ones(1, 1, 2, 2), 2, last_max=True)[1]) == 3


def test_bwd_ref_with_made_up_idx():
    """every legal position, 4 and a value that is no position: a direct loop over windows, written from the definition"""
    for k, s, pad, H, W in [(2, 2, 0, 7, 9), (2, 1, 0, 6, 9), (3, 2, 1, 7, 5), (4, 1, 1, 5, 6), (2, 3, 0, 8, 7)]:
        br = (k, s, pad) == (2, 1, 0)
        Ho, Wo = (H, W) if br else (R.pool_out(H, k, s, pad), R.pool_out(W, k, s, pad))
        g = torch.Generator().manual_seed(k + s)
        idx = torch.randint(0, k * k + 2, (1, 2, Ho, Wo), generator=g)
        idx[idx == k * k + 1] = R.NONE
        idx = idx.to(torch.uint8)
        dy = int_grad((1, 2, Ho, Wo), 4, 3)
        want = torch.zeros(1, 2, H, W, dtype=torch.float64)
        for c in range(2):
            for oh in range(Ho):
                for ow in range(Wo):
                    p = int(idx[0, c, oh, ow])
                    h, w = oh * s - pad + p // k, ow * s - pad + p % k
                    if p < k * k and 0 <= h < H and 0 <= w < W:
                        want[0, c, h, w] += float(dy[0, c, oh, ow])
        assert torch.equal(R.maxpool_bwd_ref(dy, idx, H, W, k, s, pad), want)


@pytest.mark.parametrize("sc,H,W", UPS_CASES)
def test_upsample_refs_are_torch(sc, H, W):
    x = pool_input("nan", 2, 5, H + 4, W + 4)[:, :, :H, :W].clone().requires_grad_(True)
    ty = F.interpolate(x, scale_factor=sc, mode="nearest")
    assert same(R.upsample_ref(x.detach(), sc), ty.detach())
    dy = int_grad(ty.shape, sc * sc, sc)
    ty.backward(dy)
    assert torch.equal(R.upsample_bwd_ref(dy, sc), x.grad.double())


@pytest.mark.parametrize("dt", [R.BF16, R.F32])
def test_layout_refs_are_permute(dt):
    x = torch.randn(2, 5, 3, 4)
    x[0, 0, 0, :3] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38])     # bf16 ties (to even: down, up) and a value that rounds to inf
    b = R.nhwc_of(x, 16, dt)
    assert b.dtype == R.TD[dt] and b.shape == (2, 3, 4, 16)
    assert torch.equal(b[..., :5], x.permute(0, 2, 3, 1).to(R.TD[dt])) and torch.equal(R.bits(b[..., 5:]), torch.zeros(2, 3, 4, 11, dtype=R.bits(b).dtype))
    if dt == R.BF16:
        assert b[0, 0, :3, 0].float().tolist() == [1.0, 1 + 2.0 ** -6, float("inf")]
    assert torch.equal(R.nchw_of(b, 5), R.rnd(x, dt)) and R.nchw_of(b, 5).is_contiguous()


@pytest.mark.parametrize("dt", [R.BF16, R.F32])
def test_pack_ref_is_the_definition(dt):
    for Co, Ci, k, cop, cip in [(5, 3, 3, 8, 8), (7, 12, 1, 8, 16), (2, 3, 2, 16, 8)]:
        w = torch.randn(Co, Ci, k, k)
        wf, wd = R.pack_ref(w, cop, cip, dt)
        assert wf.shape == (cop, k * k, cip) and wd.shape == (cip, k * k, cop) and wf.dtype == R.TD[dt]
        for n in range(cop):
            for t in range(k * k):
                for ci in range(cip):
                    want = R.rnd(w[n, ci, t // k, t % k], dt) if n < Co and ci < Ci else 0.0
                    assert float(wf[n, t, ci]) == float(want) and float(wd[ci, t, n]) == float(want)
        assert torch.equal(wf[:Co, :, :Ci], w.permute(0, 2, 3, 1).reshape(Co, k * k, Ci).to(R.TD[dt]))
