"""Integer-valued convolution cases whose every product and partial sum is exact in fp32 and whose every bf16 output is representable:
generator, float64 references written from the definition of each operation, the conditions that make `==` the right comparison, and
an exact comparison whose failure message places the differences (tests/test_conv_exact_host.py, tests/test_gpu_conv_exact.py).

Data rule.  Activations and output gradients are uniform in {-2..2}; weights are a random sign times a Bernoulli mask of density
q = min(1, 600 / (KH KW max(Cin, Cout))) (about 600 non-zero weights per output, so |y| stays below 256); addsrc is uniform in {-4..4};
bias in {-3..3}.  The fused BatchNorm forms take dyadic coefficients: scale in {+-1/2, +-1, +-2}, shift / mean / cC small integers, cA in
{1/2, 1, 2}, cB in {0, +-1/2}, leaky slope 0.5.  The producer layer's y is an integer in {-4..4}, EVEN where |scale| = 1/2 (so that
scale*y + shift is an integer and act(.) a multiple of 1/2), and it AVOIDS THE ROOT ALTOGETHER: wherever scale*y + shift would be 0 the
element is moved one step (two where |scale| = 1/2) away, so act'(0) never decides a comparison.

Nothing here needs a GPU or the library."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.5                      # the exact tests' leaky slope (0.1 is not a dyadic number)
TWO24 = float(1 << 24)
# Largest number of pixels one partial-statistics row covers: a 384-row ping-pong tile of the 3x3 shift kernel writes ONE row
# (csrc/conv_shift.hip: `constexpr int GR = (BM == 128 || BM == 256) ? 128 : BM;`); every other kernel writes a row per <= 256 pixels.
ROWS_MAX = 384


def pad8(c):
    return (c + 7) // 8 * 8


def out_hw(H, W, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def density(k, ci, co, budget=600.0):
    return min(1.0, budget / (k * k * max(ci, co)))


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _pick(g, n, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def gen_bn(g, shape, yr=4, shr=3):
    """Producer-layer tensors of a fused BatchNorm form for an NCHW `shape`: y (raw conv output of the layer whose BatchNorm is fused) and the
    per-channel vectors scale / shift / mean / cA / cB / cC.  scale*y + shift is a non-zero integer everywhere (module docstring)."""
    C = shape[1]
    scale = _pick(g, C, [0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    scale[:6] = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[:min(6, C)]          # every value, negative ones included, at any C
    shift = _ints(g, (C,), -shr, shr)
    mean = _ints(g, (C,), -2, 2)
    cA = _pick(g, C, [0.5, 1.0, 2.0])
    cB = _pick(g, C, [0.0, 0.5, -0.5])
    cC = _ints(g, (C,), -2, 2)
    y = _ints(g, shape, -yr, yr)
    half = (scale.abs() == 0.5).view(1, C, 1, 1)
    step = torch.where(half, 2.0, 1.0).double()
    y = torch.where(half, 2.0 * torch.div(y, 2, rounding_mode="trunc"), y)
    pre = scale.view(1, C, 1, 1) * y + shift.view(1, C, 1, 1)
    y = torch.where(pre == 0, y + step, y)
    pre = scale.view(1, C, 1, 1) * y + shift.view(1, C, 1, 1)
    assert bool((pre != 0).all()) and bool((pre == pre.round()).all())
    return dict(y=y, scale=scale, shift=shift, mean=mean, cA=cA, cB=cB, cC=cC)


def gen_case(seed, B, Ci, H, W, Co, k, s=1, p=None, d=1, bias=False, budget=600.0):
    """Integer-valued float64 CPU tensors of one conv layer Ci -> Co (NCHW / OIHW) from a seeded generator: x, w, bias (or None), dy, addsrc (for the
    data gradient, shape of x) and resid (shape of y); `bn_in` / `bn_out`: producer-layer tensors (gen_bn) on the input / output grid."""
    p = (d * (k - 1)) // 2 if p is None else p
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(H, W, k, s, p, d)
    q = density(k, Ci, Co, budget)
    x = _ints(g, (B, Ci, H, W), -2, 2)
    sign = _ints(g, (Co, Ci, k, k), 0, 1) * 2 - 1
    w = sign * (torch.rand(Co, Ci, k, k, generator=g, dtype=torch.float64) < q).double()
    b = _ints(g, (Co,), -3, 3) if bias else None
    dy = _ints(g, (B, Co, Ho, Wo), -2, 2)
    add = _ints(g, (B, Ci, H, W), -4, 4)
    resid = _ints(g, (B, Co, Ho, Wo), -4, 4)
    return dict(x=x, w=w, bias=b, dy=dy, addsrc=add, resid=resid, geom=(B, Ci, H, W, Co, k, s, p, d), Ho=Ho, Wo=Wo, q=q,
                bn_in=gen_bn(g, (B, Ci, H, W)), bn_out=gen_bn(g, (B, Co, Ho, Wo)))


# ---- references: torch CPU float64, from the definition of each operation

def ref_fwd(c, x=None, w=None):
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    return F.conv2d(c["x"] if x is None else x, c["w"] if w is None else w, c["bias"], stride=s, padding=p, dilation=d)


def ref_dgrad(c, with_add=True, w=None, dy=None):
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    dx = torch.nn.grad.conv2d_input((B, Ci, H, W), c["w"] if w is None else w, c["dy"] if dy is None else dy, stride=s, padding=p, dilation=d)
    return dx + c["addsrc"] if with_add else dx


def ref_wgrad(c, x=None, dy=None):
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    return torch.nn.grad.conv2d_weight(c["x"] if x is None else x, (Co, Ci, k, k), c["dy"] if dy is None else dy, stride=s, padding=p, dilation=d)


def act(pre, code, slope=SLOPE):
    return pre if code == 0 else torch.where(pre > 0, pre, pre * (slope if code == 1 else 0.0))


def dact(pre, code, slope=SLOPE):
    return torch.ones_like(pre) if code == 0 else torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope if code == 1 else 0.0))


def _cv(v):
    return v.view(1, -1, 1, 1)


def ref_bn_fwd(bn, code, resid=None):
    """z = act(scale*y + shift) (+ resid)"""
    z = act(_cv(bn["scale"]) * bn["y"] + _cv(bn["shift"]), code)
    return z if resid is None else z + resid


def ref_bn_sums(bn, dz, code):
    """g = dz * act'(scale*y + shift); returns g, sum g, sum g (y - mean) per channel"""
    g = dz * dact(_cv(bn["scale"]) * bn["y"] + _cv(bn["shift"]), code)
    return g, g.sum((0, 2, 3)), (g * (bn["y"] - _cv(bn["mean"]))).sum((0, 2, 3))


def ref_bn_apply(bn, dz, code):
    """dy = cA*g + cB*y + cC"""
    g = dz * dact(_cv(bn["scale"]) * bn["y"] + _cv(bn["shift"]), code)
    return _cv(bn["cA"]) * g + _cv(bn["cB"]) * bn["y"] + _cv(bn["cC"])


# ---- the conditions under which `==` is the right comparison

def bf16_exact(t):
    """True where every element of the float64 tensor is a bf16 number"""
    return bool(torch.equal(t.to(torch.bfloat16).double(), t))


def quantum(t):
    """Largest power of two (<= 1) that divides every element"""
    q = 1.0
    while q > 2.0 ** -8 and not bool(torch.equal((t / q).round() * q, t)):
        q /= 2
    return q


def check_exact_preconditions(tensors):
    """`tensors`: dict name -> (kind, float64 tensor) with kind in
         'bf16'   an expected bf16 output: every element representable in bf16;
         'fp32'   an expected fp32 output whose every partial sum is bounded by sum |terms| <= the given tensor of ABSOLUTE sums (pass the
                  reference computed on |operands|): below 2^24 quanta;
         'terms'  the per-pixel terms of a per-channel statistic whose partial rows have a pixel membership internal to the kernel:
                  ROWS_MAX * max|term| < 2^24 quanta (sufficient whatever pixels a row holds).
       Conditions, not measurements: asserted from the reference alone."""
    for name, spec in tensors.items():
        kind, t = spec[0], spec[1]
        rows_max = spec[2] if len(spec) > 2 else ROWS_MAX          # ('terms', t, rows): a kernel whose rows cover at most `rows` pixels
        assert bool(torch.isfinite(t).all()), name
        if kind == "bf16":
            assert bf16_exact(t), f"{name}: not representable in bf16 (max |v| {float(t.abs().max())}, quantum {quantum(t)})"
        elif kind == "fp32":
            assert float(t.abs().max()) / quantum(t) < TWO24, f"{name}: sum of |terms| {float(t.abs().max())} at quantum {quantum(t)} reaches 2^24"
        elif kind == "terms":
            assert rows_max * float(t.abs().max()) / quantum(t) < TWO24, f"{name}: {rows_max} x {float(t.abs().max())} at quantum {quantum(t)} reaches 2^24"
        else:
            raise ValueError(kind)


def conv_conditions(c, fwd=True, dgrad=True, wgrad=True, stats=True):
    """The tensors check_exact_preconditions needs for a plain conv case (forward y with its statistics, data gradient + addsrc, weight gradient)."""
    out = {}
    if fwd:
        y = ref_fwd(c)
        out["y"] = ("bf16", y)
        if stats:
            out["stats y"] = ("terms", y)
            out["stats y^2"] = ("terms", y * y)
    if dgrad:
        out["dx + addsrc"] = ("bf16", ref_dgrad(c))
        out["dx (fp32 accumulator, |terms|)"] = ("fp32", ref_dgrad(c, False, w=c["w"].abs(), dy=c["dy"].abs()))
    if fwd:
        ca = dict(c, bias=None)
        out["y (fp32 accumulator, |terms|)"] = ("fp32", ref_fwd(ca, x=c["x"].abs(), w=c["w"].abs()))
    if wgrad:
        out["dW (|terms|)"] = ("fp32", ref_wgrad(c, x=c["x"].abs(), dy=c["dy"].abs()))
    return out


# ---- exact comparison with a failure message that places the differences

def assert_same(got, want, what, layout="nhwc", tile=128, extra=""):
    """Exact equality of two CPU tensors of one shape.  layout 'nhwc': [image, row, column, channel]; 'oihw': [cout, cin, kh, kw]; 'rows': anything
    else.  The message: count of differing elements, their bounding box, where they sit (image borders, borders of `tile`-pixel tiles of the flat
    pixel stream, the last 8-channel chunk), and the first ten (index, got, want)."""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    bad = got != want
    bad |= torch.isnan(got) | torch.isnan(want)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
    names = {"nhwc": ("image", "row", "column", "channel"), "oihw": ("cout", "cin", "kh", "kw")}.get(layout, tuple(f"d{i}" for i in range(got.dim())))
    box = ", ".join(f"{nm} {a}..{b} of {sz}" for nm, a, b, sz in zip(names, lo, hi, got.shape))
    where = []
    if layout == "nhwc":
        _, H, W, C = got.shape
        r, col, ch = idx[:, 1], idx[:, 2], idx[:, 3]
        flat = (idx[:, 0] * H + r) * W + col
        border = (r == 0) | (r == H - 1) | (col == 0) | (col == W - 1)
        seam = (flat % tile == 0) | (flat % tile == tile - 1)
        last = ch >= (C - 1) // 8 * 8
        where = [f"{int(border.sum())} on image borders (share of all elements there: {2 * (H + W - 2) / max(1, H * W):.2f})",
                 f"{int(seam.sum())} on first/last pixels of {tile}-pixel tiles of the flat stream", f"{int(last.sum())} in the last 8-channel chunk",
                 f"distinct flat pixels {int(flat.unique().numel())}, distinct channels {int(ch.unique().numel())}"]
    elif layout == "oihw":
        where = [f"{int((idx[:, 1] >= (got.shape[1] - 1) // 8 * 8).sum())} in the last 8-channel chunk of cin",
                 f"taps hit: {sorted(set(map(tuple, idx[:, 2:].tolist())))[:9]}"]
    first = "; ".join(f"{tuple(i.tolist())}: got {float(got[tuple(i)])!r} want {float(want[tuple(i)])!r}" for i in idx[:10])
    d = (got - want)[bad]
    raise AssertionError(f"{what}: {n} of {got.numel()} elements differ {extra}\n  box: {box}\n  " + "\n  ".join(where) +
                         f"\n  difference min {float(d.min())} max {float(d.max())}\n  first: {first}")


# ---- case tables of tests/test_gpu_conv_exact.py (the host test proves the conditions at every one of them before anything is launched).
# Tables that exist in tests/test_gpu_kernels.py are taken from there by the GPU file and checked against these copies.

CONV_CASES = [  # B, Cin, H, W, Cout, k, stride, pad, dil, bias
    (2, 3, 20, 20, 16, 3, 1, 1, 1, False), (2, 16, 17, 19, 32, 3, 2, 1, 1, False), (3, 32, 13, 13, 64, 1, 1, 0, 1, False),
    (2, 64, 13, 13, 255, 1, 1, 0, 1, True), (2, 3, 24, 24, 16, 7, 1, 3, 1, True), (2, 16, 20, 20, 32, 3, 1, 2, 2, True),
    (1, 128, 9, 9, 7, 1, 1, 0, 1, True), (2, 48, 11, 11, 136, 3, 1, 1, 1, False), (1, 256, 13, 13, 512, 3, 1, 1, 1, False),
    (3, 64, 26, 20, 128, 3, 1, 1, 1, True), (2, 32, 52, 52, 256, 3, 1, 1, 1, False), (5, 96, 8, 9, 128, 3, 1, 1, 1, False),
    (1, 128, 104, 104, 128, 3, 1, 1, 1, False)]
VARIANT_CASES = [(2, 72, 15, 17, 255, 3, 1, 1, 1, True), (2, 136, 14, 14, 144, 3, 2, 1, 1, False), (3, 256, 9, 9, 160, 1, 1, 0, 1, False),
                 (2, 96, 12, 12, 192, 3, 1, 2, 2, True)]
# Narrow outputs (<= 64 channels; csrc/conv_gemm.h dispatch_conv, the branch below `if (a.Nout > 64)`), none of them shift-eligible (Cin % 32 != 0 or
# Nout not 32 / 64 / a multiple of 128), each with M >= 1024 output positions so that code 2001 turns the 256-row tiles ON and 2000 OFF:
#   40 -> 48 at 30 x 34 (forward Nout 48, data gradient Nout 40: 256 x 64 / 128 x 64 tiles, 11 / 13 K steps: code 30 switches their 3-stage ring),
#   16 -> 32 at 40 x 40 (forward Nout 32: 256 x 32 ; data gradient Nout 16: 256 x 16), and CONV_CASES[4] (7x7 3 -> 16 at 24 x 24: 256 x 16).
NARROW_CASE = (2, 40, 30, 34, 48, 3, 1, 1, 1, False)
NARROW_CASES = [NARROW_CASE, (2, 16, 40, 40, 32, 3, 1, 1, 1, False), (2, 3, 24, 24, 16, 7, 1, 3, 1, True)]
# Wide outputs (> 64 channels) on the generic kernels with >= 8 K steps of 32 forward: the default takes the 3-stage ring (conv_deep_small = 8), code 60 the
# 2-stage 128 x 64 tiles.  VARIANT_CASES[1] (stride 2, 136 -> 144: 38 K steps) and [2] (1x1 256 -> 160: 8 K steps)
DEEP_SMALL_CASES = [(2, 136, 14, 14, 144, 3, 2, 1, 1, False), (3, 256, 9, 9, 160, 1, 1, 0, 1, False)]
# A 1x1 layer whose data gradient has MORE than 64 channels (dx = 256): only there does dispatch_conv read conv_fuse_narrow -- 93 (default): 128 x 64 tiles
# on the 3-stage ring for the fused 1x1 data gradient ; 92: the heuristic's choice (here 128 x 64 tiles, 2 stages: 8 tiles of 128 x 128, 4 K steps)
FUSE1X1_CASE = (2, 256, 14, 14, 128, 1, 1, 0, 1, False)
# Rows of 63..80 pixels: the four-DMA chunk of the 1-D stream under -14 (shift_wmax 80), 2-D pixel tiles under -15 (62).  The fourth DMA exists on 256-row
# tiles only (256 + 2 * 72 halo rows = 26 KiB-chunks; a 128-row tile of this width needs 17: three DMAs), and shift_plan_bm gives 256-row tiles to grids of
# 129..256 tiles where 192-row tiles save no round: Mq = 11 * 9 * 71 = 7029 -> 28 x 7 = 196 tiles of 256 (one round), 37 x 7 = 259 of 192 (two rounds);
# the kernel takes images of at least 8 rows; 1.59e9 multiply-adds, just inside MACS_CAP.
# (Until the kernel census the case was (1, 32, 9, 70, 128): 3 tiles, 128 rows, three DMAs under BOTH codes.)
SHIFT_W70 = (11, 32, 8, 70, 896)


def c3(t, bias=False, dil=1):
    """(B, Cin, H, W, Cout) of a 3x3 stride-1 layer -> the 10-tuple of CONV_CASES"""
    B, Ci, H, W, Co = t
    return (B, Ci, H, W, Co, 3, 1, dil, dil, bias)


SHIFT_CASES = [(3, 64, 26, 20, 128), (5, 96, 8, 9, 128), (1, 256, 13, 13, 512), (4, 64, 26, 26, 256), (9, 32, 30, 17, 128), (33, 64, 13, 13, 64),
               (1, 128, 104, 104, 128)]
SHIFT_CODES = [-8, -9, -12, -30, -31, -201, -3, -4, -17, -18, -19, -15, -14]
# The 64-wide data-gradient tiles of layers with few positions and > 64 channels (-64 / -63): Cin -> Cout of the LAYER.  The first case has 4 x 8 = 32
# tiles and runs 128 x 64 tiles; 256 x 64 -- what the 13^2 layers run at batch 32 (25 x 8 = 200 tiles) -- needs 129..256 tiles of 256 x 64 that are at most 128
# tiles of 256 x 128, and more than 256 tiles of 192 x 64: 256 -> 32 at 13 x 13, B = 63: Mq = 12348 -> 49 x 4 = 196 tiles (98 of 256 x 128; 65 x 4 = 260 of 192).
# (Until the kernel census the table was the first and the third case, 128 x 64 tiles both.)
SHIFT_WIDE_DGRAD = [(4, 512, 13, 13, 1024), (63, 256, 13, 13, 32), (2, 512, 13, 11, 1024)]
SHIFT_2D = [(2, 32, 97, 131, 128), (1, 128, 9, 161, 128), (2, 32, 41, 300, 32)]
SHIFT_DIL2 = [(3, 64, 26, 26, 64), (4, 32, 30, 17, 32)]
# B, Cin, H, W, Cout of a 3x3 / stride-2 / pad-1 layer.  Odd sizes: four parity-class launches under every code.  Even sizes with MORE than 64 input
# channels (dx = 128 channels: 64 and 32 go to the shift kernel's stride-2 form, S2D_CASES): one launch for the four classes (ALLCLS), csrc/conv_igemm.hip
S2_CASES = [(2, 64, 17, 19, 128), (2, 128, 16, 20, 128)]
S2D_CASES = [(3, 32, 17, 45, 32), (2, 64, 8, 31, 64), (1, 32, 9, 63, 32), (1, 128, 52, 52, 64)]   # B, Cdy, Hdy, Wdy, Cdx (test_gpu_kernels.S2D_CASES)
FUSE_CASES = [(2, 64, 26, 20, 128, 3, 1, 1), (5, 128, 13, 13, 256, 3, 1, 1), (2, 256, 14, 14, 128, 1, 1, 0), (2, 64, 17, 19, 128, 3, 2, 1),
              (3, 32, 20, 20, 48, 3, 1, 1), (2, 16, 24, 24, 32, 3, 1, 2), (2, 64, 15, 17, 72, 3, 1, 1)]
WGRAD_SHIFT_CASES = [(2, 128, 13, 13, 128), (3, 128, 26, 20, 256), (1, 256, 52, 52, 128), (5, 128, 9, 8, 128)]
# The kw-shared-tile kernel (csrc/wgrad_shift.hip) comes AFTER the LDS-ring kernel in choose_wgrad_family (csrc/conv_igemm.hip), and the ring kernel takes every
# layer of WGRAD_SHIFT_CASES: code 8 moves none of them.  It is reached where the ring kernel is not eligible -- images of so few rows that one 64-position step
# wraps more than one image (csrc/wgrad_stream.hip: bp / (W + 1) + 1 >= H + 1): 7 rows of 8 pixels.
WGRAD_KWSHARED_CASES = [(5, 128, 7, 8, 128)]
WGRAD_STREAM_CASES = [(2, 16, 16, 12, 9, 1), (2, 16, 32, 30, 17, 2), (2, 32, 64, 40, 33, 2), (3, 64, 64, 26, 20, 1), (2, 64, 128, 80, 80, 2),
                      (1, 64, 128, 104, 104, 1), (5, 64, 64, 5, 4, 1), (2, 128, 256, 26, 26, 1), (3, 256, 128, 13, 13, 1), (1, 128, 128, 80, 80, 1),
                      (2, 192, 384, 9, 11, 1), (2, 128, 128, 20, 17, 2), (4, 512, 1024, 13, 13, 1)]
WGRAD_DIRECT_CASES = [(2, 512, 1024, 13, 11, 1), (4, 512, 1024, 13, 13, 1)]
WGRAD_S2_CASES = [(2, 32, 64, 13, 13, 0), (3, 64, 128, 9, 14, 0), (2, 128, 256, 26, 26, 0), (1, 32, 64, 52, 52, 0), (4, 96, 192, 5, 4, 0), (2, 64, 64, 40, 7, 0),
                  (5, 32, 128, 13, 11, 8)]
STEM_CASES = [(3, 33, 20), (5, 9, 12)]
BNAPPLY_CASES = [(2, 3, 40, 56, 32, 3, 1, 1, 1), (3, 3, 33, 47, 16, 3, 1, 1, 1), (2, 5, 30, 30, 32, 3, 2, 1, 1), (1, 8, 64, 40, 24, 1, 1, 0, 0)]
PW_CASES = [(64 * 21 + 17, 256, 128, 0, True, 1), (64 * 9, 128, 64, 8, True, 1), (3000, 64, 128, 0, False, 1), (32 * 40 + 5, 512, 256, 16, True, 1),
            (16 * 70 + 3, 1024, 512, 0, True, 1), (2000, 256, 24, 0, False, 2), (1100, 128, 256, 8, True, 0)]
PWB_CASES = [(32 * 21 + 17, 256, 256, 512, 0, True), (5408, 512, 512, 1024, 0, True), (3000, 128, 128, 256, 8, False), (2703, 256, 255, 256, 0, False),
             (700, 64, 64, 128, 16, True), (1100, 256, 256, 768, 8, True), (96, 128, 128, 64, 0, False)]
FIRST_CASES = [(3, 3, 37, 53, 1), (1, 3, 5, 16, 0), (2, 1, 30, 95, 2), (1, 3, 64, 640, 1)]
AFFINE_CASES = [(3, 128, 26, 26, 256, 3, 1, True, 1), (2, 256, 13, 13, 128, 1, 1, False, 1), (2, 64, 30, 30, 128, 3, 2, False, 1),
                (2, 16, 40, 40, 32, 3, 1, False, 2), (1, 32, 20, 17, 64, 3, 1, True, 0), (2, 8, 24, 24, 16, 7, 1, False, 2)]
MACS_CAP = 1.6e9                  # "about 1.5e9 multiply-adds" per CPU reference; the largest case used (104^2 128 -> 128) has 1.59e9


def macs(case):
    B, Ci, H, W, Co, k, s, p, d = case[:9]
    Ho, Wo = out_hw(H, W, k, s, p, d)
    return B * Ho * Wo * k * k * Ci * Co


def seed_of(case):
    return sum((i + 1) * int(v) for i, v in enumerate(case)) % 100003


@functools.lru_cache(maxsize=16)
def conv_case(case):
    """gen_case for a 10-tuple of CONV_CASES, cached (shared; callers do not modify it)."""
    B, Ci, H, W, Co, k, s, p, d, bias = case
    assert macs(case) <= MACS_CAP, case
    return gen_case(seed_of(case), B, Ci, H, W, Co, k, s, p, d, bias)


@functools.lru_cache(maxsize=16)
def conv_refs(case):
    """A new dict: conv_case(case) with its references beside it (_y forward, _dxa / _dx data gradient with / without addsrc, _dw weight gradient),
    computed once and shared among the tests that need them; callers do not modify it."""
    c = conv_case(case)
    return dict(c, _y=ref_fwd(c), _dxa=ref_dgrad(c, True), _dx=ref_dgrad(c, False), _dw=ref_wgrad(c))


def fused_dgrad_conditions(c, codes=(0, 1, 2), adds=(True, False)):
    """mdcv_conv2d_dgrad_bnsums / mdcv_pw_bwd: dx (+ addsrc) a bf16 number; the terms g and g (y - mean) of the per-channel sums.  A partial row of the
    shift kernel's stride-2 form covers the 16 x 62 output pixels of one 8 x 31 tile (include/mdcv_hip.h, mdcv_conv2d_dgrad_s2_form_ok): 1024 bounds every form."""
    out = {}
    bn = c["bn_in"]
    for a in adds:
        dz = ref_dgrad(c, a)
        out[f"dx add={a}"] = ("bf16", dz)
        for code in codes:
            g, _, _ = ref_bn_sums(bn, dz, code)
            out[f"g add={a} act={code}"] = ("terms", g, 1024)
            out[f"g (y - mean) add={a} act={code}"] = ("terms", g * (bn["y"] - _cv(bn["mean"])), 1024)
    return out


def bnapply_conditions(case):
    B, Ci, H, W, Co, k, s, p, code = case
    c = conv_case((B, Ci, H, W, Co, k, s, p, 1, False))
    dy = ref_bn_apply(c["bn_out"], c["dy"], code)
    return {"dy = cA g + cB y + cC": ("bf16", dy), "dW (|terms|)": ("fp32", ref_wgrad(c, x=c["x"].abs(), dy=dy.abs()))}


@functools.lru_cache(maxsize=4)
def pw_refs(case):
    """(M, K, N, extra stride, resid, act) of PW_CASES: mdcv_pw_conv_fwd as a 1x1 layer K -> N over an M x 1 image.  z = act(scale y + shift) (+ resid)
    is a multiple of 1/2 and out = z . W^T (+ bias) a sum of them: smaller values and fewer non-zero weights than the plain rule keep |out| <= 128
    (y in {-2..2}, shift in {-1..1}, resid in {-2..2}, 48 non-zero weights per output).  One partial row per tile of <= 64 pixels
    (csrc/pw_block.hip mdcv_pw_tile_rows)."""
    M, K, N, xs, with_r, a = case
    c = gen_case(seed_of(case[:4]) + 1, 1, K, M, 1, N, 1, 1, 0, 1, bias=(a == 2), budget=48.0)
    g = torch.Generator().manual_seed(seed_of(case[:4]) + 2)
    bn = gen_bn(g, (1, K, M, 1), yr=2, shr=1)
    resid = _ints(g, (1, K, M, 1), -2, 2)
    z = ref_bn_fwd(bn, a, resid if with_r else None)
    out = F.conv2d(z, c["w"], c["bias"])
    cond = {"z": ("bf16", z), "out": ("bf16", out), "out (|terms|)": ("fp32", F.conv2d(z.abs(), c["w"].abs())),
            "stats out": ("terms", out, 64), "stats out^2": ("terms", out * out, 64)}
    return dict(c=c, bn=bn, resid=resid, z=z[0, :, :, 0].t().contiguous(), out=out[0, :, :, 0].t().contiguous(), cond=cond)


@functools.lru_cache(maxsize=4)
def pwb_refs(case):
    """(M, Cout padded, Cout real, Cin, extra stride, addsrc) of PWB_CASES: the backward of a 1x1 layer Cin -> Cout over an M x 1 image"""
    M, K, Kr, N, xs, with_add = case
    c = gen_case(seed_of(case[:5]) + 3, 1, N, M, 1, Kr, 1, 1, 0, 1)
    cond = fused_dgrad_conditions(c, codes=(1,), adds=(with_add,))
    cond["dW (|terms|)"] = ("fp32", ref_wgrad(c, x=c["x"].abs(), dy=c["dy"].abs()))
    return dict(c=c, dx=ref_dgrad(c, False), dxa=ref_dgrad(c, True), dw=ref_wgrad(c), cond=cond)


@functools.lru_cache(maxsize=4)
def first_refs(case):
    """(B, Cin, H, W, act) of FIRST_CASES: 3x3 conv Cin -> 32, then z = act(scale y + shift) with dyadic scale / shift.  One partial row per strip of
    4 output rows (csrc/first_conv.hip: `constexpr int TR = 4;`)."""
    B, Ci, H, W, a = case
    c = gen_case(seed_of(case) + 4, B, Ci, H, W, 32, 3)
    y = ref_fwd(c)
    scale, shift = c["bn_out"]["scale"], c["bn_out"]["shift"]
    z = act(_cv(scale) * y + _cv(shift), a)
    cond = {"y": ("bf16", y), "z": ("bf16", z), "stats y": ("terms", y, 4 * W), "stats y^2": ("terms", y * y, 4 * W)}
    return dict(c=c, y=y, z=z, scale=scale, shift=shift, cond=cond)


@functools.lru_cache(maxsize=4)
def affine_refs(case):
    """(B, Cin, H, W, Cout, k, stride, resid, act) of AFFINE_CASES: out = act(conv(x) scale + shift) (+ resid); 150 non-zero weights per output keep
    2 |conv| + 3 + 4 a bf16 number."""
    B, Ci, H, W, Co, k, s, with_r, a = case
    c = gen_case(seed_of(case) + 5, B, Ci, H, W, Co, k, s, (k - 1) // 2, 1, budget=150.0)
    y = ref_fwd(c)
    scale, shift = c["bn_out"]["scale"], c["bn_out"]["shift"]
    out = act(_cv(scale) * y + _cv(shift), a)
    if with_r:
        out = out + c["resid"]
    cond = {"out": ("bf16", out), "conv (|terms|)": ("fp32", ref_fwd(c, x=c["x"].abs(), w=c["w"].abs()))}
    return dict(c=c, out=out, scale=scale, shift=shift, cond=cond)


def conv_np_int(x, w, s, p, d):
    """Independent direct-loop int64 forward conv (numpy): y[b, o, i, j] = sum x[b, c, i s - p + u d, j s - p + v d] w[o, c, u, v]"""
    x, w = np.asarray(x, dtype=np.int64), np.asarray(w, dtype=np.int64)
    B, C, H, W = x.shape
    O, _, KH, KW = w.shape
    Ho, Wo = out_hw(H, W, KH, s, p, d)
    y = np.zeros((B, O, Ho, Wo), dtype=np.int64)
    for b in range(B):
        for i in range(Ho):
            for j in range(Wo):
                for u in range(KH):
                    for v in range(KW):
                        r, q = i * s - p + u * d, j * s - p + v * d
                        if 0 <= r < H and 0 <= q < W:
                            y[b, :, i, j] += w[:, :, u, v] @ x[b, :, r, q]
    return y


def dgrad_np_int(dy, w, xshape, s, p, d):
    dy, w = np.asarray(dy, dtype=np.int64), np.asarray(w, dtype=np.int64)
    B, C, H, W = xshape
    O, _, KH, KW = w.shape
    dx = np.zeros(xshape, dtype=np.int64)
    for b in range(B):
        for i in range(dy.shape[2]):
            for j in range(dy.shape[3]):
                for u in range(KH):
                    for v in range(KW):
                        r, q = i * s - p + u * d, j * s - p + v * d
                        if 0 <= r < H and 0 <= q < W:
                            dx[b, :, r, q] += w[:, :, u, v].T @ dy[b, :, i, j]
    return dx


def wgrad_np_int(x, dy, k, s, p, d):
    x, dy = np.asarray(x, dtype=np.int64), np.asarray(dy, dtype=np.int64)
    B, C, H, W = x.shape
    O = dy.shape[1]
    dw = np.zeros((O, C, k, k), dtype=np.int64)
    for b in range(B):
        for i in range(dy.shape[2]):
            for j in range(dy.shape[3]):
                for u in range(k):
                    for v in range(k):
                        r, q = i * s - p + u * d, j * s - p + v * d
                        if 0 <= r < H and 0 <= q < W:
                            dw[:, :, u, v] += np.outer(dy[b, :, i, j], x[b, :, r, q])
    return dw


# ---- dense grids: the instantiations the production plans launch and the small grids above cannot reach (tests/test_gpu_conv_census.py).
# launch_shift_f (csrc/conv_shift.hip) picks the ping-pong K loop (LOOP = 1) and the 4-slot weight ring (BRING = 4) for grids of at most 256 tiles, and
# every table above stays below that; the forms the 52^2 layers of the benchmark run (forward BRING = 3, LOOP = 0; fused data gradient FUSE, BRING = 3)
# need MORE than 256 tiles under the default code.  Many output channels over few positions is the cheapest such grid.  With Mq = B (H + 1) (W + 1)
# stream positions, tiles = ceil(Mq / BM) * ceil(Nout / 128), and shift_plan_bm's choice between 192- and 256-row tiles:
#   DENSE_FWD     32 -> 2048 at 26 x 26, B = 6: Mq = 4374: 18 x 16 = 288 tiles of 256 rows, 23 x 16 = 368 of 192 -> 2 rounds of 192 beat 2 of 256: BM = 192
#   DENSE_FWD256  32 -> 3584 at 26 x 26, B = 6: 18 x 28 = 504 tiles of 256 (2 rounds), 23 x 28 = 644 of 192 (3 rounds): BM = 256, as the 52^2 layers at batch 32
#   DENSE_DGRAD   the layer 2048 -> 32 at 8 x 31, B = 15 (dx = 2048 channels): Mq = 15 * 9 * 32 = 4320: 17 x 16 = 272 tiles of 256, 23 x 16 = 368 of 192: the plain
#                 form runs 192-row tiles (what the 52^2 data gradients of the benchmark run), the fused form always 256-row tiles (BM = 256, NPA = 3; no
#                 plan launches that one 128 wide -- the fused dense grids of the plans are 64 wide, PROD_CASES -- it is here because the ring depth of
#                 the fused 128-wide tile is decided by the same line of launch_shift_f)
# B, Cin, H, W, Cout of a 3x3 stride-1 layer
DENSE_FWD = (6, 32, 26, 26, 2048)                 # forward; also as a channel slice of a wider buffer
DENSE_FWD256 = (6, 32, 26, 26, 3584)              # forward
DENSE_DGRAD = (15, 2048, 8, 31, 32)               # data gradient, plain (+ addsrc) and with the fused sums
DENSE_CASES = [DENSE_FWD, DENSE_FWD256, DENSE_DGRAD]
# These references are above MACS_CAP: a dense grid of 128-wide tiles costs at least 257 x 256 x 128 x 9 x 32 = 2.4e9 multiply-adds, padding included.  The
# largest is DENSE_FWD256: 6 * 26 * 26 * 9 * 32 * 3584 = 4.19e9 (DENSE_FWD 2.39e9, DENSE_DGRAD 2.19e9, the dense PROD_CASES 2.1e9 .. 3.2e9); the cap is that
# case.  Measured on 16 CPU threads (torch float64): DENSE_FWD256 1.2 s, reference and conditions together; each is computed once per module.
DENSE_MACS_CAP = 4.2e9


def prod_macs_ok(pc):
    return macs(pc["geom"]) <= (DENSE_MACS_CAP if pc.get("dense") else MACS_CAP)


@functools.lru_cache(maxsize=4)
def dense_refs(case):
    """gen_case for a DENSE_CASES entry with the references its tests use, computed once per module and shared (callers do not modify it)"""
    t = c3(case)
    assert case in DENSE_CASES and macs(t) <= DENSE_MACS_CAP, case
    B, Ci, H, W, Co = case
    c = gen_case(seed_of(t), B, Ci, H, W, Co, 3)
    if case == DENSE_DGRAD:
        return dict(c, _dxa=ref_dgrad(c, True), _dx=ref_dgrad(c, False))
    return dict(c, _y=ref_fwd(c))


# ---- the forms the production plans launch that no table above reaches (tests/test_gpu_conv_census.py printed them; docs/conv_census.md).  Each entry: the
# smallest geometry found that reaches the instantiation, what runs on it (f forward, d data gradient, b data gradient with the fused sums), the variant code
# (0 wherever the default is what production runs; 2001 -- 256-row tiles from 1024 positions -- for the tall narrow tiles, whose default threshold of 256 Ki
# positions no integer reference affords) and the instantiation it is there for.  All within MACS_CAP.
def _s(**kw):
    return ("mdcv_conv3x3_shift_kernel", dict(dict(WN=2, EPI=False, LOOP=0), **kw))


def _g(**kw):
    return ("conv_glds_kernel", dict(dict(FUSE=False, EPI=False, ALLCLS=False, UT=True), **kw))


PROD_CASES = [
    # 1x1 64 -> 32 (the 208^2 layers): forward on 256 x 32 tiles, data gradient (64 channels) on 256 x 64 tiles with the 3-stage ring, uniform-tap addresses;
    # y and dx as channel slices of wider buffers
    dict(id="tall-1x1-64to32", geom=(2, 64, 24, 24, 32, 1, 1, 0, 1, False), run="fd", code=2001, slices=True,
         need=[_g(MODE=0, BM=256, BN=32, WM=4, WN=1, STAGES=2), _g(MODE=1, BM=256, BN=64, WM=4, WN=2, STAGES=3)]),
    # 1x1 32 -> 64 (KeypointNet's 80^2 layers at batch 256): the data gradient (32 channels) on 256 x 32 tiles
    dict(id="tall-1x1-32to64", geom=(2, 32, 24, 24, 64, 1, 1, 0, 1, False), run="d", code=2001, need=[_g(MODE=1, BM=256, BN=32, WM=4, WN=1, STAGES=2)]),
    # 3x3 / stride 2 32 -> 64 (416 -> 208): forward on 256 x 64 tiles
    dict(id="tall-s2-32to64", geom=(2, 32, 48, 48, 64, 3, 2, 1, 1, False), run="f", code=2001, need=[_g(MODE=0, BM=256, BN=64, WM=4, WN=2, STAGES=3)]),
    # 3x3 32 -> 64 on rows wider than the 1-D stream takes (the 208^2 layers): 2-D tiles, 52 x 5 = 260 of them: dense grid, 64- / 32-wide tiles
    dict(id="2d-dense-32to64", geom=(1, 32, 416, 121, 64, 3, 1, 1, 1, False), run="fd", code=0,
         need=[_s(MODE=0, BM=256, NPA=3, BRING=3, FUSE=False, BN=64), _s(MODE=1, BM=256, NPA=3, BRING=3, FUSE=False, BN=32)]),
    # fused data gradients on grids of 129..256 tiles of 256 rows (the 26^2 and 13^2 layers at batch 32): 4-slot ring.  Mq = 12 * 53 * 53 = 33708: 132 tiles
    dict(id="fused-ring4-128", geom=(12, 128, 52, 52, 32, 3, 1, 1, 1, False), run="b", code=0, need=[_s(MODE=1, BM=256, NPA=3, BRING=4, FUSE=True, BN=128)]),
    dict(id="fused-ring4-64", geom=(12, 64, 52, 52, 32, 3, 1, 1, 1, False), run="b", code=0, need=[_s(MODE=1, BM=256, NPA=3, BRING=4, FUSE=True, BN=64)]),
    # fused data gradient of 64 channels on rows of 81..104 pixels (the 104^2 layers): four DMAs, dense grid: Mq = 6 * 105 * 105 = 66150: 259 tiles
    dict(id="fused-w104-64", geom=(6, 64, 104, 104, 32, 3, 1, 1, 1, False), run="b", code=0, need=[_s(MODE=1, BM=256, NPA=4, BRING=3, FUSE=True, BN=64)]),
    # the reference cfgs' own size (800^2, B = 4): forward on 192-row tiles of a one-round grid (4-slot ring, ping-pong loop) with three DMAs per chunk
    # (rows of >= 31 pixels): Mq = 4 * 32 * 33 = 4224 -> 17 x 8 = 136 tiles of 256, 22 x 8 = 176 of 192 (one round of 192 rows beats one of 256)
    dict(id="fwd-192-ring4-w32", geom=(4, 32, 31, 32, 1024, 3, 1, 1, 1, False), run="f", code=0,
         need=[_s(MODE=0, BM=192, NPA=3, BRING=4, FUSE=False, BN=128, LOOP=1)]),
    # ... and the fused data gradient of 64 channels on a dense grid (its 200^2 ... 50^2 layers): Mq = 24 * 53 * 53 = 67416 -> 264 tiles
    dict(id="fused-dense-64", geom=(24, 64, 52, 52, 32, 3, 1, 1, 1, False), run="b", code=0, need=[_s(MODE=1, BM=256, NPA=3, BRING=3, FUSE=True, BN=64)]),
    # stride-2 data gradients on the shift kernel with the fused sums, dense grid (416 <- 208, 208 <- 104): 37 x 7 = 259 tiles of 8 x 31 positions of dy
    dict(id="s2d-dense-32", geom=(1, 32, 592, 416, 32, 3, 2, 1, 1, False), run="b", code=0, need=[_s(MODE=3, BM=256, NPA=3, BRING=3, FUSE=True, BN=32)]),
    dict(id="s2d-dense-64", geom=(1, 64, 592, 416, 32, 3, 2, 1, 1, False), run="b", code=0, need=[_s(MODE=3, BM=256, NPA=3, BRING=3, FUSE=True, BN=64)]),
    # ---- the tiny cfg at 416^2, batch 32
    # forward on 192-row tiles of a one-round grid at 13 x 13 (two DMAs): Mq = 21 * 196 = 4116 -> 17 x 8 = 136 tiles of 256, 22 x 8 = 176 of 192
    dict(id="fwd-192-ring4-w13", geom=(21, 32, 13, 13, 1024, 3, 1, 1, 1, False), run="f", code=0,
         need=[_s(MODE=0, BM=192, NPA=2, BRING=4, FUSE=False, BN=128, LOOP=1)]),
    # data gradient of 64 channels, one round of 192-row tiles at 26 x 26: Mq = 50 * 729 = 36450 -> 143 tiles of 256, 190 of 192
    dict(id="dgrad-192-ring4-64", geom=(50, 64, 26, 26, 32, 3, 1, 1, 1, False), run="d", code=0, need=[_s(MODE=1, BM=192, NPA=2, BRING=4, FUSE=False, BN=64)]),
    # data gradient of 64 / 32 channels on a dense grid of 192-row tiles, rows of 31 pixels (three DMAs): Mq = 228 * 9 * 32 = 65664 -> 257 tiles of 256 (two
    # rounds), 342 of 192 (two rounds of fewer rows); the same layers forward (KeypointNet inference, 80^2 at batch 64)
    dict(id="dense-192-w31-64", geom=(228, 32, 8, 31, 64, 3, 1, 1, 1, False), run="f", code=0, need=[_s(MODE=0, BM=192, NPA=3, BRING=3, FUSE=False, BN=64)]),
    dict(id="dgrad-dense-192-w31-64", geom=(228, 64, 8, 31, 32, 3, 1, 1, 1, False), run="d", code=0, need=[_s(MODE=1, BM=192, NPA=3, BRING=3, FUSE=False, BN=64)]),
    dict(id="dense-192-w31-32", geom=(228, 32, 8, 31, 32, 3, 1, 1, 1, False), run="f", code=0, need=[_s(MODE=0, BM=192, NPA=3, BRING=3, FUSE=False, BN=32)]),
    # ---- KeypointNet at 80 x 80: rows of 63..104 pixels (four DMAs) on dense grids of 256-row tiles, 64 / 32 channels: Mq = 154 * 9 * 71 = 98406 -> 385 tiles
    # of 256 (two rounds), 513 of 192 (three rounds)
    dict(id="dense-256-w70-64", geom=(154, 32, 8, 70, 64, 3, 1, 1, 1, False), run="f", code=0, need=[_s(MODE=0, BM=256, NPA=4, BRING=3, FUSE=False, BN=64)]),
    dict(id="dgrad-dense-256-w70-64", geom=(154, 64, 8, 70, 32, 3, 1, 1, 1, False), run="d", code=0, need=[_s(MODE=1, BM=256, NPA=4, BRING=3, FUSE=False, BN=64)]),
    dict(id="dense-256-w70-32", geom=(154, 32, 8, 70, 32, 3, 1, 1, 1, False), run="fd", code=0,
         need=[_s(MODE=0, BM=256, NPA=4, BRING=3, FUSE=False, BN=32), _s(MODE=1, BM=256, NPA=4, BRING=3, FUSE=False, BN=32)]),
    # dilation-2 data gradients of 32 / 64 channels on rows of 80 pixels: the halo (4 * 83 rows) leaves room for 192-row tiles only, five DMAs; more than 256
    # tiles: Mq = 61 * 10 * 82 = 50020 -> 261 tiles
    dict(id="dil2-dense-w80-32", geom=(61, 32, 8, 80, 64, 3, 1, 2, 2, False), run="d", code=0, need=[_s(MODE=1, BM=192, NPA=5, BRING=3, FUSE=False, BN=32)]),
    dict(id="dil2-dense-w80-64", geom=(61, 64, 8, 80, 64, 3, 1, 2, 2, False), run="d", code=0, need=[_s(MODE=1, BM=192, NPA=5, BRING=3, FUSE=False, BN=64)]),
    # ---- above MACS_CAP, under DENSE_MACS_CAP (dense=True): 128-wide tiles on dense grids cost 256 x 128 x 9 x 32 multiply-adds a tile at the least
    # forward on a dense grid of 192-row tiles, rows of 31 pixels (KeypointNet inference): Mq = 15 * 288 = 4320 -> 17 x 16 = 272 of 256, 23 x 16 = 368 of 192
    dict(id="dense-192-w31-128", geom=(15, 32, 8, 31, 2048, 3, 1, 1, 1, False), run="f", code=0, dense=True,
         need=[_s(MODE=0, BM=192, NPA=3, BRING=3, FUSE=False, BN=128)]),
    # data gradient of 2048 channels on a dense grid of 192-row tiles at 13 x 13 (the tiny cfg): Mq = 21 * 196 = 4116 -> 17 x 16 = 272 of 256, 22 x 16 = 352 of 192
    dict(id="dgrad-dense-192-w13-128", geom=(21, 2048, 13, 13, 32, 3, 1, 1, 1, False), run="d", code=0, dense=True,
         need=[_s(MODE=1, BM=192, NPA=2, BRING=3, FUSE=False, BN=128)]),
    # rows of 70 pixels on a dense grid of 256-row, 128-wide tiles (KeypointNet's 64 -> 128 / 128 -> 128 layers): Mq = 22 * 639 = 14058 -> 55 x 7 = 385 tiles of
    # 256 (two rounds), 74 x 7 = 518 of 192 (three)
    dict(id="dense-256-w70-128", geom=(22, 32, 8, 70, 896, 3, 1, 1, 1, False), run="f", code=0, dense=True,
         need=[_s(MODE=0, BM=256, NPA=4, BRING=3, FUSE=False, BN=128)]),
    dict(id="dgrad-dense-256-w70-128", geom=(22, 896, 8, 70, 32, 3, 1, 1, 1, False), run="d", code=0, dense=True,
         need=[_s(MODE=1, BM=256, NPA=4, BRING=3, FUSE=False, BN=128)]),
]
PW_PROD_CASES = [(600, 128, 64, 8, False, 1)]              # 1x1 128 -> 64 WITHOUT a residual (PW_CASES has it with one); rows 8 channels apart
# one-launch 1x1 backward with the fused sums: 128 output channels with addsrc (3 stages; rows 8 channels apart), 512 without (2 stages)
PWB_PROD_CASES = [(1500, 128, 128, 256, 8, True), (2000, 512, 512, 1024, 0, False)]
# KeypointNet's 16 -> 16 and 32 -> 32 layers at 80 x 80: the untiled ring kernels (WGRAD_STREAM_CASES has 16 -> 16 only at a size the kernel does not take)
WGRAD_STREAM_PROD = [(2, 16, 16, 80, 80, 1), (2, 32, 32, 80, 80, 1)]
# The inference epilogue (mdcv_conv2d_affine_act; tuples as AFFINE_CASES, then the variant code) on the tiles the 608^2 detector and KeypointNet inference run
AFFINE_PROD_CASES = [
    ((3, 256, 80, 80, 256, 1, 1, True, 1), 0),       # 1x1 on 150 x 2 = 300 tiles of 128 x 128, 8 K steps: 128 x 128 tiles, 3-stage ring
    ((8, 32, 128, 128, 128, 1, 1, False, 1), 0),     # 1024 tiles of 128 x 128: 256 x 128 tiles
    ((2, 8, 24, 24, 16, 7, 1, False, 2), 2001),      # tall narrow tiles: 256 x 16 (7x7 stem; generic addresses)
    ((2, 16, 40, 40, 32, 3, 1, False, 2), 2001),     # 256 x 32, generic addresses
    ((2, 64, 24, 24, 32, 1, 1, False, 1), 2001),     # 256 x 32, uniform-tap addresses
    ((2, 32, 48, 48, 64, 3, 2, False, 1), 2001),     # 256 x 64 (stride 2)
    ((65, 32, 8, 105, 64, 3, 1, False, 1), 0),       # shift kernel, 2-D tiles, 65 x 4 = 260 of them, 64 wide
    ((15, 32, 8, 31, 2048, 3, 1, True, 1), 0),       # shift kernel, dense grid of 192-row tiles (2.2e9 multiply-adds: under DENSE_MACS_CAP)
    ((43, 32, 8, 81, 256, 3, 1, False, 1), 0),       # shift kernel, 2-D tiles, 43 x 3 x 2 = 258 tiles of 256 x 128 (2.1e9: under DENSE_MACS_CAP)
]
_AFFINE_NEED = [_g(MODE=0, BM=128, BN=128, WM=2, WN=2, STAGES=3, EPI=True), _g(MODE=0, BM=256, BN=128, WM=4, WN=2, STAGES=3, EPI=True),
                _g(MODE=0, BM=256, BN=16, WM=4, WN=1, STAGES=2, UT=False, EPI=True), _g(MODE=0, BM=256, BN=32, WM=4, WN=1, STAGES=2, UT=False, EPI=True),
                _g(MODE=0, BM=256, BN=32, WM=4, WN=1, STAGES=2, EPI=True), _g(MODE=0, BM=256, BN=64, WM=4, WN=2, STAGES=3, EPI=True),
                _s(MODE=0, BM=256, NPA=3, BRING=3, FUSE=False, BN=64, EPI=True), _s(MODE=0, BM=192, NPA=3, BRING=3, FUSE=False, BN=128, EPI=True),
                _s(MODE=0, BM=256, NPA=3, BRING=3, FUSE=False, BN=128, EPI=True)]


@functools.lru_cache(maxsize=2)
def _prod_refs(geom, run):
    B, Ci, H, W, Co, k, s, p, d, bias = geom
    c = gen_case(seed_of(geom), B, Ci, H, W, Co, k, s, p, d, bias)
    if "f" in run:
        c["_y"] = ref_fwd(c)
    if "d" in run or "b" in run:
        c["_dxa"] = ref_dgrad(c, True)
    return c


def prod_refs(pc):
    """gen_case for a PROD_CASES entry with the references its runs use, under the entry's cap; shared, callers do not modify it"""
    assert prod_macs_ok(pc), pc["id"]
    return _prod_refs(pc["geom"], pc["run"])


# ---- purpose patterns: what each case of tests/test_gpu_conv_exact.py is THERE for, as a condition on the template instantiations it launches
# (helpers/kernel_census.py).  Written from the reason the case exists (the table in that file's docstring, csrc/tune.h, the dispatch code), not from a
# run: a pattern that does not hold means the case does not test what its comment says.  A pattern is (kernel name(s), {template parameter: value});
# purpose() returns (need, forbid): every `need` pattern must match at least one launched instantiation, no `forbid` pattern may match any.
SHIFT = "mdcv_conv3x3_shift_kernel"
GLDS = "conv_glds_kernel"
IGEMM = "conv_igemm_kernel"
CONV = (IGEMM, GLDS, SHIFT)
WG_GENERIC = ("conv_wgrad_kernel", "conv_wgrad_dma_kernel", "conv_wgrad_dma_narrow_kernel")
WG_STREAM, WG_SHIFT, WG_S2, WG_STEM = "wgrad3x3_stream_kernel", "wgrad3x3_shift_kernel", "wgrad3x3_s2_stream_kernel", "wgrad7x7_stream_kernel"
WG_ANY = WG_GENERIC + (WG_STREAM, WG_SHIFT, WG_S2, WG_STEM)
FWD, DGRAD = (CONV, {"MODE": 0}), (CONV, {"MODE": 1})
# forced tile configurations of wide layers (csrc/conv_gemm.h dispatch_conv): code -> (BM, BN, KT) register-staged / (BM, BN, STAGES) LDS-DMA
_IG_BF = {0: (128, 128, 1), 1: (128, 128, 2), 2: (256, 128, 1), 3: (256, 128, 2), 4: (128, 64, 2), 5: (128, 64, 1)}
_IG_F32 = {0: (128, 128, 1), 1: (128, 128, 1), 2: (128, 128, 1), 3: (128, 128, 1), 4: (128, 64, 1), 5: (128, 64, 1)}
_GL_BF = {6: (128, 128, 2), 7: (128, 64, 2), 8: (256, 128, 2), 9: (128, 128, 3), 10: (128, 64, 3), 11: (256, 128, 3)}
_GL_F32 = {**_GL_BF, 8: (128, 128, 2), 11: (128, 128, 3)}         # the 256-row tiles exist in bf16 only


def shift_npa(bm, W, dil=1):
    """DMAs per wave of one activation chunk of the 1-D stream (csrc/conv_shift.hip launch_shift_bm): BM + 2 dil (W + 2) rows in KiB-chunks of 16, eight per DMA"""
    return ((bm + 2 * dil * (W + 2) + 15) // 16 + 7) // 8


# csrc/wgrad_stream.hip stream_cfg: (Cin, Cout) -> NCI, NCO, A, PG, BP, D, TGRP of the untiled instantiations
_STREAM_CFG = {(16, 16): (1, 1, 1, 8, 256, 2, 9), (16, 32): (1, 2, 2, 8, 256, 2, 9), (32, 32): (2, 2, 2, 4, 128, 2, 9), (32, 64): (2, 4, 4, 4, 128, 2, 3),
               (64, 64): (4, 4, 4, 2, 64, 2, 3)}


def stream_eligible(t):
    """mdcv_wgrad_stream_eligible for a (B, Cin, Cout, H, W, dil) of the stream tables: a step of BP positions wraps one image at most"""
    B, Ci, Co, H, W, dil = t
    bp = 64 if _tiled(Ci, Co) else _STREAM_CFG[(Ci, Co)][4]
    return H >= 4 and W >= 4 and bp // (W + dil) + 1 < H + dil


def _tiled(ci, co):
    return ci % 64 == 0 and co % 128 == 0           # csrc/wgrad_stream.hip stream_cfg: the channel-tiled instantiation


def purpose(test, p):
    """(need, forbid) for the test function `test` with the parametrisation `p` (dict: argument name -> value)"""
    need, forbid = [], []
    code, case, dt = p.get("code"), p.get("case"), p.get("dt")
    if dt is not None:                                # dt: 0 = fp32, 1 = bf16 (test_gpu_kernels.F32 / BF16): T = float there and nowhere else
        (need if dt == 0 else forbid).append(((IGEMM, GLDS, "conv_wgrad_kernel"), {"T": "float"}))
    if test in ("test_a_conv_cases", "test_a_wrong_kernel_would_fail"):
        need += [FWD, (CONV, {"MODE": 2 if case[6] == 2 else 1})]
        if test == "test_a_conv_cases":
            need.append((WG_ANY, {}))
    elif test == "test_a_tile_variants":
        v, bf = code % 100, dt == 1
        for mode in (0, 1):
            if v < 6:
                bm, bn, kt = (_IG_BF if bf else _IG_F32)[v]
                need.append((IGEMM, {"MODE": mode, "BM": bm, "BN": bn, "KT": kt}))
            else:
                bm, bn, stg = (_GL_BF if bf else _GL_F32)[v]
                need.append((GLDS, {"MODE": mode, "BM": bm, "BN": bn, "STAGES": stg, "UT": code < 100}))
        if code >= 100:
            forbid.append((GLDS, {"UT": True}))       # 100 + v: the generic address path
    elif test == "test_a_narrow_output_codes":
        if code in (30, 31) and case == NARROW_CASE:
            need += [(GLDS, {"MODE": m, "BM": 128, "BN": 64, "STAGES": 2 if code == 30 else 3}) for m in (0, 1)]
            if code == 30:
                forbid.append((GLDS, {"STAGES": 3}))
        elif code == 2001:
            bn = {NARROW_CASES[0]: (64, 64), NARROW_CASES[1]: (32, 16), NARROW_CASES[2]: (16, 16)}[case]
            need += [(GLDS, {"MODE": m, "BM": 256, "BN": bn[m]}) for m in (0, 1)]
        elif code == 2000:
            need += [(GLDS, {"MODE": 0}), (GLDS, {"MODE": 1})]
            forbid.append((GLDS, {"BM": 256}))
        else:
            need += [FWD, DGRAD]
    elif test == "test_a_deep_small_codes":
        need.append((GLDS, {"MODE": 0, "BM": 128, "BN": 64, "STAGES": 3 if code == 68 else 2}))
        need.append((CONV, {"MODE": 2 if case[6] == 2 else 1}))
    elif test == "test_a_fused_1x1_tiles":
        need.append((GLDS, {"MODE": 1, "FUSE": True, "BM": 128, "BN": 64, "STAGES": 3 if code == 93 else 2}))
    elif test == "test_b_shift_default":
        need.append((SHIFT, {"MODE": 0}))
        if case[1] in (32, 64) or case[1] % 128 == 0:  # (a data gradient of 96 channels is not the shift kernel's: csrc/conv_shift.hip mdcv_shift_launch_dgrad)
            need.append((SHIFT, {"MODE": 1}))
        if case[4] == 64:                              # the narrow column
            need.append((SHIFT, {"MODE": 0, "BN": 64}))
    elif test == "test_b_shift_codes":
        need.append((SHIFT, {"MODE": 0}))
        if code in (-8, -9):                           # tile plans: 256-row tiles only / 128-row only
            bm = 256 if code == -8 else 128
            need.append((SHIFT, {"MODE": 0, "BM": bm}))
            forbid += [(SHIFT, {"BM": b}) for b in (128, 192, 256, 384) if b != bm]
        elif code in (-30, -31):                       # K loop of the forward launches: lockstep / ping-pong
            need.append((SHIFT, {"MODE": 0, "LOOP": 0 if code == -30 else 1}))
            forbid.append((SHIFT, {"MODE": 0, "LOOP": 1 if code == -30 else 0}))
        elif code == -201:
            need.append((SHIFT, {"MODE": 0, "BM": 384, "LOOP": 1}))
        elif code in (-3, -4):                         # ring depth
            need.append((SHIFT, {"MODE": 0, "BRING": -code}))
            forbid.append((SHIFT, {"WN": 2, "EPI": False, "BRING": 7 + code}))
        elif code in (-17, -18, -19) and case[1] == 64:     # the data gradient of a 64-channel input: one narrow tile column on / off
            (forbid if code == -18 else need).append((SHIFT, {"MODE": 1, "BN": 64}))
    elif test == "test_b_shift_rows_of_63_to_80_pixels":
        need += [(SHIFT, {"MODE": 0}), (SHIFT, {"MODE": 1})]
        if code == -14:                                # the 1-D stream's four-DMA chunk
            need.append((SHIFT, {"MODE": 0, "BM": 256, "NPA": 4}))
        else:                                          # 2-D tiles of 8 x 30 outputs: 256 positions + 2 * 33 halo rows -> three DMAs
            need.append((SHIFT, {"MODE": 0, "BM": 256, "NPA": 3}))
            forbid.append((SHIFT, {"MODE": 0, "NPA": 4}))
    elif test == "test_b_shift_wide_dgrad_tiles":
        if code == -64:
            need.append((SHIFT, {"MODE": 1, "BN": 64}))
            if case == SHIFT_WIDE_DGRAD[1]:
                need.append((SHIFT, {"MODE": 1, "BM": 256, "BN": 64}))
        else:
            need.append((SHIFT, {"MODE": 1, "BN": 128}))
            forbid.append((SHIFT, {"BN": 64}))
    elif test == "test_b_shift_2d_tiles":
        need += [(SHIFT, {"MODE": 0, "BM": 256}), (SHIFT, {"MODE": 1, "BM": 256})]
        forbid += [(SHIFT, {"BM": b}) for b in (128, 192, 384)] + [(GLDS, {}), (IGEMM, {})]
    elif test == "test_b_shift_dilation2":
        if code == -20:
            need += [(SHIFT, {"MODE": 0}), (SHIFT, {"MODE": 1})]
        else:
            need += [((IGEMM, GLDS), {"MODE": 0}), ((IGEMM, GLDS), {"MODE": 1})]
            forbid.append((SHIFT, {}))
    elif test == "test_c_stride2_dgrad_forms":
        one = case == S2_CASES[1] and code in (17, 15, 4001)
        need.append((GLDS, {"MODE": 2}))
        if one:
            need += [(GLDS, {"MODE": 2, "ALLCLS": True, "FUSE": False}), (GLDS, {"MODE": 2, "ALLCLS": True, "FUSE": True})]
        else:
            need.append((GLDS, {"MODE": 2, "FUSE": True}))
            forbid.append((GLDS, {"ALLCLS": True}))
    elif test == "test_c_shift_stride2_dgrad":
        if code == -60:
            need.append((SHIFT, {"MODE": 3, "BN": case[4], "FUSE": p["form"] == "addsrc+bnsums"}))
            forbid += [(GLDS, {}), (IGEMM, {})]
        else:
            need.append((GLDS, {"MODE": 2, "FUSE": p["form"] == "addsrc+bnsums"}))
            forbid.append((SHIFT, {}))
    elif test == "test_d_conv_xstats_digits":
        need.append(FWD)
        if code == -201:
            need.append((SHIFT, {"MODE": 0, "BM": 384}))
    elif test == "test_e_wgrad_family_codes":
        need.append((WG_ANY, {}))
        if code == 9:                                  # every layer on the generic kernels
            need.append((WG_GENERIC, {}))
            forbid.append(((WG_STREAM, WG_SHIFT, WG_S2, WG_STEM), {}))
        elif code == 10:                               # all but the kw-shared kernel's
            forbid.append(((WG_STREAM, WG_S2, WG_STEM), {}))
        elif code == 4:                                # the generic address path: never the same-size fast path of the wide DMA kernel
            forbid.append(("conv_wgrad_dma_kernel", {"SAME": True}))
        elif code == 5:                                # the wide tile everywhere: never the narrow kernel
            forbid.append(("conv_wgrad_dma_narrow_kernel", {}))
        else:                                          # 8 / 11 widen the kw-shared kernel's share -- of layers it is eligible for (3x3, stride 1, channels in
            kwshared = case[5] == 3 and case[6] == 1 and case[8] == 1 and case[1] % 128 == 0 and case[4] % 128 == 0     # 128s) and the ring kernel does not
            if kwshared:                               # take first (csrc/conv_igemm.hip choose_wgrad_family): here it takes every such layer
                need.append((WG_STREAM, {}))
            else:
                forbid.append((WG_SHIFT, {}))
    elif test == "test_e_wgrad_shift":
        if code == 9:
            need.append((WG_GENERIC, {}))
            forbid.append(((WG_STREAM, WG_SHIFT), {}))
        elif code == 8:                                # the kw-shared kernel where the ring kernel does not come first (WGRAD_KWSHARED_CASES)
            need.append((WG_SHIFT, {}) if case in WGRAD_KWSHARED_CASES else (WG_STREAM, {}))
        else:
            need.append((WG_ANY, {}))
    elif test in ("test_e_wgrad_stream", "test_e_wgrad_slab_free", "test_i_wgrad_stream_production"):
        if stream_eligible(case):
            need.append((WG_STREAM, {}))
        else:                                          # images of so few rows that one step wraps more than one image: the generic kernels
            need.append((WG_GENERIC, {}))
            forbid.append((WG_STREAM, {}))
        if test == "test_i_wgrad_stream_production":
            B, Ci, Co = case[:3]
            need.append((WG_STREAM, dict(zip(("NCI", "NCO", "A", "PG", "BP", "D", "TGRP"), _STREAM_CFG[(Ci, Co)]), TILED=False, NW=8, TBL=True, DIRECT=False)))
        elif _tiled(case[1], case[2]):
            need.append((WG_STREAM, {"TILED": True}))
            if code == 30003:
                need.append((WG_STREAM, {"TILED": True, "NW": 4}))
                forbid.append((WG_STREAM, {"NW": 8}))
            elif code == 30005:
                need.append((WG_STREAM, {"TILED": True, "NW": 8}))
                forbid.append((WG_STREAM, {"NW": 4}))
            elif code == 34021:
                need.append((WG_STREAM, {"TBL": True}))
            elif code == 34020:
                forbid.append((WG_STREAM, {"TBL": True}))
            elif code == 34051 and test == "test_e_wgrad_slab_free":
                need.append((WG_STREAM, {"DIRECT": True, "TBL": True}))
            if code in (34050, 34020, 30005):
                forbid.append((WG_STREAM, {"DIRECT": True}))
    elif test == "test_e_wgrad_stride2":
        if code == 34060:                              # parity-plane ring kernel off
            need.append((WG_GENERIC, {}))
            forbid.append((WG_S2, {}))
        else:                                          # on (34061: the default depth 2) / prefetch depth 34070 + d (csrc/tune.h)
            d = 2 if code == 34061 else code - 34070
            need.append((WG_S2, {"D": d}))
            forbid += [(WG_S2, {"D": o}) for o in (1, 2, 3) if o != d]
    elif test == "test_e_wgrad_stem_7x7":
        need.append((WG_STEM, {}) if code == 0 else (WG_GENERIC, {}))
        if code == 9:
            forbid.append((WG_STEM, {}))
    elif test == "test_e_wgrad_bnapply":
        need.append(("conv_wgrad_dma_narrow_kernel", {"BNA": True}))
    elif test == "test_f_pw_forward":
        M, K, N, xs, with_r, a = case
        need.append(("pw_block_kernel", {"BMP": 64 if K <= 256 else (32 if K <= 512 else 16), "HASR": bool(with_r), "WRES": K * N * 2 <= 64 * 1024}))   # resident weights: K * N * 2 <= 64 KiB (csrc/pw_block.hip)
    elif test == "test_f_pw_backward":
        need += [("pw_bwd_kernel", {"ADD": bool(case[5]), "FUSE": bool(p["fused"])}), ("wgrad_reduce*_kernel", {})]
    elif test == "test_g_first_conv":
        need += [("first_conv_kernel", {"MODE": 0}), ("first_conv_kernel", {"MODE": 1})]
    elif test == "test_g_affine_act":
        need.append(((GLDS, SHIFT), {"MODE": 0, "EPI": True}))
        forbid.append(((GLDS, SHIFT), {"EPI": False}))
    elif test == "test_h_dgrad_bnsums":
        need.append(((GLDS, SHIFT), {"FUSE": True}))
        forbid.append(((GLDS, SHIFT), {"FUSE": False}))
    elif test == "test_i_dense_forward":                # the production forward of the dense grids, under the DEFAULT code
        bm = 192 if case == DENSE_FWD else 256
        need.append((SHIFT, {"MODE": 0, "BM": bm, "NPA": shift_npa(bm, case[3]), "BRING": 3, "FUSE": False, "WN": 2, "EPI": False, "BN": 128, "LOOP": 0}))
        forbid += [(SHIFT, {"BRING": 4}), (SHIFT, {"LOOP": 1})]
    elif test == "test_i_dense_dgrad":
        fused = p["form"] == "bnsums"
        need.append((SHIFT, {"MODE": 1, "BM": 256 if fused else 192, "NPA": 3, "BRING": 3, "FUSE": fused, "WN": 2, "EPI": False, "BN": 128, "LOOP": 0}))
        forbid.append((SHIFT, {"BRING": 4}))
    elif test == "test_i_dense_wrong_kernel_would_fail":
        need.append((SHIFT, {"MODE": 0, "BRING": 3, "LOOP": 0}))
    elif test == "test_i_production_forms":
        need += p["pc"]["need"]
        forbid += p["pc"].get("forbid", [])
    elif test == "test_i_affine_production":
        need.append(_AFFINE_NEED[[c for c, _ in AFFINE_PROD_CASES].index(case)])
        forbid.append(((GLDS, SHIFT), {"EPI": False}))
    elif test == "test_i_pw_forward_production":
        M, K, N, xs, with_r, a = case
        need.append(("pw_block_kernel", {"BMP": 64, "FNW": 2, "NV": 4, "HASR": False, "WRES": True}))
    elif test == "test_i_pw_backward_production":
        need.append(("pw_bwd_kernel", {"CO4": case[1] // 64, "S": 2 if case[1] >= 512 else 3, "ADD": bool(case[5]), "FUSE": True}))
    else:
        raise KeyError(f"no purpose pattern for {test}")
    return need, forbid
