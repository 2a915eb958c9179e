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
SHIFT_W70 = (1, 32, 9, 70, 128)       # rows of 63..80 pixels: the four-DMA chunk of the 1-D stream under -14 (shift_wmax 80), 2-D pixel tiles under -15 (62)


def c3(t, bias=False, dil=1):
    """(B, Cin, H, W, Cout) of a 3x3 stride-1 layer -> the 10-tuple of CONV_CASES"""
    B, Ci, H, W, Co = t
    return (B, Ci, H, W, Co, 3, 1, dil, dil, bias)


SHIFT_CASES = [(3, 64, 26, 20, 128), (5, 96, 8, 9, 128), (1, 256, 13, 13, 512), (4, 64, 26, 26, 256), (9, 32, 30, 17, 128), (33, 64, 13, 13, 64),
               (1, 128, 104, 104, 128)]
SHIFT_CODES = [-8, -9, -12, -30, -31, -201, -3, -4, -17, -18, -19, -15, -14]
SHIFT_WIDE_DGRAD = [(4, 512, 13, 13, 1024), (2, 512, 13, 11, 1024)]          # the 256 x 64 data-gradient tiles (-64 / -63): Cin -> Cout of the LAYER
SHIFT_2D = [(2, 32, 97, 131, 128), (1, 128, 9, 161, 128), (2, 32, 41, 300, 32)]
SHIFT_DIL2 = [(3, 64, 26, 26, 64), (4, 32, 30, 17, 32)]
# B, Cin, H, W, Cout of a 3x3 / stride-2 / pad-1 layer.  Odd sizes: four parity-class launches under every code.  Even sizes with MORE than 64 input
# channels (dx = 128 channels: 64 and 32 go to the shift kernel's stride-2 form, S2D_CASES): one launch for the four classes (ALLCLS), csrc/conv_igemm.hip
S2_CASES = [(2, 64, 17, 19, 128), (2, 128, 16, 20, 128)]
S2D_CASES = [(3, 32, 17, 45, 32), (2, 64, 8, 31, 64), (1, 32, 9, 63, 32), (1, 128, 52, 52, 64)]   # B, Cdy, Hdy, Wdy, Cdx (test_gpu_kernels.S2D_CASES)
FUSE_CASES = [(2, 64, 26, 20, 128, 3, 1, 1), (5, 128, 13, 13, 256, 3, 1, 1), (2, 256, 14, 14, 128, 1, 1, 0), (2, 64, 17, 19, 128, 3, 2, 1),
              (3, 32, 20, 20, 48, 3, 1, 1), (2, 16, 24, 24, 32, 3, 1, 2), (2, 64, 15, 17, 72, 3, 1, 1)]
WGRAD_SHIFT_CASES = [(2, 128, 13, 13, 128), (3, 128, 26, 20, 256), (1, 256, 52, 52, 128), (5, 128, 9, 8, 128)]
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
