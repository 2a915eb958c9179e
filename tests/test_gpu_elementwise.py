"""-m gpu: the BatchNorm / per-channel kernels of csrc/bn_fwd.hip, bn_bwd.hip and col_reduce.hip and the optimizers of csrc/optim.hip at production
sizes, through the C ABI, against float64 references computed on the CPU from the values AS STORED on the device.

Groups (the numbers are those of the sections below):
 1. exact coverage: integer-valued data whose every product and partial sum is exactly representable, compared with ``==``;
    sentinel-filled buffers around every strided output.
 3. accuracy: random data, every tolerance computed per element / per channel from float64 reference quantities
    (u = 2^-24, k = number of rounded fp32 operations, written beside each assert).  The bf16 output rounding is the half ulp of the
    value that was rounded, 2^(floor(log2 |v|) - 8) with |v| <= |ref| + k u A: bf16 has 8 significand bits, so round-to-nearest errs by
    up to 2^-8 |v| at the bottom of a binade; 2^-9 |v| is the half ulp only at the top of one (a correctly rounded kernel measures
    1.99 against 2^-9 |v|, and 1.00 against the half ulp).
 4. partial-row fold (more than 4096 rows) and column finalize with test-made rows.
 5. the inference coefficient kernels.   6. Adam / SGD.

Geometry grid (section 2).  VEC = 4 (fp32) / 8 (bf16) channels per thread, CV = C / VEC, PPI = 256 / CV pixels per iteration, one
trip of the unrolled loop = 4 PPI pixels.  wg = workgroups; "live a/4" = pixels slots alive in the last trip.

  M, C           options                         what the row is there for
  1, 8           single +resid, leaky, strided   M = 1; CV at its minimum (bf16 CV = 1, fp32 CV = 2): the whole shuffle fold
  127, 8         dual, relu, base + 24 ch        M = PPI - 1 (fp32); M not a multiple of PPI
  255, 8         s1 = NULL + resid (plain add)   M = PPI - 1 (bf16); fp32 last trip live 2/4
  1000, 24       dual + resid, leaky, strided    CV = 3 / 6 (forward, apply, colsum); the reduce must answer MDCV_EARG
  3001, 16       dual + resid, leaky, base + 24  several workgroups, ragged last workgroup, fp32 last trip live 3/4
  5408, 1024     single + resid, leaky           real 13x13 x 32; fp32 CV = 256 (`CV > 64` wave selection), bf16 CV = 128
  21632, 512     single, leaky                   real 26x26 x 32; bf16 CV = 64 (one wave per vector), fp32 CV = 128; fp32 reduce 3 trips, live 3/4
  86528, 256     dual + resid, leaky, base + 8   real 52x52 x 32 (and the head column sum); fp32 CV = 64; 984 reduce wg; last trip live 2/4, 3/4
  346112, 128    single, leaky                   real 104x104 x 32; 1967 forward wg, 1007 / 984 reduce wg, 6 - 11 trips
  1638400, 64    single, leaky                   RektNet 80x80 x 256; BOTH caps reached exactly (2048 forward wg, 1024 reduce rows), 7 - 25 trips
  651420, 32     dual, relu, strided             1018 reduce wg with a ragged tail (the 416x416 x 32 tensor has 1018); last trip live 1/4
  3001, 2048     single + resid (bf16 only)      bf16 CV = 256; last workgroup of one pixel; fp32 must answer MDCV_EARG (CV = 512)
  70001, 256     s1 = NULL, no resid (copy)      ragged everywhere: M % PPI = 1, last workgroup 17 / 1 pixels, last trip live 1/4
  40003, 512     dual + resid, leaky, strided    2001 forward wg (cap within 3 %), 1001 reduce wg, last workgroup of 3 pixels
  9001, 1024     single, relu, strided           fp32 CV = 256 with 2 - 3 trips, live 1/4; last workgroup of one pixel

"strided": every leading dimension differs from C and from every other one (C + 8, + 16, ...) and every base pointer is offset by 8
or 24 channels into its buffer; the others are contiguous (ld = C), as the plans pass most tensors.  The dual rows run the two-BatchNorm
form (y2), the others the single one.  The reduce row counts the table quotes are asserted from mdcv_bn_act_bwd_reduce_ws_floats.
The forward / apply workgroup counts and the "live a/4" figures have no public query: they are computed by hand from make_strip(M, C, 2048, 4)
and make_strip(M, C, kReduceBlocks = 1024, 8) in csrc/strip.h as of this commit; a change of the strip heuristics needs the table redone.
mdcv_bn_act_bwd_reduce_finalize's column stage only ever sees the reduce kernel's own rows (at most 1024); test_reduce_finalize_row_counts
drives it at 1, 63, 64 and 65 rows, the fold tests of section 4 drive the other two entry points up to 20 001 rows.

Run with ``-s`` to see the worst error / bound ratio of every group (DESIGN.md section 5 records them).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from test_gpu_kernels import F32, BF16, TD, st  # noqa: E402

U = 2.0 ** -24            # unit roundoff of fp32
EARG = -1
SENT = {F32: 0x5A5A5A5A, BF16: 0x5A5A}
ITYPE = {F32: torch.int32, BF16: torch.int16}
DT = pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
RATIOS = {}


def note(group, r):
    r = float(r)
    RATIOS[group] = max(RATIOS.get(group, 0.0), r)
    print(f"[ratio] {group}: {r:.4f}")


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nworst error / bound per group:")
    for k in sorted(RATIOS):
        print(f"  {k:28s} {RATIOS[k]:.4f}")


def P(t):
    return t.data_ptr() if t is not None else None


def w64(t):
    """device (or host) tensor of any dtype -> float64 on the CPU (exact widening)"""
    return t.detach().float().cpu().double() if t.dtype == torch.bfloat16 else t.detach().cpu().double()


class Buf:
    """[M, C] values inside a sentinel-filled [M + tail, ld] device buffer at channel offset `off`"""

    def __init__(self, dt, M, C, ld=None, off=0, tail=0, vals=None):
        self.dt, self.M, self.C, self.ld, self.off = dt, M, C, ld or C, off
        assert self.ld >= off + C and self.ld % 8 == 0 and off % 8 == 0
        self.full = torch.full((M + tail, self.ld), SENT[dt], dtype=ITYPE[dt], device="cuda").view(TD[dt])
        if vals is not None:
            self.full[:M, off:off + C] = vals.to(TD[dt])
        self.ptr = self.full.data_ptr() + off * self.full.element_size()

    def rows(self, r0, r1):
        return w64(self.full[r0:r1, self.off:self.off + self.C])

    def assert_sentinel_intact(self):
        raw = self.full.view(ITYPE[self.dt])
        s = SENT[self.dt]
        assert bool((raw[:self.M, :self.off] == s).all()) and bool((raw[:self.M, self.off + self.C:] == s).all()), "wrote outside the channel slice"
        assert bool((raw[self.M:] == s).all()), "wrote beyond row M"


def layouts(C, strided, n, base=8):
    """n (ld, off) pairs: all leading dimensions different from C and from each other, offsets 8 / 24 channels"""
    if not strided:
        return [(C, 0)] * n
    return [(C + 24 + 8 * (i + 1), base if i % 2 == 0 else 32 - base) for i in range(n)]


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, device="cuda")


def randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda").float()


def half_ulp_bf16(x):
    """half a unit in the last place of bf16 (8 significand bits) at magnitude x >= 0: 2^(floor(log2 x) - 8); between 2^-9 x and 2^-8 x"""
    _, e = torch.frexp(x)                      # x = m 2^e, m in [1/2, 1)
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), e - 9), torch.zeros_like(x))


def chunks(M, C):
    step = max(1, (1 << 23) // C)
    return [(r0, min(M, r0 + step)) for r0 in range(0, M, step)]


def cdiv(a, b):
    return (a + b - 1) // b


# (M, C, dual, resid, act, s1null, strided, base offset, dtypes)
GEOM = [
    (1, 8, False, True, 1, False, True, 8, (F32, BF16)),
    (127, 8, True, False, 2, False, True, 24, (F32, BF16)),
    (255, 8, False, True, 0, True, True, 8, (F32, BF16)),
    (1000, 24, True, True, 1, False, True, 8, (F32, BF16)),
    (3001, 16, True, True, 1, False, True, 24, (F32, BF16)),
    (5408, 1024, False, True, 1, False, False, 0, (F32, BF16)),
    (21632, 512, False, False, 1, False, False, 0, (F32, BF16)),
    (86528, 256, True, True, 1, False, True, 8, (F32, BF16)),
    (346112, 128, False, False, 1, False, False, 0, (F32, BF16)),
    (1638400, 64, False, False, 1, False, False, 0, (F32, BF16)),
    (651420, 32, True, False, 2, False, True, 8, (F32, BF16)),
    (3001, 2048, False, True, 1, False, True, 8, (BF16,)),
    (70001, 256, False, False, 0, True, False, 0, (F32, BF16)),
    (40003, 512, True, True, 1, False, True, 24, (F32, BF16)),
    (9001, 1024, False, False, 2, False, True, 8, (F32, BF16)),
]
GEOM_IDS = [f"M{c[0]}-C{c[1]}" for c in GEOM]
# reduce rows (workgroups) the docstring table quotes, per dtype: asserted from the public workspace query
TABLE_ROWS = {(1638400, 64): (1024, 1024), (86528, 256): (984, 984), (346112, 128): (1007, 984), (651420, 32): (1018, 1018),
              (40003, 512): (1001, 1001), (21632, 512): (984, 676), (5408, 1024): (676, 338), (1, 8): (1, 1)}


def reduce_rows(L, dt, M, C, nsums):
    return L.bn_act_bwd_reduce_ws_floats(dt, M, C, nsums) // (nsums * C)


def coef(g, C, kind):
    if kind == "scale":
        return (torch.rand(C, generator=g, device="cuda") + 0.5) * torch.where(torch.rand(C, generator=g, device="cuda") < 0.25, -1.0, 1.0)
    return randn(g, C) * 0.3 + 0.1


def actf(pre, act, slope):
    return pre if act == 0 else torch.where(pre > 0, pre, pre * slope)


def agrad(pre, act, slope):
    return torch.ones_like(pre) if act == 0 else torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))


# ---------------------------------------------------------------- sections 1 - 3: forward
@DT
@pytest.mark.parametrize("case", GEOM, ids=GEOM_IDS)
def test_bn_act_fwd_vs_fp64(case, dt):
    M, C, dual, resid, act, s1null, strided, base, dts = case
    L = _lib.lib()
    if dt not in dts:       # CV = C / VEC > 256: refused, not launched
        y = Buf(dt, 8, C, vals=torch.zeros(8, C, device="cuda"))
        o = Buf(dt, 8, C)
        assert L.bn_act_fwd(dt, y.ptr, C, None, None, None, 0, None, None, None, 0, o.ptr, C, 8, C, 0, 0.0, st()) == EARG
        torch.cuda.synchronize()
        o.assert_sentinel_intact()
        return
    g = gen(1000 + M + C)
    slope = 0.1
    (l1, o1), (l2, o2), (lr, orr), (lo, oo) = layouts(C, strided, 4, base)
    y1 = Buf(dt, M, C, l1, o1, vals=randn(g, M, C) * 1.5 + 0.3)
    y2 = Buf(dt, M, C, l2, o2, vals=randn(g, M, C)) if dual else None
    rs = Buf(dt, M, C, lr, orr, vals=randn(g, M, C)) if resid else None
    out = Buf(dt, M, C, lo, oo, tail=3 if strided else 0)
    s1 = None if s1null else coef(g, C, "scale")
    b1 = None if s1null else coef(g, C, "shift")
    s2, b2 = (coef(g, C, "scale"), coef(g, C, "shift")) if dual else (None, None)
    L.check(L.bn_act_fwd(dt, y1.ptr, l1, P(s1), P(b1), y2.ptr if dual else None, l2, P(s2), P(b2), rs.ptr if resid else None, lr,
                         out.ptr, lo, M, C, act, slope, st()))
    torch.cuda.synchronize()
    out.assert_sentinel_intact()
    S1 = w64(s1) if s1 is not None else torch.ones(C, dtype=torch.float64)
    B1 = w64(b1) if b1 is not None else torch.zeros(C, dtype=torch.float64)
    sl = float(np.float32(0.0 if act == 2 else slope))
    worst = 0.0
    for r0, r1 in chunks(M, C):
        t1 = y1.rows(r0, r1) * S1
        pre = t1 + B1
        A = t1.abs() + B1.abs()
        if dual:
            t2 = y2.rows(r0, r1) * w64(s2)
            pre = pre + t2 + w64(b2)
            A = A + t2.abs() + w64(b2).abs()
        ref = actf(pre, act, sl)
        if resid:
            r = rs.rows(r0, r1)
            ref = ref + r
            A = A + r.abs()
        # k = 7 rounded fp32 operations at most: y1*s1, +b1, y2*s2, +b2, the sum of the two branches, *slope, +resid
        bound = 7 * U * A
        if dt == BF16:
            bound = bound + half_ulp_bf16(ref.abs() + 7 * U * A)
        err = (out.rows(r0, r1) - ref).abs()
        assert bool((err <= bound).all()), f"rows {r0}..{r1}: max err/bound {float((err / bound.clamp_min(1e-300)).max())}"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    note(f"fwd {'bf16' if dt else 'fp32'}", worst)


# ---------------------------------------------------------------- sections 1 - 3: backward reduce (+ finalize) and apply
def _bwd_inputs(dt, M, C, dual, strided, base, exact, g):
    (ld, od), (l1, o1), (l2, o2), (ly1, oy1), (ly2, oy2) = layouts(C, strided, 5, base)
    if exact:
        dout = Buf(dt, M, C, ld, od, vals=randint(g, -3, 3, M, C))
        y1 = Buf(dt, M, C, l1, o1, vals=randint(g, -4, 4, M, C))
        y2 = Buf(dt, M, C, l2, o2, vals=randint(g, -4, 4, M, C)) if dual else None
        pick = torch.tensor([0.5, 1.0, 2.0], device="cuda")
        co = dict(s1=torch.ones(C, device="cuda"), b1=torch.zeros(C, device="cuda"), m1=randint(g, -1, 1, C), i1=pick[torch.randint(0, 3, (C,), generator=g, device="cuda")],
                  s2=torch.ones(C, device="cuda"), b2=torch.zeros(C, device="cuda"), m2=randint(g, -1, 1, C), i2=pick[torch.randint(0, 3, (C,), generator=g, device="cuda")],
                  g1=torch.ones(C, device="cuda"), g2=torch.ones(C, device="cuda"))
    else:
        dout = Buf(dt, M, C, ld, od, vals=randn(g, M, C))
        y1 = Buf(dt, M, C, l1, o1, vals=randn(g, M, C) * 1.5 + 0.3)
        y2 = Buf(dt, M, C, l2, o2, vals=randn(g, M, C) * 0.7 - 0.2) if dual else None
        co = {}
        for k, mu, sd in (("1", 0.3, 1.5), ("2", -0.2, 0.7)):
            co["g" + k] = coef(g, C, "scale")
            co["m" + k] = mu + randn(g, C) * 0.05
            co["i" + k] = (1.0 / sd) * (1.0 + 0.1 * torch.rand(C, generator=g, device="cuda"))
            co["s" + k] = co["g" + k] * co["i" + k]
            co["b" + k] = coef(g, C, "shift") - co["m" + k] * co["s" + k]
    return dout, y1, y2, co, (ld, l1, l2, ly1, ly2, oy1, oy2)


def _ref_sums(dout, y1, y2, co, M, C, dual, act, sl, exact):
    """float64 per-channel sums [3][C], sums of |term|, kink slack, ambiguous count, max |term| -- from the stored values alone"""
    c = {k: w64(v) for k, v in co.items()}
    S = torch.zeros(3, C, dtype=torch.float64)
    SA = torch.zeros(3, C, dtype=torch.float64)
    slack = torch.zeros(3, C, dtype=torch.float64)
    tmax = torch.zeros(3, C, dtype=torch.float64)
    namb = 0
    for r0, r1 in chunks(M, C):
        d, a = dout.rows(r0, r1), y1.rows(r0, r1)
        t1 = a * c["s1"]
        pre = t1 + c["b1"]
        pa = t1.abs() + c["b1"].abs()
        x1 = (a - c["m1"]) * c["i1"]
        xs = [torch.ones_like(x1), x1]
        if dual:
            b = y2.rows(r0, r1)
            t2 = b * c["s2"]
            pre = pre + t2 + c["b2"]
            pa = pa + t2.abs() + c["b2"].abs()
            xs.append((b - c["m2"]) * c["i2"])
        gg = d * agrad(pre, act, sl)
        # the fp32 `pre` carries at most 3 roundings (fma, fma, add): below that the branch of act' is not determined
        # (integer data: `pre` is exact in fp32, pre == 0 takes the slope branch in both)
        amb = (pre.abs() < 3 * U * pa) if act != 0 and not exact else torch.zeros_like(pre, dtype=torch.bool)
        namb += int(amb.sum())
        for k, x in enumerate(xs):
            t = gg * x
            S[k] += t.sum(0)
            SA[k] += t.abs().sum(0)
            tmax[k] = torch.maximum(tmax[k], t.abs().amax(0))
            if namb:
                slack[k] += torch.where(amb, (d * x).abs() * abs(1.0 - sl), torch.zeros_like(d)).sum(0)
    return S, SA, slack, namb, tmax


def _bwd_args(dt, dout, ld, y1, l1, y2, l2, co, dual):
    """the leading arguments mdcv_bn_act_bwd_reduce and mdcv_bn_act_bwd_reduce_finalize share"""
    return (dt, dout.ptr, ld, y1.ptr, l1, P(co["s1"]), P(co["b1"]), P(co["m1"]), P(co["i1"]), y2.ptr if dual else None, l2,
            P(co["s2"]) if dual else None, P(co["b2"]) if dual else None, P(co["m2"]) if dual else None, P(co["i2"]) if dual else None)


def _check_apply(L, dt, M, C, dual, act, slope, strided, dout, y1, y2, co, f1, f2, lds):
    """pass 2, dy_i = cA_i g + cB_i y_i + cC_i, with the coefficients f1 / f2 hold on the device, per element against float64"""
    ld, l1, l2, ly1, ly2, oy1, oy2 = lds
    sl = float(np.float32(0.0 if act == 2 else slope))
    c64 = {k: w64(v) for k, v in co.items()}
    dy1 = Buf(dt, M, C, ly1, oy1, tail=3 if strided else 0)
    dy2 = Buf(dt, M, C, ly2, oy2, tail=3 if strided else 0) if dual else None
    L.check(L.bn_act_bwd_apply(dt, dout.ptr, ld, y1.ptr, l1, P(co["s1"]), P(co["b1"]), P(f1[2]), P(f1[3]), P(f1[4]), dy1.ptr, ly1,
                               y2.ptr if dual else None, l2, P(co["s2"]) if dual else None, P(co["b2"]) if dual else None,
                               P(f2[2]) if dual else None, P(f2[3]) if dual else None, P(f2[4]) if dual else None,
                               dy2.ptr if dual else None, ly2, M, C, act, slope, st()))
    torch.cuda.synchronize()
    dy1.assert_sentinel_intact()
    if dual:
        dy2.assert_sentinel_intact()
    worst = 0.0
    for r0, r1 in chunks(M, C):
        d, a = dout.rows(r0, r1), y1.rows(r0, r1)
        t1 = a * c64["s1"]
        pre, pa = t1 + c64["b1"], t1.abs() + c64["b1"].abs()
        if dual:
            b = y2.rows(r0, r1)
            t2 = b * c64["s2"]
            pre, pa = pre + t2 + c64["b2"], pa + t2.abs() + c64["b2"].abs()
        ag = agrad(pre, act, sl)
        amb = (pre.abs() < 3 * U * pa) if act != 0 else torch.zeros_like(pre, dtype=torch.bool)
        alt = torch.where(ag == 1.0, torch.full_like(ag, sl), torch.ones_like(ag))
        for f, y, dy in ((f1, a, dy1),) + (((f2, b, dy2),) if dual else ()):
            cA, cB, cC = w64(f[2]), w64(f[3]), w64(f[4])
            got = dy.rows(r0, r1)
            res = []
            for gr in (ag, alt):
                ref = cA * (d * gr) + cB * y + cC
                A = (cA * d * gr).abs() + (cB * y).abs() + cC.abs()
                # k = 5: d*act', cA*g, cB*y, two additions
                bound = 5 * U * A + (half_ulp_bf16(ref.abs() + 5 * U * A) if dt == BF16 else 0.0)
                res.append((got - ref).abs() / bound.clamp_min(1e-300))
            ratio = torch.where(amb, torch.minimum(res[0], res[1]), res[0])     # on the kink either branch is accepted
            assert bool((ratio <= 1.0).all()), f"rows {r0}..{r1}: max err/bound {float(ratio.max())}"
            worst = max(worst, float(ratio.max()))
    note(f"bwd apply {'bf16' if dt else 'fp32'}", worst)


# The float64 reference is what this module's time goes to.  Trimmed, largest first: the random (accuracy) backward of the three largest
# tensors runs in bf16 only (the dtype the plans use); their exact cases, which are what needs the size, run in both dtypes.
# (C = 24 and fp32 C = 2048 are widths the reduce refuses: test_bn_act_bwd_reduce_refuses, test_bn_act_bwd_apply_without_reduce)
BWD_CASES = [pytest.param(c, e, d, id=f"{i}-{'exact' if e else 'random'}-{'bf16' if d else 'fp32'}")
             for c, i in zip(GEOM, GEOM_IDS) for e in (True, False) for d in c[8] if c[1] != 24 and (e or d == BF16 or c[0] < 346112)]


@pytest.mark.parametrize("case,exact,dt", BWD_CASES)
def test_bn_act_bwd_vs_fp64(case, exact, dt):
    M, C, dual, resid, act, s1null, strided, base, dts = case
    L = _lib.lib()
    nsums = 3 if dual else 2
    g = gen(2000 + M + C + (7 if exact else 0))
    slope = 0.5 if exact else 0.1
    sl = float(np.float32(0.0 if act == 2 else slope))
    rows = reduce_rows(L, dt, M, C, nsums)
    if (M, C) in TABLE_ROWS:
        assert rows == TABLE_ROWS[(M, C)][dt], (rows, "the docstring table is out of date")
    dout, y1, y2, co, lds = _bwd_inputs(dt, M, C, dual, strided, base, exact, g)
    ld, l1, l2 = lds[:3]
    S, SA, slack, namb, tmax = _ref_sums(dout, y1, y2, co, M, C, dual, act, sl, exact)
    assert namb <= 1e-4 * M * C, f"{namb} of {M * C} elements sit on the activation kink: pick other inputs"
    f1 = [torch.zeros(C, device="cuda") for _ in range(5)]
    f2 = [torch.zeros(C, device="cuda") for _ in range(5)]
    a = _bwd_args(dt, dout, ld, y1, l1, y2, l2, co, dual)
    ws = torch.empty(rows * nsums * C, device="cuda")
    acc = torch.zeros(nsums * C, dtype=torch.float64, device="cuda")
    L.check(L.bn_act_bwd_reduce(*a, acc.data_ptr(), ws.data_ptr(), M, C, act, slope, st()))
    ws2 = torch.empty(rows * nsums * C, device="cuda")
    L.check(L.bn_act_bwd_reduce_finalize(*a, ws2.data_ptr(), M, C, act, slope, float(M), P(co["g1"]), *[P(t) for t in f1],
                                         P(co["g2"]) if dual else None, *[(P(t) if dual else None) for t in f2], st()))
    torch.cuda.synchronize()
    accv = acc.cpu().reshape(nsums, C)
    dbeta, dg1, dg2 = w64(f1[1]), w64(f1[0]), w64(f2[0])
    if exact:
        # every term is a multiple of 1/4 (g of 1/2, invstd of 1/2): condition for "no fp32 partial can round", from the reference alone.
        # A workgroup sums at most ceil(M / 64) pixels of a channel (so does a fold row); the fp64 column totals are cast to fp32 once.
        q = 0.25
        assert float(tmax.max()) / q * cdiv(M, 64) < 2 ** 24 and float(S.abs().max()) / q < 2 ** 24
        assert bool((S[:nsums] * 4 == (S[:nsums] * 4).round()).all())
        want = (S[:nsums] * 4).round().to(torch.int64)
        assert torch.equal((accv * 4).to(torch.int64), want) and bool((accv * 4 == (accv * 4).round()).all()), "bwd_reduce accumulators"
        assert torch.equal((dbeta * 4).to(torch.int64), want[0]) and torch.equal((dg1 * 4).to(torch.int64), want[1]), "dbeta / dgamma #1"
        assert bool((dbeta * 4 == want[0].double()).all()) and bool((dg1 * 4 == want[1].double()).all())
        if dual:
            assert bool((dg2 * 4 == want[2].double()).all()) and bool((w64(f2[1]) * 4 == want[0].double()).all()), "dgamma / dbeta #2"
        return
    # recursive-summation bound; n = the longest fp32 chain <= ceil(M / rows) pixels of a workgroup + 256 for its fold
    # (the <= 4 roundings inside a term are covered by the + 256), plus one rounding of the stored total
    n = cdiv(M, rows) + 256
    bound = (n - 1) * U * SA[:nsums] + U * S[:nsums].abs() + slack[:nsums]
    for name, got in (("accum", accv), ("finalize", torch.stack([dbeta, dg1] + ([dg2] if dual else [])))):
        err = (got - S[:nsums]).abs()
        assert bool((err <= bound).all()), f"{name}: err/bound {float((err / bound.clamp_min(1e-300)).max())}"
        note(f"bwd sums {'bf16' if dt else 'fp32'}", (err / bound.clamp_min(1e-300)).max())
    if dual:
        assert bool(((w64(f2[1]) - S[0]).abs() <= bound[0]).all())
    # finalize outputs from the device's own fp32 sums: k = 2 (the sum was rounded to fp32 once; the coefficient is stored once)
    c64 = {k: w64(v) for k, v in co.items()}
    for sfx, f in (("1", f1), ("2", f2))[:2 if dual else 1]:
        gm, isd, mu = c64["g" + sfx], c64["i" + sfx], c64["m" + sfx]
        mg, mgx = w64(f[1]) / M, w64(f[0]) / M
        ta, tb = gm * isd * mg, gm * isd * isd * mu * mgx
        for name, got, ref, A in (("cA", f[2], gm * isd, (gm * isd).abs()), ("cB", f[3], -gm * isd * isd * mgx, (gm * isd * isd * mgx).abs()),
                                  ("cC", f[4], -ta + tb, ta.abs() + tb.abs())):
            err = (w64(got) - ref).abs()
            assert bool((err <= 2 * U * A).all()), f"{name}{sfx}: err/bound {float((err / (2 * U * A).clamp_min(1e-300)).max())}"
            note("bwd coefficients", (err / (2 * U * A).clamp_min(1e-300)).max())
    _check_apply(L, dt, M, C, dual, act, slope, strided, dout, y1, y2, co, f1, f2, lds)


@pytest.mark.parametrize("C,dt", [(24, F32), (24, BF16), (2048, F32)], ids=["C24-fp32", "C24-bf16", "C2048-fp32"])
def test_bn_act_bwd_reduce_refuses(C, dt):
    """CV = C / VEC that does not divide 256 (3, 6) or exceeds it (512): both reduce entry points answer MDCV_EARG and launch nothing"""
    L = _lib.lib()
    M = 64
    dout, y1, y2, co, _ = _bwd_inputs(dt, M, C, True, False, 0, True, gen(C))
    ws = torch.full((4 * 3 * C,), 7.0, device="cuda")
    acc = torch.zeros(3 * C, dtype=torch.float64, device="cuda")
    o = [torch.full((C,), 7.0, device="cuda") for _ in range(10)]
    for dual in (False, True):
        a = _bwd_args(dt, dout, C, y1, C, y2, C, co, dual)
        assert L.bn_act_bwd_reduce(*a, acc.data_ptr(), ws.data_ptr(), M, C, 1, 0.5, st()) == EARG
        assert L.bn_act_bwd_reduce_finalize(*a, ws.data_ptr(), M, C, 1, 0.5, float(M), P(co["g1"]), *[P(t) for t in o[:5]],
                                            P(co["g2"]) if dual else None, *[(P(t) if dual else None) for t in o[5:]], st()) == EARG
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0 and all(bool((t == 7.0).all()) for t in o + [ws])


@DT
def test_bn_act_bwd_apply_without_reduce(dt):
    """the (1000, 24) row of the table for the apply pass: CV = 3 / 6, no reduce exists for this width, so the coefficients are the test's own"""
    M, C, dual, resid, act, s1null, strided, base, dts = GEOM[3]
    assert C == 24
    g = gen(2500 + dt)
    dout, y1, y2, co, lds = _bwd_inputs(dt, M, C, dual, strided, base, False, g)
    f1 = [randn(g, C) * 0.5 for _ in range(5)]
    f2 = [randn(g, C) * 0.5 for _ in range(5)]
    _check_apply(_lib.lib(), dt, M, C, dual, act, 0.1, strided, dout, y1, y2, co, f1, f2, lds)


@DT
def test_reduce_finalize_row_counts(dt):
    """the column stage of mdcv_bn_act_bwd_reduce_finalize at 1, 63, 64, 65 partial rows (its 64 row lanes: one short, full, one over)"""
    L = _lib.lib()
    C = 8
    lo, hi = 1, 1 << 20
    while lo < hi:          # pixels per workgroup, from the public query alone: the largest M that still is one row
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if reduce_rows(L, dt, mid, C, 3) == 1 else (lo, mid - 1)
    PB = lo
    for want in (1, 63, 64, 65):
        M = want * PB - 3
        assert reduce_rows(L, dt, M, C, 3) == want
        g = gen(M)
        dout, y1, y2, co, _ = _bwd_inputs(dt, M, C, True, False, 0, True, g)
        S, SA, slack, namb, tmax = _ref_sums(dout, y1, y2, co, M, C, True, 1, 0.5, True)
        assert float(tmax.max()) * 4 * cdiv(M, 64) < 2 ** 24 and float(S.abs().max()) * 4 < 2 ** 24
        f1 = [torch.zeros(C, device="cuda") for _ in range(5)]
        f2 = [torch.zeros(C, device="cuda") for _ in range(5)]
        ws = torch.empty(want * 3 * C, device="cuda")
        L.check(L.bn_act_bwd_reduce_finalize(dt, dout.ptr, C, y1.ptr, C, P(co["s1"]), P(co["b1"]), P(co["m1"]), P(co["i1"]), y2.ptr, C, P(co["s2"]),
                                             P(co["b2"]), P(co["m2"]), P(co["i2"]), ws.data_ptr(), M, C, 1, 0.5, float(M), P(co["g1"]),
                                             *[P(t) for t in f1], P(co["g2"]), *[P(t) for t in f2], st()))
        torch.cuda.synchronize()
        assert torch.equal(w64(f1[1]), S[0]) and torch.equal(w64(f1[0]), S[1]) and torch.equal(w64(f2[0]), S[2]) and torch.equal(w64(f2[1]), S[0]), want


# ---------------------------------------------------------------- column sums
@DT
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("case", GEOM, ids=GEOM_IDS)
def test_colsum_vs_fp64(case, exact, dt):
    M, C, _, _, _, _, strided, base, dts = case
    L = _lib.lib()
    if dt not in dts:       # CV = C / VEC > 256: both forms refuse and write nothing
        x = Buf(dt, 8, C, vals=torch.ones(8, C, device="cuda"))
        acc = torch.zeros(C, dtype=torch.float64, device="cuda")
        ws, o = torch.full((8 * C,), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")
        assert L.colsum(dt, x.ptr, C, 8, C, acc.data_ptr(), st()) == EARG
        assert L.colsum_f32(dt, x.ptr, C, 8, C, ws.data_ptr(), o.data_ptr(), st()) == EARG
        torch.cuda.synchronize()
        assert float(acc.abs().max()) == 0.0 and bool((ws == 7.0).all()) and bool((o == 7.0).all())
        return
    g = gen(3000 + M + C)
    (ld, off), = layouts(C, strided, 1, base)
    x = Buf(dt, M, C, ld, off, vals=randint(g, -4, 4, M, C) if exact else randn(g, M, C) + 0.25)
    rows = L.colsum_ws_floats(dt, M, C) // C
    ws = torch.empty(rows * C, device="cuda")
    o1 = torch.zeros(C, device="cuda")
    L.check(L.colsum_f32(dt, x.ptr, ld, M, C, ws.data_ptr(), o1.data_ptr(), st()))
    acc = torch.zeros(C, dtype=torch.float64, device="cuda")
    o2 = torch.full((C,), 7.0, device="cuda")
    L.check(L.colsum(dt, x.ptr, ld, M, C, acc.data_ptr(), st()))
    L.check(L.accum_to_f32(acc.data_ptr(), o2.data_ptr(), C, 1, st()))
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0          # zero_after
    S = torch.zeros(C, dtype=torch.float64)
    SA = torch.zeros(C, dtype=torch.float64)
    for r0, r1 in chunks(M, C):
        v = x.rows(r0, r1)
        S += v.sum(0)
        SA += v.abs().sum(0)
    if exact:
        assert 4 * cdiv(M, 64) < 2 ** 24 and float(S.abs().max()) < 2 ** 24
        assert torch.equal(w64(o1), S) and torch.equal(w64(o2), S)
    else:
        n = cdiv(M, rows) + 256            # one workgroup's pixels + its fold; k = n - 1 additions, one rounding of the stored total
        bound = (n - 1) * U * SA + U * S.abs()
        for got in (o1, o2):
            err = (w64(got) - S).abs()
            assert bool((err <= bound).all())
            note(f"colsum {'bf16' if dt else 'fp32'}", (err / bound.clamp_min(1e-300)).max())


# ---------------------------------------------------------------- section 4: partial-row fold and column finalize
FOLD_ROWS = [1, 63, 64, 65, 4095, 4096, 4097, 8191, 12800, 20001]
FOLD_C = [(8, 8), (24, 24), (64, 64), (1000, 1008), (1024, 1024)]      # (channels, padded width: 1000 real channels in 1008)
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))


def _make_rows(rows, C, Cp, exact, g, stats):
    """[rows][2][Cp] fp32 partial rows; channels >= C (the pad of C = 1000) are zero"""
    part = torch.zeros(rows, 2, Cp, device="cuda")
    if exact:
        part[:, 0, :C] = randint(g, -8, 8, rows, C)
        part[:, 1, :C] = randint(g, 0, 64, rows, C) if stats else randint(g, -8, 8, rows, C)
    elif stats:     # as if every row summed 16 pixels of mean 0.3 and mean square ~2
        part[:, 0, :C] = 16 * 0.3 + randn(g, rows, C) * 4
        part[:, 1, :C] = 16 * (1.5 + torch.rand(rows, C, generator=g, device="cuda"))
    else:
        part[:, 0, :C] = randn(g, rows, C) * 3
        part[:, 1, :C] = randn(g, rows, C) * 5
    return part


def _sum_err(rows, absum):
    """error of the device's fp64 column sums: fp64 rounding only, plus one fp32 rounding per folded row on the fold path
    (the bound the fold is given: 64 u sum |row values|)"""
    return (64 * U * absum if rows > 4096 else 0.0) + rows * 2.0 ** -53 * absum


def _stats_ref(S, Q, eS, eQ, count, gam, bet, rm, rv):
    """float64 statistics from the column sums, and the propagated error bound of every output (first order in eS, eQ)"""
    mean = S / count
    var = (Q / count - mean * mean).clamp_min(0.0)
    e_mean = eS / count
    e_var = eQ / count + 2 * mean.abs() * e_mean + 4 * 2.0 ** -53 * (Q.abs() / count + mean * mean)
    isd = 1.0 / torch.sqrt(var + EPS)
    e_is = 0.5 * ((var - e_var).clamp_min(0.0) + EPS) ** -1.5 * e_var
    unb = var * count / (count - 1.0) if count > 1.0 else var
    e_unb = e_var * (count / (count - 1.0) if count > 1.0 else 1.0)
    t = mean * gam * isd
    e_t = e_mean * (gam * isd).abs() + (mean * gam).abs() * e_is
    ref = dict(scale=gam * isd, shift=bet - t, mean=mean, invstd=isd)
    # k: mean, invstd: the fp32 store (1).  scale: store of invstd, product (2).  shift: (float)mean, invstd, two products, subtraction (5)
    bnd = dict(scale=gam.abs() * e_is + 2 * U * (gam * isd).abs(), shift=e_t + 5 * U * (bet.abs() + t.abs()),
               mean=e_mean + U * mean.abs(), invstd=e_is + U * isd)
    if rm is not None:
        # k = 5: 1 - momentum, two products, the sum, the fp32 cast of mean / unbiased
        ref.update(rm=(1 - MOM) * rm + MOM * mean, rv=(1 - MOM) * rv + MOM * unb)
        bnd.update(rm=MOM * e_mean + 5 * U * (((1 - MOM) * rm).abs() + (MOM * mean).abs()), rv=MOM * e_unb + 5 * U * (((1 - MOM) * rv).abs() + (MOM * unb).abs()))
    return ref, bnd


def _run_stats(L, part, rows, Cp, count, gam, bet, rm0, rv0):
    p = part.clone()            # the fold consumes its input
    o = [torch.full((Cp,), 7.0, device="cuda") for _ in range(4)]
    rm, rv = (rm0.clone(), rv0.clone()) if rm0 is not None else (None, None)
    scratch = torch.zeros(3 * Cp, dtype=torch.float64, device="cuda")
    L.check(L.bn_stats_finalize(p.data_ptr(), rows, scratch.data_ptr(), float(count), gam.data_ptr(), bet.data_ptr(), P(rm), P(rv), 0.1, 1e-5,
                                *[t.data_ptr() for t in o], Cp, st()))
    torch.cuda.synchronize()
    return dict(scale=o[0], shift=o[1], mean=o[2], invstd=o[3], **({"rm": rm, "rv": rv} if rm is not None else {}))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("rows", FOLD_ROWS)
def test_bn_stats_finalize_rows(rows, exact):
    L = _lib.lib()
    for C, Cp in FOLD_C:
        g = gen(4000 + rows + C)
        part = _make_rows(rows, C, Cp, exact, g, True)
        count = float(1 << 20) if exact else rows * 16.0
        gam, bet = coef(g, Cp, "scale"), coef(g, Cp, "shift")
        rm0, rv0 = randn(g, Cp) * 0.2, torch.rand(Cp, generator=g, device="cuda") + 0.5
        got = _run_stats(L, part, rows, Cp, count, gam, bet, rm0, rv0)
        again = _run_stats(L, part, rows, Cp, count, gam, bet, rm0, rv0)
        for k in got:
            assert torch.equal(got[k], again[k]), f"{k}: two runs differ (C={C})"
        p64 = w64(part)
        S, Q = p64[:, 0].sum(0), p64[:, 1].sum(0)
        if exact:
            # integer rows: every fp32 / fp64 partial is exact (|sum| <= 64 rows < 2^24), count = 2^20 makes mean = S / count exact
            assert float(p64.abs().sum(0).max()) < 2 ** 24
            assert torch.equal(w64(got["mean"]) * count, S), f"C={C}"
            continue
        A = p64.abs().sum(0)
        ref, bnd = _stats_ref(S, Q, _sum_err(rows, A[0]), _sum_err(rows, A[1]), count, w64(gam), w64(bet), w64(rm0), w64(rv0))
        for k in ref:
            err = (w64(got[k]) - ref[k]).abs()
            assert bool((err <= bnd[k]).all()), f"{k} C={C}: err/bound {float((err / bnd[k].clamp_min(1e-300)).max())}"
            note("stats finalize" + (" (fold)" if rows > 4096 else ""), (err / bnd[k].clamp_min(1e-300)).max())
        if C == 1000:       # the pad channels: all-zero column -> var = 0, invstd = 1 / sqrt(eps)
            assert bool((w64(got["invstd"])[C:] - 1.0 / math.sqrt(EPS)).abs().max() <= U / math.sqrt(EPS)) and float(got["mean"][C:].abs().max()) == 0.0


@pytest.mark.parametrize("count,with_running", [(1.0, True), (37.0, False), (1.0, False)])
def test_bn_stats_finalize_edges(count, with_running):
    """count = 1 (the unbiased variance falls back to var), running_mean == NULL, an all-zero channel"""
    L = _lib.lib()
    C, rows = 64, 5
    g = gen(int(count) + with_running)
    part = _make_rows(rows, C, C, False, g, True)
    part *= count / (rows * 16.0)
    part[:, :, 3] = 0.0
    gam, bet = coef(g, C, "scale"), coef(g, C, "shift")
    rm0, rv0 = (randn(g, C) * 0.2, torch.rand(C, generator=g, device="cuda") + 0.5) if with_running else (None, None)
    got = _run_stats(L, part, rows, C, count, gam, bet, rm0, rv0)
    p64 = w64(part)
    A = p64.abs().sum(0)
    ref, bnd = _stats_ref(p64[:, 0].sum(0), p64[:, 1].sum(0), _sum_err(rows, A[0]), _sum_err(rows, A[1]), count, w64(gam), w64(bet),
                          w64(rm0) if with_running else None, w64(rv0) if with_running else None)
    assert set(ref) == set(got)
    for k in ref:
        err = (w64(got[k]) - ref[k]).abs()
        assert bool((err <= bnd[k]).all()), f"{k}: err/bound {float((err / bnd[k].clamp_min(1e-300)).max())}"
        note("stats finalize", (err / bnd[k].clamp_min(1e-300)).max())
    assert abs(float(got["invstd"][3]) - 1.0 / math.sqrt(EPS)) <= U / math.sqrt(EPS)


def _run_bwd_rows(L, part, rows, Cp, count, gam, mean, isd):
    p = part.clone()
    o = [torch.full((Cp,), 7.0, device="cuda") for _ in range(5)]
    L.check(L.bn_bwd_finalize_rows(p.data_ptr(), rows, Cp, float(count), gam.data_ptr(), mean.data_ptr(), isd.data_ptr(), *[t.data_ptr() for t in o], st()))
    torch.cuda.synchronize()
    return dict(dgamma=o[0], dbeta=o[1], cA=o[2], cB=o[3], cC=o[4])


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("rows", FOLD_ROWS)
def test_bn_bwd_finalize_rows(rows, exact):
    """rows of [sum g, sum g (y - mean)] (the fused data gradient's sums: the second one is not yet divided by std)"""
    L = _lib.lib()
    for C, Cp in FOLD_C:
        g = gen(5000 + rows + C)
        part = _make_rows(rows, C, Cp, exact, g, False)
        count = rows * 16.0
        gam, mean = coef(g, Cp, "scale"), coef(g, Cp, "shift")
        isd = torch.tensor([0.5, 1.0, 2.0], device="cuda")[torch.randint(0, 3, (Cp,), generator=g, device="cuda")] if exact else torch.rand(Cp, generator=g, device="cuda") + 0.5
        got = _run_bwd_rows(L, part, rows, Cp, count, gam, mean, isd)
        again = _run_bwd_rows(L, part, rows, Cp, count, gam, mean, isd)
        for k in got:
            assert torch.equal(got[k], again[k]), f"{k}: two runs differ (C={C})"
        p64 = w64(part)
        S0, S1 = p64[:, 0].sum(0), p64[:, 1].sum(0)
        if exact:
            assert float(p64.abs().sum(0).max()) * 2 < 2 ** 24
            assert torch.equal(w64(got["dbeta"]), S0) and torch.equal(w64(got["dgamma"]), S1 * w64(isd)), f"C={C}"
            continue
        A = p64.abs().sum(0)
        e0, e1 = _sum_err(rows, A[0]), _sum_err(rows, A[1])
        G, MU, IS = w64(gam), w64(mean), w64(isd)
        sgx, e_sgx = S1 * IS, e1 * IS
        ta, tb = G * IS * S0 / count, G * IS * IS * MU * sgx / count
        ref = dict(dbeta=S0, dgamma=sgx, cA=G * IS, cB=-G * IS * IS * sgx / count, cC=-ta + tb)
        # k = 1: every output is formed in fp64 and stored to fp32 once
        bnd = dict(dbeta=e0 + U * S0.abs(), dgamma=e_sgx + U * sgx.abs(), cA=U * (G * IS).abs(),
                   cB=(G * IS * IS).abs() * e_sgx / count + U * ref["cB"].abs(),
                   cC=(G * IS).abs() * e0 / count + (G * IS * IS * MU).abs() * e_sgx / count + U * (ta.abs() + tb.abs()) + 4 * 2.0 ** -53 * (ta.abs() + tb.abs()))
        for k in ref:
            err = (w64(got[k]) - ref[k]).abs()
            assert bool((err <= bnd[k]).all()), f"{k} C={C}: err/bound {float((err / bnd[k].clamp_min(1e-300)).max())}"
            note("bwd finalize rows" + (" (fold)" if rows > 4096 else ""), (err / bnd[k].clamp_min(1e-300)).max())


# ---------------------------------------------------------------- section 5: inference coefficients
@pytest.mark.parametrize("C", [8, 136, 1024])
@pytest.mark.parametrize("bias", [None, False, True], ids=["plain", "bias-null", "bias"])
def test_bn_eval_coeffs(C, bias):
    L = _lib.lib()
    g = gen(6000 + C)
    gam, bet, rm, cb = coef(g, C, "scale"), coef(g, C, "shift"), randn(g, C) * 0.5, randn(g, C) * 0.3
    rv = torch.rand(C, generator=g, device="cuda") + 0.05
    rv[C // 2] = 0.0
    sc, sh = torch.full((C,), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")
    if bias is None:
        L.check(L.bn_eval_coeffs(P(gam), P(bet), P(rm), P(rv), 1e-5, P(sc), P(sh), C, st()))
    else:
        L.check(L.bn_eval_coeffs_bias(P(gam), P(bet), P(rm), P(rv), 1e-5, P(cb) if bias else None, P(sc), P(sh), C, st()))
    torch.cuda.synchronize()
    G, B, RM, RV, CB = w64(gam), w64(bet), w64(rm), w64(rv), (w64(cb) if bias else torch.zeros(C, dtype=torch.float64))
    scale = G / torch.sqrt(RV + EPS)
    shift = B + (CB - RM) * scale
    # invstd = 1 / sqrtf(rv + eps): sum, root, quotient (3); scale: one product more (4).  shift: rm * (gamma invstd) and bias * scale carry
    # 5 roundings each, the two additions one each (7), against the sum of the absolute values of the terms
    e1 = (w64(sc) - scale).abs() / (4 * U * scale.abs())
    A = B.abs() + (RM * scale).abs() + (CB * scale).abs()
    e2 = (w64(sh) - shift).abs() / (7 * U * A).clamp_min(1e-300)
    assert float(e1.max()) <= 1.0 and float(e2.max()) <= 1.0, (float(e1.max()), float(e2.max()))
    note("eval coeffs", max(float(e1.max()), float(e2.max())))


# ---------------------------------------------------------------- section 6: optimizers
CAP = 4096 * 256 * 4        # elements one pass of the Adam grid covers
OPT_N = [1, 3, 4, 5, CAP - 1, CAP + 5, 2 * CAP + 3]
OPT_CASES = [(n, gs, wd) for n in OPT_N[:4] for gs in (1.0, 1.0 / 32) for wd in (0.0, 5e-4)] + \
            [(n, gs, wd) for n in OPT_N[4:] for gs, wd in ((1.0, 0.0), (1.0 / 32, 5e-4))]
f32 = lambda v: float(np.float32(v))  # noqa: E731


def _bc_err(beta, step):
    """relative error of the host's fp32 `1 - powf(beta, step)`: powf within 1 ulp (2 u beta^t), the subtraction (u)"""
    bt = beta ** step
    return 0.0 if step == 1 else 2 * U * bt / (1 - bt) + U       # (step 1: powf(x, 1) = x and 1 - x is exact for x in [1/2, 1])


@pytest.mark.parametrize("n,gs,wd", OPT_CASES, ids=str)
def test_adam_vs_fp64(n, gs, wd):
    L = _lib.lib()
    g = gen(n)
    p, gr = randn(g, n), randn(g, n) * (1.0 / gs)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lr, b1, b2, eps, wdf, gsf = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd), f32(gs)
    G = w64(gr)
    worst = 0.0
    for step in (1, 2, 3, 1000):        # three consecutive steps, then a late one; every step is checked from the state the device holds
        p0, m0, v0 = w64(p), w64(m), w64(v)
        L.check(L.adam_step(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, lr, b1, b2, eps, wdf, gsf, st()))
        torch.cuda.synchronize()
        grad = G * gsf + wdf * p0
        ga = (G * gsf).abs() + (wdf * p0).abs()
        mr, ma = b1 * m0 + (1 - b1) * grad, (b1 * m0).abs() + (1 - b1) * ga
        vr, va = b2 * v0 + (1 - b2) * grad * grad, b2 * v0 + (1 - b2) * ga * ga
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        den = torch.sqrt(vr) / math.sqrt(bc2) + eps
        upd = (lr / bc1) * mr / den
        pr = p0 - upd
        # m: k = 7 (grad: 3; 1 - beta1, two products, sum).  v: k = 10 (grad twice: 6; 1 - beta2, two products... , sum)
        em, ev = (w64(m) - mr).abs() / (7 * U * ma).clamp_min(1e-300), (w64(v) - vr).abs() / (10 * U * va).clamp_min(1e-300)
        # update = (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps): k = 7 for m, 10 / 2 for sqrt(v), 6 for lr / bc1, the root, three
        # quotients / products and the sum, against the update formed with the absolute values of the terms; plus the host's bc1 / bc2
        ua = (lr / bc1) * ma / den
        rel = (7 + 5 + 6) * U + _bc_err(b1, step) + 0.5 * _bc_err(b2, step) + 0.5 * 10 * U * (va / vr.clamp_min(1e-300) - 1)
        bound = U * torch.maximum(p0.abs(), pr.abs()) + rel * ua
        ep = (w64(p) - pr).abs() / bound.clamp_min(1e-300)
        assert float(em.max()) <= 1.0 and float(ev.max()) <= 1.0 and float(ep.max()) <= 1.0, (step, float(em.max()), float(ev.max()), float(ep.max()))
        worst = max(worst, float(em.max()), float(ev.max()), float(ep.max()))
    note("adam", worst)


def test_adam_refuses_a_misaligned_pointer():
    L = _lib.lib()
    t = [torch.zeros(16, device="cuda") for _ in range(4)]
    for k in range(4):
        ptrs = [x.data_ptr() + (4 if i == k else 0) for i, x in enumerate(t)]
        assert L.adam_step(*ptrs, 8, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, st()) == EARG
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0.0 for x in t)


@pytest.mark.parametrize("mom", [0.9, 0.0])
@pytest.mark.parametrize("n,gs,wd", OPT_CASES, ids=str)
def test_sgd_vs_fp64(n, gs, wd, mom):
    L = _lib.lib()
    g = gen(n + 1)
    p, gr = randn(g, n), randn(g, n) * (1.0 / gs)
    buf = torch.zeros(n, device="cuda") if mom else None
    lr, mo, wdf, gsf = f32(1e-2), f32(mom), f32(wd), f32(gs)
    G = w64(gr)
    worst = 0.0
    for step in (1, 2, 3):
        p0, b0 = w64(p), (w64(buf) if mom else None)
        L.check(L.sgd_step(p.data_ptr(), gr.data_ptr(), P(buf), n, step, lr, mo, wdf, gsf, st()))
        torch.cuda.synchronize()
        grad = G * gsf + wdf * p0
        ga = (G * gsf).abs() + (wdf * p0).abs()
        if mom:
            br, ba = (grad, ga) if step == 1 else (mo * b0 + grad, (mo * b0).abs() + ga)
            eb = (w64(buf) - br).abs() / (5 * U * ba).clamp_min(1e-300)      # k = 5: grad (3), product, sum
            assert float(eb.max()) <= 1.0, (step, float(eb.max()))
            worst = max(worst, float(eb.max()))
            grad, ga = br, ba
        pr = p0 - lr * grad
        bound = U * torch.maximum(p0.abs(), pr.abs()) + 6 * U * lr * ga      # k = 6: the 5 above and lr * grad; the final subtraction u |p|
        ep = (w64(p) - pr).abs() / bound.clamp_min(1e-300)
        assert float(ep.max()) <= 1.0, (step, float(ep.max()))
        worst = max(worst, float(ep.max()))
    note("sgd", worst)


@pytest.mark.parametrize("n", [5, CAP // 2 + 5, 2 * CAP + 3])
def test_sgd_exact_dyadic(n):
    """lr = 1/4, parameters and gradients multiples of 1/8, no momentum (NULL buffer), no decay: p - lr g is exact, every element =="""
    L = _lib.lib()
    g = gen(n + 2)
    p, gr = randint(g, -64, 64, n) / 8, randint(g, -32, 32, n) / 8
    ref = w64(p)
    for step in (1, 2, 3):
        L.check(L.sgd_step(p.data_ptr(), gr.data_ptr(), None, n, step, 0.25, 0.0, 0.0, 1.0, st()))
        ref = ref - 0.25 * w64(gr)
    torch.cuda.synchronize()
    assert torch.equal(w64(p), ref)
    assert L.sgd_step(p.data_ptr(), gr.data_ptr(), None, n, 1, 0.25, 0.9, 0.0, 1.0, st()) == EARG      # momentum without a buffer
