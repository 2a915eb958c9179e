"""-m gpu: the two loss heads, csrc/yolo_head.hip (mdcv_yolo_head_train / _grad / _decode) and csrc/rektnet_head.hip (mdcv_softargmax_fwd /
_bwd, mdcv_cross_ratio_loss), through the C ABI against float64 references (tests/helpers/head_refs.py, pinned to the reference project's
recorded outputs by tests/test_head_refs.py).

Tolerances.  Nothing here is a constant fitted to what the kernels return.  For every compared tensor the reference expression is evaluated
twice on the inputs of the case, in float64 (`ref`) and in float32 (`r32`); e32 = max |r32 - ref| is what a correct fp32 evaluation loses,
scale = max |ref|, and the assertion is

    max |kernel - ref|  <=  8 max(e32, 4 u scale),   u = 2^-24                                  (head_refs.bound)

8 covers device expf / logf at a few ulp against libm's half ulp and a different summation order.  bf16 cases: the reference sees the
logits as stored (bf16-rounded), so only fp32 arithmetic and the rounding of the bf16 dlogits remain; the latter adds, per element, the half
ulp of bf16 at the magnitude that was rounded, 2^(floor(log2 |v|) - 8) with |v| <= |ref| + bound.  That is between 2^-9 |v| (top of a binade)
and 2^-8 |v| (bottom): a correctly rounded store measures up to 1.99 against a flat 2^-9 |ref| (tests/test_gpu_elementwise.py records the
same), so the flat figure cannot be met by any bf16 store and the exact half ulp is what is asserted; `lit` in the printed lines is the
worst error against bound + 2^-9 |ref| for the record.
Support is exact: pad and class channels of dlogits are bit-zero, bytes outside the addressed rows / channels keep their sentinel, and
(kernel != 0) == (reference != 0) element by element.

Every comparison prints `[heads] <tag>: err, e32, err/e32, err/bound` (run with -s).  The docstrings quote, from the MI355X run that came
with the tests, the worst err / max(e32, 4 u scale) = 8 err/bound of the test, the figure the assertion holds below 8: err/e32 alone says
nothing where the fp32 evaluation happens to be exact (e32 = 0 for single-term sums, the L1 gradients, the saturated case) and the floor
4 u scale takes over.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from mdcv import _lib  # noqa: E402
from test_gpu_kernels import F32, BF16, TD, st, rnd  # noqa: E402
from test_gpu_elementwise import SENT, ITYPE, EARG, Buf, P  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import head_refs as hr  # noqa: E402

DT = pytest.mark.parametrize("dt", [F32, BF16], ids=["fp32", "bf16"])
F64 = torch.float64
HYPER = (0.5, 2.0, 1.6, 0.1, 25.0)              # thresh, xy, wh, obj, noobj as the C ABI orders them
_REFS = {}


def sync():
    torch.cuda.synchronize()


def report(tag, err, e32, bnd, lit=None):
    r32 = err / e32 if e32 > 0 else float("nan")
    print(f"[heads] {tag}: err {err:.3e} e32 {e32:.3e} err/e32 {r32:.3f} err/bound {err / bnd if bnd > 0 else float(err > 0):.4f}"
          + (f" lit {lit:.3f}" if lit is not None else ""))


def compare(tag, got, ref, r32=None, bf16_store=False):
    """max |got - ref| <= bound(e32, scale) [+ half ulp of bf16 per element]; every argument a CPU float64 tensor"""
    e32 = hr.maxabs(r32 - ref) if r32 is not None else 0.0
    bnd = hr.bound(e32, hr.maxabs(ref))
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite output"
    if not bf16_store:
        report(tag, hr.maxabs(err), e32, bnd)
        assert hr.maxabs(err) <= bnd, f"{tag}: err {hr.maxabs(err):.4e} > bound {bnd:.4e} (e32 {e32:.3e})"
        return
    allowed = bnd + hr.half_ulp_bf16(ref.abs() + bnd)
    lit = float((err / (bnd + 2.0 ** -9 * ref.abs()).clamp_min(1e-300)).max())
    worst = float((err / allowed.clamp_min(1e-300)).max())
    report(tag + " (bf16 store)", hr.maxabs((err - hr.half_ulp_bf16(ref.abs() + bnd)).clamp_min(0)), e32, bnd, lit)
    assert bool((err <= allowed).all()), f"{tag}: worst err / (bound + half ulp) = {worst:.4f}"


class Zone:
    """n fp32 values between two sentinel-filled guard bands (the red-zone idea of test_gpu_elementwise.Buf for flat fp32 outputs)"""

    def __init__(self, n, guard=64):
        self.n, self.g = n, guard
        self.raw = torch.full((n + 2 * guard,), SENT[F32], dtype=torch.int32, device="cuda")
        self.ptr = self.raw.data_ptr() + 4 * guard

    def vals(self):
        return self.raw[self.g:self.g + self.n].view(torch.float32).cpu().double()

    def guards_intact(self):
        return bool((self.raw[:self.g] == SENT[F32]).all()) and bool((self.raw[self.g + self.n:] == SENT[F32]).all())

    def untouched(self):
        return bool((self.raw == SENT[F32]).all())


# ================================================================================================ YOLO head
class YoloCase:
    """one head: logits [B, A(5+C), Gh, Gw] as the dtype stores them, targets, anchors of the head with this stride"""

    def __init__(self, B, C, Gh, Gw, T, dt, stride, seed, min_real=1):
        g = torch.Generator().manual_seed(seed)
        self.B, self.C, self.Gh, self.Gw, self.T, self.dt, self.stride, self.A = B, C, Gh, Gw, T, dt, stride, 3
        self.attrs, self.ch = 5 + C, 3 * (5 + C)
        self.anchors_px = hr.yolo_anchors(stride)
        self.cfg_h = stride * Gh                                   # the layer derives its stride from the grid HEIGHT (models.py:145)
        self.sample = rnd(dt, (torch.randn(B, self.ch, Gh, Gw, generator=g) * 2).clamp(-8, 8))
        self.targets = hr.yolo_targets(B, T, g, cls_hi=max(1, min(C, 3)), min_real=min_real)
        self.key = (B, C, Gh, Gw, T, dt, stride, seed)

    def geo(self):
        return (self.B, self.T, self.A, self.C, self.Gh, self.Gw) + HYPER

    def live(self, Cpad):
        m = torch.zeros(Cpad, dtype=torch.bool)
        for an in range(self.A):
            m[an * self.attrs:an * self.attrs + 5] = True
        return m

    def refs(self, layer=hr.yo.yolo_layer):
        """(loss, parts, dsample, eval) in float64 and in float32, computed once per case"""
        k = self.key + (layer.__name__,)
        if k not in _REFS:
            out = []
            for dtype in (F64, torch.float32):
                loss, parts, ds = hr.yolo_train(self.sample, self.anchors_px, self.C, self.cfg_h, self.targets, dtype, layer=layer)
                out.append((loss, parts, ds, hr.yolo_eval(self.sample, self.anchors_px, self.C, self.cfg_h, dtype)))
            _REFS[k] = out
        return _REFS[k]

    def masks(self):
        return hr.yolo_masks(self.targets, self.anchors_px, self.C, self.Gh, self.Gw, self.stride)


def nhwc(case, ldc):
    """device NHWC logits, channel stride ldc, NaN in the pad channels (the kernels must not read them)"""
    t = torch.full((case.B, case.Gh, case.Gw, ldc), float("nan"))
    t[..., :case.ch] = case.sample.permute(0, 2, 3, 1)
    return t.to(TD[case.dt]).cuda()


def head_counts(ws, B, A, Gh, Gw):
    """the eight fp64 accumulators behind the int section of a head workspace (layout: mdcv_yolo_head_workspace_bytes)"""
    ints = B * A * Gh * Gw + Gh * Gw + 2
    ints = (ints + 1) & ~1
    return ws[ints * 4:ints * 4 + 64].view(torch.float64).cpu()


def run_train(case, Cpad, ldc=None, ldd=None, gscale=None, out7=None, grad=True, lg=None):
    """mdcv_yolo_head_train -> out7 (device fp32[7], accumulated into), dlogits Buf (or None), workspace, logits"""
    L = _lib.lib()
    ldc, ldd = ldc or Cpad, ldd or Cpad
    lg = nhwc(case, ldc) if lg is None else lg
    tg = case.targets.cuda()
    an = hr.scaled_anchors(case.anchors_px, case.stride).cuda()
    ws = torch.empty(int(L.yolo_head_workspace_bytes(case.B, case.A, case.Gh, case.Gw)), dtype=torch.uint8, device="cuda")
    out7 = torch.zeros(7, device="cuda") if out7 is None else out7
    dl = Buf(case.dt, case.B * case.Gh * case.Gw, Cpad, ld=ldd, tail=3) if grad else None
    gs = torch.tensor([gscale], device="cuda") if gscale is not None else None
    L.check(L.yolo_head_train(case.dt, lg.data_ptr(), ldc, dl.ptr if grad else None, ldd, Cpad, tg.data_ptr(), an.data_ptr(), *case.geo(),
                              ws.data_ptr(), out7.data_ptr(), P(gs), st()), "yolo_head_train")
    sync()
    return out7, dl, ws, (lg, tg, an)


def dl_nchw(case, dl):
    M = case.B * case.Gh * case.Gw
    return dl.rows(0, M)[:, :case.ch].view(case.B, case.Gh, case.Gw, case.ch).permute(0, 3, 1, 2)


def check_train(tag, case, out7, dl, Cpad, refs=None, e32_free=False):
    (loss, parts, ds, _), (loss32, parts32, ds32, _) = refs or case.refs()
    o = out7.cpu().double()
    none = lambda t: None if e32_free else t        # noqa: E731
    compare(f"{tag} loss", o[0], loss, none(loss32))
    for k, nm in enumerate(("x", "y", "w", "h", "obj", "noobj")):
        compare(f"{tag} part {nm}", o[1 + k], parts[k], none(parts32[k]))
    if dl is None:
        return
    got = dl_nchw(case, dl)
    compare(f"{tag} dlogits", got, ds, none(ds32), bf16_store=case.dt == BF16)
    assert torch.equal(got != 0, ds != 0), f"{tag}: gradient support differs from the reference"
    dl.assert_sentinel_intact()
    raw = dl.full.view(ITYPE[case.dt])[:dl.M, :Cpad]
    assert bool((raw[:, ~case.live(Cpad).cuda()] == 0).all()), f"{tag}: pad / class channels are not bit-zero"


def check_decode(tag, case, ldc, lg=None, refs=None, e32_free=False):
    """decode into a larger detection tensor at a row offset: values vs the reference, every other row untouched"""
    L = _lib.lib()
    lg = nhwc(case, ldc) if lg is None else lg
    an = hr.scaled_anchors(case.anchors_px, case.stride).cuda()
    rows, off, after = case.A * case.Gh * case.Gw, 5, 7
    total = off + rows + after
    out = torch.full((case.B, total, case.attrs), SENT[F32], dtype=torch.int32, device="cuda")
    L.check(L.yolo_head_decode(case.dt, lg.data_ptr(), ldc, an.data_ptr(), float(case.stride), case.B, case.A, case.C, case.Gh, case.Gw,
                               out.data_ptr(), total, off, st()), "yolo_head_decode")
    sync()
    assert bool((out[:, :off] == SENT[F32]).all()) and bool((out[:, off + rows:] == SENT[F32]).all()), f"{tag}: wrote outside its rows"
    got = out[:, off:off + rows].contiguous().view(torch.float32).cpu().double()
    r64, r32 = (refs or case.refs())[0][3], (refs or case.refs())[1][3]
    for nm, sl in (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("conf+cls", slice(4, None))):
        compare(f"{tag} decode {nm}", got[..., sl], r64[..., sl], None if e32_free else r32[..., sl])


PROD = [(4, 80, 13, 13, 16, 32, 256, F32), (4, 80, 13, 13, 16, 32, 256, BF16), (4, 1, 52, 52, 16, 8, 24, F32), (4, 1, 52, 52, 16, 8, 24, BF16),
        (2, 80, 19, 19, 30, 32, 256, BF16)]


@pytest.mark.parametrize("case", PROD, ids=lambda c: f"B{c[0]}-C{c[1]}-{c[2]}x{c[3]}-T{c[4]}-{'bf16' if c[7] else 'fp32'}")
def test_yolo_production_layouts(case):
    """The layouts the plans run: 255 channels in a 256-wide row, 18 in 24, Cpad = ldc = ldd; logits randn * 2 clipped to |z| <= 8.
    Loss, six parts, dlogits (16-pixel tile kernel), decode at a row offset.  MI355X: worst err / max(e32, 4 u scale) = 0.54; bf16 dlogits against the flat 2^-9 |ref|: 1.93 (8 allowed)."""
    B, C, Gh, Gw, T, stride, Cpad, dt = case
    c = YoloCase(B, C, Gh, Gw, T, dt, stride, seed=11 + Gh + C)
    tag = f"prod {C}c {Gh}x{Gw} {'bf16' if dt else 'fp32'}"
    out7, dl, _, (lg, _, _) = run_train(c, Cpad)
    check_train(tag, c, out7, dl, Cpad)
    check_decode(tag, c, Cpad, lg)


@DT
@pytest.mark.parametrize("B,Gh,Gw", [(3, 13, 19), (2, 19, 13)])
def test_yolo_non_square_grids(B, Gh, Gw, dt):
    """Gh != Gw, three different channel strides (ldc 32, Cpad 24, ldd 40), one target in the last column of the last row: every index
    expression of the four kernels mixes Gh and Gw.  MI355X: worst err / max(e32, 4 u scale) = 0.52; bf16 dlogits against the flat 2^-9 |ref|: 1.94 (8 allowed)."""
    c = YoloCase(B, 1, Gh, Gw, 6, dt, 32, seed=100 + Gh)
    c.targets[0, 0, 1:5] = torch.tensor([(Gw - 0.4) / Gw, (Gh - 0.3) / Gh, 0.2, 0.15])
    pos, _ = c.masks()
    assert bool(pos[0, :, Gh - 1, Gw - 1].any())
    tag = f"rect {Gh}x{Gw} {'bf16' if dt else 'fp32'}"
    out7, dl, _, (lg, _, _) = run_train(c, 24, ldc=32, ldd=40)
    check_train(tag, c, out7, dl, 24)
    check_decode(tag, c, 32, lg)


def test_yolo_loss_grid_stride_second_pass():
    """B A Gh Gw = 61 * 3 * 76 * 76 = 1 057 008 > 4096 * 256: the loss kernel's (and decode's) grid-stride loop runs a second pass over the
    last 8 432 cells, all of them in the last image, whose target sits there (anchor 2): a dropped tail changes nM, nN and every part.
    bf16, 18 channels in 24.  MI355X: worst err / max(e32, 4 u scale) = 0.36; bf16 dlogits against the flat 2^-9 |ref|: 1.86 (8 allowed)."""
    B, G = 61, 76
    c = YoloCase(B, 1, G, G, 4, BF16, 8, seed=61)
    c.targets[B - 1, 0] = torch.tensor([0.0, 0.97, 0.98, 0.25, 0.28])
    assert B * 3 * G * G > 4096 * 256 >= (B - 1) * 3 * G * G + G * G     # the tail holds the whole anchor-2 plane of the last image
    pos, neg = c.masks()
    assert bool(pos[B - 1, 2, G - 2:, :].any())                     # a positive cell inside the second pass
    out7, dl, ws, (lg, _, _) = run_train(c, 24)
    acc = head_counts(ws, B, 3, G, G)
    assert (float(acc[6]), float(acc[7])) == (float(pos.sum()), float(neg.sum()))
    check_train("stride2 61x76x76 bf16", c, out7, dl, 24)
    check_decode("stride2 61x76x76 bf16", c, 24, lg)


@DT
def test_yolo_collisions_and_batch_wide_ignore(dt):
    """Two rows of image 1 fall into one cell with one best anchor: the later row owns the cell.  Row 0 of image 0 has IoU > thresh with
    anchor 0 but anchor 1 as its best: cell (6, 5) leaves the no-object sum of EVERY image and anchor (utils.py:244-255).  nM and nN of
    the workspace equal the oracle's mask counts exactly; loss and gradients follow.  MI355X: worst err / max(e32, 4 u scale) = 0.54; bf16 dlogits against the flat 2^-9 |ref|: 1.68 (8 allowed)."""
    c = YoloCase(3, 1, 13, 13, 2, dt, 32, seed=5)                  # T = 2: a padding row behind the pair would repeat row 0 and own the cell
    t = torch.zeros(3, 2, 5)
    t[0, 0] = torch.tensor([0, 5.3 / 13, 6.6 / 13, 4.2 / 13, 4.5 / 13])
    t[0, 1] = torch.tensor([0, 2.4 / 13, 9.7 / 13, 1.5 / 13, 2.0 / 13])
    t[1, 0] = torch.tensor([0, 8.2 / 13, 3.3 / 13, 0.10, 0.10])
    t[1, 1] = torch.tensor([0, 8.7 / 13, 3.6 / 13, 0.11, 0.09])
    t[2, 0] = torch.tensor([0, 0.2, 0.8, 0.1, 0.2])
    c.targets = t
    sa = hr.scaled_anchors(c.anchors_px, 32)
    m, cm, tx = hr.yo.build_targets(t, sa, 3, 1, 13, 13, 0.5)[:3]
    assert int(m[0, :, 6, 5].argmax()) == 1 and int(m[0, :, 6, 5].sum()) == 1            # best anchor 1 ...
    assert int(cm[:, :, 6, 5].sum()) == 1                                                 # ... and the cell ignored everywhere else
    assert int(m[1, :, 3, 8].sum()) == 1 and float(tx[1, :, 3, 8].max()) == float(t[1, 1, 1] * 13 - 8)   # row 1 overwrote row 0
    pos, neg = c.masks()
    out7, dl, ws, _ = run_train(c, 24)
    acc = head_counts(ws, 3, 3, 13, 13)
    assert (float(acc[6]), float(acc[7])) == (float(pos.sum()), float(neg.sum()))
    check_train(f"collide {'bf16' if dt else 'fp32'}", c, out7, dl, 24)


@DT
def test_yolo_three_heads_accumulate_gscale_and_split_grad(dt):
    """out7 accumulates: three heads (13, 26, 52) into one out7 = the sum of three oracle results.  *gscale = 0.25 scales dlogits exactly
    (a power of two: 0.25 g rounds as g does).  mdcv_yolo_head_grad after train(dlogits = NULL) gives the one-call gradients bit for
    bit.  MI355X: worst err / max(e32, 4 u scale) = 0.39 (8 allowed)."""
    L = _lib.lib()
    heads = [YoloCase(2, 1, G, G, 6, dt, s, seed=77) for G, s in ((13, 32), (26, 16), (52, 8))]
    out7 = torch.zeros(7, device="cuda")
    tot64, tot32 = torch.zeros(7, dtype=F64), torch.zeros(7, dtype=torch.float32)
    for c in heads:
        out7, dl, _, _ = run_train(c, 24, out7=out7)
        (l64, p64, _, _), (l32, p32, _, _) = c.refs()
        tot64 += torch.cat([l64.view(1), p64])
        tot32 += torch.cat([l32.view(1), p32]).float()
    o = out7.cpu().double()
    for k, nm in enumerate(("loss", "x", "y", "w", "h", "obj", "noobj")):
        compare(f"3 heads {nm} {'bf16' if dt else 'fp32'}", o[k], tot64[k], tot32[k].double())
    c = heads[1]
    _, d1, _, _ = run_train(c, 24)
    _, dq, _, _ = run_train(c, 24, gscale=0.25)
    M = c.B * c.Gh * c.Gw
    assert torch.equal(dq.rows(0, M), 0.25 * d1.rows(0, M))
    _, _, ws, (lg, tg, an) = run_train(c, 24, grad=False)
    d2 = Buf(dt, M, 24, tail=3)
    L.check(L.yolo_head_grad(dt, lg.data_ptr(), 24, d2.ptr, 24, 24, tg.data_ptr(), an.data_ptr(), *c.geo(), ws.data_ptr(), None, st()))
    sync()
    assert torch.equal(d2.full.view(ITYPE[dt]), d1.full.view(ITYPE[dt]))


@DT
def test_yolo_saturated_logits(dt):
    """Objectness +30 / -30 and x / y logits +30 / -30 in a positive and in a no-object cell, objectness -95 in a positive cell: fp32
    sigmoid rounds to 1 (log(1 - p) clamps at -100, p (1 - p) = 0 takes the 1e-12 clamp of BCELoss.backward) and exp(95) overflows.
    Reference: the fp32 restatement with nn.BCELoss (head_refs.yolo_layer_bce; the oracle's clamp(log()) has a NaN backward here) - both
    sides are fp32, so the bound is 8 * 4 u scale.  sigmoid(-95) = 5.5e-42 is a denormal and BCE = 95; 1 / (1 + expf(95)) = 1 / inf = 0
    gave loss 100 and a zero gradient there until sigmoidf_ returned expf(x) where expf(-x) overflows.  MI355X: worst err / max(e32, 4 u scale) = 0.67 after the change; before it the loss was off by 5.56e-2 (0.1 * (100 - 95) / 9 positives) against a bound of 7.9e-5 (8 allowed)."""
    c = YoloCase(2, 1, 13, 13, 6, dt, 32, seed=30, min_real=4)
    pos, neg = c.masks()
    pc, nc = pos.nonzero().tolist(), neg.nonzero().tolist()
    assert len(pc) >= 3
    s = c.sample.view(2, 3, 6, 13, 13)
    (b, a, j, i) = pc[0]; s[b, a, 4, j, i] = 30.0; s[b, a, 0, j, i] = 30.0; s[b, a, 1, j, i] = -30.0      # noqa: E702
    (b, a, j, i) = pc[1]; s[b, a, 4, j, i] = -30.0; s[b, a, 0, j, i] = -30.0; s[b, a, 1, j, i] = 30.0     # noqa: E702
    (b, a, j, i) = pc[2]; s[b, a, 4, j, i] = -95.0                                                        # noqa: E702
    (b, a, j, i) = nc[0]; s[b, a, 4, j, i] = 30.0; s[b, a, 0, j, i] = 30.0; s[b, a, 1, j, i] = -30.0      # noqa: E702
    (b, a, j, i) = nc[7]; s[b, a, 4, j, i] = -30.0; s[b, a, 0, j, i] = -30.0; s[b, a, 1, j, i] = 30.0     # noqa: E702
    assert torch.equal(rnd(dt, c.sample), c.sample)
    loss, parts, ds = hr.yolo_train(c.sample, c.anchors_px, 1, c.cfg_h, c.targets, torch.float32, layer=hr.yolo_layer_bce)
    ev = hr.yolo_eval(c.sample, c.anchors_px, 1, c.cfg_h, torch.float32)
    assert bool(torch.isfinite(ds).all()) and 94.9 < float(-torch.log(hr.stable_sigmoid(torch.tensor(-95.0)))) < 95.1
    refs = [(loss, parts, ds, ev)] * 2
    tag = f"saturated {'bf16' if dt else 'fp32'}"
    out7, dl, _, (lg, _, _) = run_train(c, 24)
    check_train(tag, c, out7, dl, 24, refs=refs, e32_free=True)
    check_decode(tag, c, 24, lg, refs=refs, e32_free=True)
    # the planted cells element by element: tiny gradients that the bound relative to the largest gradient would not see.  Both sides
    # are fp32 products of a handful of factors, each a few ulp off (expf): 64 u relative
    got = dl_nchw(c, dl).view(2, 3, 6, 13, 13)
    want = ds.view(2, 3, 6, 13, 13)
    for (b, a, j, i) in (pc[0], pc[1], nc[0], nc[7]):
        g, w = got[b, a, [0, 1, 4], j, i], want[b, a, [0, 1, 4], j, i]                 # the three sigmoid channels
        extra = hr.half_ulp_bf16(w.abs()) if dt == BF16 else 0.0
        assert bool(((g - w).abs() <= 64 * hr.U * w.abs() + extra).all()), (b, a, j, i, g.tolist(), w.tolist())


def test_yolo_grad_scalar_kernel_when_the_tile_does_not_fit():
    """C = 200, fp32: Cpad = 616 is a whole number of 16-byte vectors and the base is aligned, but 16 pixels x 616 channels x 4 B = 39 424 B
    exceeds the tile's 32 KiB: the launcher takes the per-element kernel on SIZE.  Against float64 like the others.  MI355X: worst err / max(e32, 4 u scale) = 1.32 (8 allowed)."""
    c = YoloCase(1, 200, 7, 7, 4, F32, 32, seed=200)
    Cpad = 616
    assert c.ch <= Cpad and Cpad % 4 == 0 and 16 * Cpad * 4 > 32768
    out7, dl, _, (lg, _, _) = run_train(c, Cpad)
    assert dl.ptr % 16 == 0
    check_train("fallback C200 7x7 fp32", c, out7, dl, Cpad)
    check_decode("fallback C200 7x7 fp32", c, Cpad, lg)


# ================================================================================================ key-point head
def kp_logits(B, K, H, W, dt, seed, scale=4.0):
    g = torch.Generator().manual_seed(seed)
    return rnd(dt, torch.randn(B, K, H, W, generator=g) * scale)


def kp_nhwc(z, ldc, dt):
    B, K, H, W = z.shape
    t = torch.full((B, H, W, ldc), float("nan"))
    t[..., :K] = z.permute(0, 2, 3, 1)
    return t.to(TD[dt]).cuda()


def run_softargmax(z, ldc, dt):
    L = _lib.lib()
    B, K, H, W = z.shape
    lg = kp_nhwc(z, ldc, dt)
    hm, pts = Zone(B * K * H * W), Zone(B * K * 2)
    L.check(L.softargmax_fwd(dt, lg.data_ptr(), ldc, B, K, H, W, hm.ptr, pts.ptr, st()), "softargmax_fwd")
    sync()
    assert hm.guards_intact() and pts.guards_intact()
    return hm.vals().view(B, K, H, W), pts.vals().view(B, K, 2)


def check_softargmax(tag, z, ldc, dt):
    hm, pts = run_softargmax(z, ldc, dt)
    h64, p64 = hr.softargmax(z, F64)
    h32, p32 = hr.softargmax(z, torch.float32)
    compare(f"{tag} hm", hm, h64, h32.double())
    compare(f"{tag} pts", pts, p64, p32.double())
    one = torch.ones(z.shape[0], z.shape[1], dtype=F64)
    compare(f"{tag} sum(hm)", hm.sum((2, 3)), one, one + (h32.double().sum((2, 3)) - h64.sum((2, 3))))


SOFTARGMAX = [(3, 7, 80, 80, 8), (2, 5, 9, 31, 16), (1, 1, 1, 1, 8)]


@DT
@pytest.mark.parametrize("case", SOFTARGMAX, ids=lambda c: "x".join(map(str, c)))
def test_softargmax_fwd(case, dt):
    """Flat softmax over H W + expected x / y, NHWC logits (randn * 4) with NaN in the pad channels K..ldc-1: the production map, an odd
    H != W map with K = 5 in ldc = 16, and the 1 x 1 map.  Heat-map, points, and every map summing to 1.  MI355X: worst err / max(e32, 4 u scale) = 0.66 (8 allowed)."""
    B, K, H, W, ldc = case
    check_softargmax(f"softargmax {B}x{K}x{H}x{W} {'bf16' if dt else 'fp32'}", kp_logits(B, K, H, W, dt, seed=H * W + K), ldc, dt)


@pytest.mark.parametrize("shift", [60.0, 100.0, -100.0])
def test_softargmax_fwd_subtracts_the_maximum(shift):
    """A map whose logits are all shifted by +60 must give the same heat-map as the float64 softmax of the shifted logits; +100 / -100
    are past expf's fp32 range in either direction, so exp(z) without the maximum subtracted is inf / 0 there.  MI355X: worst err / max(e32, 4 u scale) = 0.28 (8 allowed)."""
    z = kp_logits(3, 7, 80, 80, F32, seed=6407)
    z[1, 3] += shift
    check_softargmax(f"softargmax shift {shift:+.0f}", z, 8, F32)


def test_softargmax_fwd_lds_guard():
    """The kernel holds H W floats of dynamic LDS beside 32 static bytes (red[8]).  The launcher accepts H W * 4 <= 64 KiB, at most
    65 568 B of a workgroup's 160 KiB on gfx950, so every accepted map can launch and the guard stands as it is.  One row above the
    limit (129 x 128) is refused with MDCV_EARG and nothing is written; 128 x 127 (65 024 B) runs and matches float64.
    MI355X: worst err / max(e32, 4 u scale) = 0.11 (8 allowed)."""
    L = _lib.lib()
    H, W = 129, 128
    assert (H - 1) * W * 4 <= 64 * 1024 < H * W * 4
    lg = torch.zeros(H * W, 8, device="cuda")
    hm, pts = Zone(H * W), Zone(2)
    for dt in (F32, BF16):
        assert L.softargmax_fwd(dt, lg.data_ptr(), 8, 1, 1, H, W, hm.ptr, pts.ptr, st()) == EARG
    sync()
    assert hm.untouched() and pts.untouched()
    check_softargmax("softargmax 128x127", kp_logits(1, 2, 128, 127, F32, seed=128127), 8, F32)


@DT
@pytest.mark.parametrize("ldd", [8, 16])
@pytest.mark.parametrize("B,K,H,W", [(3, 7, 80, 80), (2, 5, 9, 31)])
def test_softargmax_bwd(B, K, H, W, ldd, dt):
    """dlogits of sum(pts dpts) + sum(hm dhm) with dpts only, dhm only (softmax_dot_kernel) and both, against float64 autograd through
    softmax + soft-argmax from the logits.  Channels K..7 are bit-zero, channels 8..ldd-1 and the rows behind keep their sentinel.
    MI355X: worst err / max(e32, 4 u scale) = 0.34; bf16 dlogits against the flat 2^-9 |ref|: 1.95 (8 allowed)."""
    L = _lib.lib()
    z = kp_logits(B, K, H, W, F32, seed=B * 1000 + W)
    g = torch.Generator().manual_seed(ldd + K)
    dpts, dhm = torch.randn(B, K, 2, generator=g), torch.randn(B, K, H, W, generator=g)
    h64, p64 = hr.softargmax(z, F64)
    hm_d, pts_d = h64.float().cuda(), p64.float().cuda()
    sdot = torch.empty(B * K, device="cuda")
    for mode, (dp, dh) in (("dpts", (dpts, None)), ("dhm", (None, dhm)), ("both", (dpts, dhm))):
        out = Buf(dt, B * H * W, 8, ld=ldd, tail=2)
        dp_d, dh_d = (dp.cuda() if dp is not None else None), (dh.cuda() if dh is not None else None)
        L.check(L.softargmax_bwd(dt, hm_d.data_ptr(), pts_d.data_ptr(), P(dp_d), P(dh_d), sdot.data_ptr(), B, K, H, W, out.ptr, ldd, st()))
        sync()
        out.assert_sentinel_intact()
        assert bool((out.full.view(ITYPE[dt])[:out.M, K:8] == 0).all()), "pad channels K..7 are not bit-zero"
        got = out.rows(0, out.M)[:, :K].view(B, H, W, K).permute(0, 3, 1, 2)
        compare(f"softargmax_bwd {B}x{K}x{H}x{W} ldd{ldd} {mode} {'bf16' if dt else 'fp32'}", got, hr.softargmax_bwd(z, dp, dh, F64),
                hr.softargmax_bwd(z, dp, dh, torch.float32), bf16_store=dt == BF16)


def kp_loss_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    pts, tpts = torch.rand(B, 7, 2, generator=g), torch.rand(B, 7, 2, generator=g) * (1 - 1.0 / max(H, W))
    hm = torch.softmax(torch.randn(B, 7, H * W, generator=g) * 2, -1).view(B, 7, H, W)
    thm = torch.softmax(torch.randn(B, 7, H * W, generator=g) * 3, -1).view(B, 7, H, W)
    return hm, pts, thm, tpts


def run_cross_ratio(hm, pts, thm, tpts, lt, geo, gscale, acc, want_dpts=True, want_dhm=True, gam=(0.05, 0.07)):
    L = _lib.lib()
    B, _, H, W = hm.shape
    dev = [t.cuda() for t in (hm, pts, thm, tpts)]
    gs = torch.tensor(gscale, device="cuda") if gscale is not None else None
    out3, dpts = Zone(3), Zone(B * 14)
    dhm = Zone(B * 7 * H * W) if (lt == 1 and want_dhm) else None
    L.check(L.cross_ratio_loss(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), B, H, W, lt, int(geo), gam[0], gam[1],
                               P(acc), P(gs), out3.ptr, dpts.ptr if want_dpts else None, dhm.ptr if dhm else None, st()), "cross_ratio_loss")
    sync()
    assert out3.guards_intact() and dpts.guards_intact() and (dhm is None or dhm.guards_intact())
    if not want_dpts:
        assert dpts.untouched()
    return out3.vals(), dpts.vals().view(B, 7, 2), (dhm.vals().view(B, 7, H, W) if dhm else None)


def check_cross_ratio(tag, inp, lt, geo, gscale, acc, want_dpts=True):
    hm, pts, thm, tpts = inp
    out3, dpts, dhm = run_cross_ratio(hm, pts, thm, tpts, lt, geo, gscale, acc, want_dpts)
    o64, d64 = hr.cross_ratio(hm, pts, thm, tpts, hr.LOSS_TYPES[lt], geo, 0.05, 0.07, gscale, F64, want_dpts)
    o32, d32 = hr.cross_ratio(hm, pts, thm, tpts, hr.LOSS_TYPES[lt], geo, 0.05, 0.07, gscale, torch.float32, want_dpts)
    for k, nm in enumerate(("loc", "geo", "total")):
        compare(f"{tag} {nm}", out3[k], o64[k], o32[k])
    if want_dpts:
        compare(f"{tag} dpts", dpts, d64, d32)
    if dhm is not None:
        up = 1.0 if gscale is None else gscale[0]
        B = hm.shape[0]
        r64 = 2.0 * (hm.double() - thm.double()) / B * up
        r32 = (2.0 * (hm - thm) / B * up).double()
        compare(f"{tag} dhm", dhm, r64, r32)
    return out3, dpts, dhm


@pytest.mark.parametrize("lt", [0, 1, 2], ids=hr.LOSS_TYPES)
@pytest.mark.parametrize("B", [1, 2, 256, 257, 600])
def test_cross_ratio_loss(B, lt):
    """B on both sides of the single block's `i += 256` loop, every loss type, geo on / off, gamma = (0.05, 0.07), gscale NULL and
    (0.5, 2.0): out3 = (location, geo, total) and dpts against the float64 oracle; for l2_heatmap (5 x 4 maps, H != W) dhm too.
    MI355X: worst err / max(e32, 4 u scale) = 0.77 (8 allowed)."""
    inp = kp_loss_inputs(B, 5, 4, seed=B * 3 + lt)
    acc = torch.zeros(1, dtype=F64, device="cuda") if lt == 1 else None
    for geo in (False, True):
        for gscale in (None, (0.5, 2.0)):
            check_cross_ratio(f"cross_ratio B{B} {hr.LOSS_TYPES[lt]} geo{int(geo)} gs{int(gscale is not None)}", inp, lt, geo, gscale, acc)


@pytest.mark.parametrize("B", [2, 47])
def test_cross_ratio_heatmap_loss_at_80x80(B):
    """l2_heatmap on 80 x 80 maps.  B = 47 is the smallest batch with B 7 H W = 2 105 600 > 2048 * 1024: hm_l2_kernel's grid-stride loop
    runs a second pass.  The call runs twice on ONE acc_ws (the single block resets it after reading): identical results.
    MI355X: worst err / max(e32, 4 u scale) = 0.92 (8 allowed)."""
    assert B != 47 or (B * 7 * 6400 > 2048 * 1024 >= (B - 1) * 7 * 6400)
    inp = kp_loss_inputs(B, 80, 80, seed=80 + B)
    acc = torch.zeros(1, dtype=F64, device="cuda")
    first = check_cross_ratio(f"cross_ratio hm80 B{B} first", inp, 1, True, (0.5, 2.0), acc)
    again = check_cross_ratio(f"cross_ratio hm80 B{B} again", inp, 1, True, (0.5, 2.0), acc)
    assert float(acc.cpu()) == 0.0
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_cross_ratio_coincident_key_points_forward():
    """Two coincident key points (P3 = P1 in one image): F.normalize's 1e-12 clamp makes that unit vector zero.  Forward only (dpts = NULL
    writes nothing); the value matches the oracle.  MI355X: worst err / max(e32, 4 u scale) = 0.38 (8 allowed)."""
    hm, pts, thm, tpts = kp_loss_inputs(5, 5, 4, seed=31)
    pts[2, 3] = pts[2, 1]
    for lt in (0, 2):
        check_cross_ratio(f"cross_ratio coincident {hr.LOSS_TYPES[lt]}", (hm, pts, thm, tpts), lt, True, None, None, want_dpts=False)


def test_cross_ratio_refuses_bad_arguments():
    """unknown loss_type; l2_heatmap without acc_ws, without hm, without thm: MDCV_EARG and nothing written"""
    L = _lib.lib()
    hm, pts, thm, tpts = [t.cuda() for t in kp_loss_inputs(2, 5, 4, seed=1)]
    acc = torch.zeros(1, dtype=F64, device="cuda")
    out3, dpts, dhm = Zone(3), Zone(28), Zone(2 * 7 * 20)

    def call(hm_, thm_, lt, acc_):
        return L.cross_ratio_loss(P(hm_), pts.data_ptr(), P(thm_), tpts.data_ptr(), 2, 5, 4, lt, 1, 0.05, 0.07, P(acc_), None, out3.ptr, dpts.ptr,
                                  dhm.ptr, st())
    assert call(hm, thm, 3, acc) == EARG and call(hm, thm, -1, acc) == EARG
    assert call(hm, thm, 1, None) == EARG and call(None, thm, 1, acc) == EARG and call(hm, None, 1, acc) == EARG
    sync()
    assert out3.untouched() and dpts.untouched() and dhm.untouched() and float(acc.cpu()) == 0.0
