"""-m gpu: the layout, weight-pack, max-pool and nearest-upsample kernels (csrc/layout.hip, pack_weights.hip, pool_upsample.hip) through the
C ABI against the plain references of tests/helpers/datamove_refs.py, with `==` on bit patterns, in fp32 and bf16.

These kernels copy, take maxima and add a few numbers; nothing here needs a tolerance.  Gradients are integers with |d| <= 256 // n
(n = the most terms one pixel can receive: sc * sc for the upsample, ceil(k / s)^2 for a pool), so that every sum is a bf16 number.
Every NaN counts as one bit pattern (datamove_refs.bits): neither side promises a NaN's sign or payload.  tests/test_datamove_refs.py pins
the references, and the input generators used here, to torch.nn.functional on the CPU.

Every output is a channel slice of a wider buffer pre-filled with the bit pattern 0x5A5A... (Slice of tests/test_gpu_conv_exact.py) and
everything outside the slice must stay untouched; every input slice has junk in its neighbouring channels (1000 for pool inputs: it would
win every maximum).  idx, the dense [B, Ho, Wo, C] byte buffer between a pool's forward and backward, is compared itself, between guard bytes.

  what                      cases                                                  there for
  nchw_to_nhwc              LAYOUT_CASES                                           ldc > Cpad at a channel offset, Cpad > pad8(C), C = 1, C = 255
  nhwc_to_nchw              UNLAYOUT_CASES                                         out of a strided slice, C no multiple of 8, junk in the pad channels
  both                      1 x 61 (29) x 513 x 513, 1 x 9 x 513 x 513             the grid-stride loop wraps: more than 8192 x 256 vectors / elements
  upsample, both forms      UPS_CASES, 184 x 184 x 128 (64) x2                     concat slices, non-square, scale 1..4; forward wraps (backward does not)
  max-pool 2x2 / generic    POOL2_SHAPES, POOL_KS x POOL_KINDS                     odd sizes, padding that wins, asymmetric windows, stride > k, ties, -0.0, -inf
  max-pool 2x2              368 x 368 x 128 (64), strides 2 and 1                  backward wraps at both strides, forward at stride 1
  max-pool, NaN             pool_input("nan")                                      y NaN, idx the last NaN in scan order, dx routed there
  pack, single and batched  PACK_SHAPES                                            against pack_ref, sentinel-filled outputs, fp32 too, special values
  mutations                 last maximum, live pad channel, a vector moved over the wrap   the comparisons above can fail

Left out on purpose: tensors beyond 2^31 elements, and idx in a window of only -inf -- the kernels leave idx = 0 there, torch points at the
first element inside the image; y is asserted there, and dx wherever the two agree (always for the 2x2 forms, whose position 0 is never padding;
for the generic form those windows get a zero gradient, because with idx = 0 on a padding position the kernels route it nowhere)."""
import functools
import os
import struct
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import datamove_refs as R  # noqa: E402
import test_datamove_refs as H  # noqa: E402
from test_gpu_conv_exact import Slice, _fill_sentinel, _is_sentinel  # noqa: E402
from test_gpu_kernels import pad8, F32, BF16, TD, st  # noqa: E402
from mdcv import _lib  # noqa: E402

torch.set_num_threads(16)
DTS = pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
NINF = float("-inf")
GUARD = 64


def check_nhwc(s, want, what):
    """the slice == want ([B, H, W, Cp] of the element type, pad channels included) bit for bit, everything outside it untouched"""
    torch.cuda.synchronize()
    got = s.buf[..., s.off:s.off + s.Cp]
    want = want.cuda()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = R.bits(got) != R.bits(want)
    n = int(bad.sum())
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} elements differ, first at [b, h, w, c] = {i}: got {float(got[i])!r}, want {float(want[i])!r}")
    outside = torch.cat((s.buf[..., :s.off], s.buf[..., s.off + s.Cp:]), -1)
    assert bool(_is_sentinel(outside.contiguous()).all()), f"{what}: written outside the channel slice"


def check(s, want_nchw, what):
    check_nhwc(s, R.nhwc_of(want_nchw, s.Cp, s.dt), what)


def check_flat(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = R.bits(got) != R.bits(want) if got.is_floating_point() else got != want
    n = int(bad.sum())
    if n:
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {n} elements differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}")


def guarded(n, dtype):
    """n elements between two runs of GUARD sentinel elements"""
    raw = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
    if dtype == torch.uint8:
        raw.fill_(0xA5)
    else:
        _fill_sentinel(raw)
    return raw, raw[GUARD:GUARD + n]


def guards_ok(raw, n):
    g = torch.cat((raw[:GUARD], raw[GUARD + n:]))
    return bool((g == 0xA5).all()) if raw.dtype == torch.uint8 else bool(_is_sentinel(g).all())


def layout_input(B, C, H, W, seed=1):
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed * 7919 + C)) * 4
    sp = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, 3.4e38, -3.4e38, float("inf"), NINF, -0.0, 0.0, 2.0 ** -20])
    flat = x.view(-1)
    n = min(sp.numel(), flat.numel())
    flat[:n] = sp[:n]                                             # bf16 ties to even, values that round to +-inf, infinities, signed zeros
    flat[flat.numel() - n:] = sp[:n]
    return x


# ================================================================== layout

LAYOUT_CASES = [(2, 5, 7, 9, 8, 0, 0), (2, 5, 7, 9, 8, 8, 8), (2, 3, 5, 6, 32, 0, 0), (1, 3, 4, 5, 32, 16, 8), (2, 1, 6, 7, 8, 24, 0),
                (1, 255, 3, 5, 256, 0, 8), (3, 13, 5, 3, 24, 8, 16)]                     # B, C, H, W, Cpad, channel offset, channels behind
UNLAYOUT_CASES = [(2, 5, 7, 9, 8, 8), (1, 255, 3, 5, 0, 8), (2, 1, 4, 4, 24, 0), (3, 13, 5, 3, 8, 16), (2, 16, 3, 3, 0, 0)]   # B, C, H, W, offset, behind


def run_to_nhwc(dt, x, Cpad, off, extra):
    L = _lib.lib()
    B, C, Hh, W = x.shape
    s = Slice.out(dt, B, Hh, W, Cpad, off, extra)
    src = x.contiguous().cuda()
    L.check(L.nchw_to_nhwc(dt, src.data_ptr(), s.ptr, B, C, Hh, W, s.ld, Cpad, st()), "nchw_to_nhwc")
    return s


@DTS
@pytest.mark.parametrize("case", LAYOUT_CASES, ids=str)
def test_nchw_to_nhwc(case, dt):
    B, C, Hh, W, Cpad, off, extra = case
    x = layout_input(B, C, Hh, W)
    s = run_to_nhwc(dt, x, Cpad, off, extra)
    assert s.Cp == Cpad and s.ld == off + Cpad + extra
    check_nhwc(s, R.nhwc_of(x, Cpad, dt), f"nchw_to_nhwc {case}")


def run_to_nchw(dt, x, off, extra):
    """x (values of the element type) sits in a slice whose pad channels and neighbours hold junk; -> the raw fp32 output with its guards, n"""
    L = _lib.lib()
    B, C, Hh, W = x.shape
    s = Slice.of(dt, x, off, extra, junk=77.0)
    s.buf[..., off + C:off + s.Cp] = -55.0                         # the kernel reads C channels, not pad8(C)
    raw, dst = guarded(B * C * Hh * W, torch.float32)
    L.check(L.nhwc_to_nchw(dt, s.ptr, s.ld, dst.data_ptr(), B, C, Hh, W, st()), "nhwc_to_nchw")
    torch.cuda.synchronize()
    return raw, dst


@DTS
@pytest.mark.parametrize("case", UNLAYOUT_CASES, ids=str)
def test_nhwc_to_nchw(case, dt):
    B, C, Hh, W, off, extra = case
    x = R.rnd(layout_input(B, C, Hh, W, seed=2), dt)
    raw, dst = run_to_nchw(dt, x, off, extra)
    check_flat(dst.view(B, C, Hh, W), R.nchw_of(R.nhwc_of(x, pad8(C), dt), C), f"nhwc_to_nchw {case}")
    assert guards_ok(raw, B * C * Hh * W), "written outside the output"


@functools.lru_cache(maxsize=None)
def big_layout(dt):
    """1 x 61 (bf16) / 29 (fp32) x 513 x 513 -> Cpad 64 / 32: 513 * 513 * 8 = 2 105 352 vectors, 8 200 more than the 8192 x 256 threads of
    the capped grid, so the last 8 200 are written by threads on their second trip.  (input, expected NHWC), never modified."""
    C, Cpad = (61, 64) if dt == BF16 else (29, 32)
    x = layout_input(1, C, 513, 513, seed=3)
    return x, R.nhwc_of(x, Cpad, dt)


@DTS
def test_nchw_to_nhwc_wraps_the_grid(dt):
    x, want = big_layout(dt)
    assert want.numel() // (16 // want.element_size()) == 2105352 > 8192 * 256
    s = run_to_nhwc(dt, x, want.shape[-1], 8, 8)
    check_nhwc(s, want, "nchw_to_nhwc past the grid cap")


@DTS
def test_nhwc_to_nchw_wraps_the_grid(dt):
    B, C, Hh, W = 1, 9, 513, 513                                   # one thread per ELEMENT: 2 368 521 > 2 097 152
    assert B * C * Hh * W > 8192 * 256
    x = R.rnd(layout_input(B, C, Hh, W, seed=4), dt)
    raw, dst = run_to_nchw(dt, x, 8, 8)
    check_flat(dst.view(B, C, Hh, W), x, "nhwc_to_nchw past the grid cap")
    assert guards_ok(raw, B * C * Hh * W), "written outside the output"


@DTS
def test_layout_argument_errors(dt):
    """refused on the host before any launch: the output keeps its sentinel"""
    L = _lib.lib()
    x = torch.randn(1, 12, 3, 3).cuda()
    s = Slice.out(dt, 1, 3, 3, 16, 8, 8)
    for C, ldc, Cpad in [(12, 32, 8), (12, 32, 12), (12, 28, 16), (3, 32, 4)]:       # Cpad < C; Cpad, ldc no multiple of 8
        assert L.nchw_to_nhwc(dt, x.data_ptr(), s.ptr, 1, C, 3, 3, ldc, Cpad, st()) == -1, (C, ldc, Cpad)
    assert L.nchw_to_nhwc(2, x.data_ptr(), s.ptr, 1, 12, 3, 3, 32, 16, st()) == -1   # no such element type
    torch.cuda.synchronize()
    assert bool(_is_sentinel(s.buf).all())


# ================================================================== nearest upsample

def run_upsample(dt, x, sc, form, sliced=True):
    """forward into a concat slice (offset 8 of a wider buffer), from an input that is a slice itself"""
    L = _lib.lib()
    B, C, Hh, W = x.shape
    xs = Slice.of(dt, x, *((16, 8) if sliced else (0, 0)), junk=77.0)
    ys = Slice.out(dt, B, Hh * sc, W * sc, C, *((8, 16) if sliced else (0, 0)))
    if form == "2x":
        L.check(L.upsample2x_fwd(dt, xs.ptr, xs.ld, ys.ptr, ys.ld, B, Hh, W, C, st()), "upsample2x_fwd")
    else:
        L.check(L.upsample_fwd(dt, xs.ptr, xs.ld, ys.ptr, ys.ld, B, Hh, W, C, sc, st()), "upsample_fwd")
    return ys


def run_upsample_bwd(dt, dy, sc, form, Hh, W, sliced=True):
    """backward out of a concat slice"""
    L = _lib.lib()
    B, C = dy.shape[:2]
    dys = Slice.of(dt, dy, *((8, 16) if sliced else (0, 0)), junk=77.0)
    dxs = Slice.out(dt, B, Hh, W, C, *((16, 8) if sliced else (0, 0)))
    if form == "2x":
        L.check(L.upsample2x_bwd(dt, dys.ptr, dys.ld, dxs.ptr, dxs.ld, B, Hh, W, C, st()), "upsample2x_bwd")
    else:
        L.check(L.upsample_bwd(dt, dys.ptr, dys.ld, dxs.ptr, dxs.ld, B, Hh, W, C, sc, st()), "upsample_bwd")
    return dxs


@DTS
@pytest.mark.parametrize("sliced", [True, False], ids=["slices", "dense"])
@pytest.mark.parametrize("sc,Hh,W", H.UPS_CASES)
def test_upsample(sc, Hh, W, sliced, dt):
    B, C = 2, 24
    x = R.rnd(layout_input(B, C, Hh, W, seed=sc), dt)
    dy = H.int_grad((B, C, Hh * sc, W * sc), sc * sc, sc)
    want, dwant = R.upsample_ref(x, sc), R.upsample_bwd_ref(dy, sc).float()
    assert float(dwant.abs().max()) <= 256
    outs = {}
    for form in ("generic", "2x") if sc == 2 else ("generic",):
        ys = run_upsample(dt, x, sc, form, sliced)
        check(ys, want, f"upsample forward x{sc} {form}")
        outs[form] = ys.buf
        check(run_upsample_bwd(dt, dy, sc, form, Hh, W, sliced), dwant, f"upsample backward x{sc} {form}")
    if sc == 2:
        assert torch.equal(R.bits(outs["generic"]), R.bits(outs["2x"])), "upsample_fwd(2) and upsample2x_fwd differ"


@functools.lru_cache(maxsize=None)
def big_maps(dt):
    """184 x 184 and 368 x 368 maps of 128 (bf16) / 64 (fp32) channels = 16 vectors per pixel: 368 * 368 * 16 = 2 166 784 vectors wrap the
    capped grid, 184 * 184 * 16 = 541 696 do not.  Shared by the upsample and the 2x2 pool; never modified."""
    C = 128 if dt == BF16 else 64
    g = torch.Generator().manual_seed(11)
    small = torch.randn(1, C, 184, 184, generator=g).to(torch.bfloat16).float()
    large = torch.randn(1, C, 368, 368, generator=g).to(torch.bfloat16).float()
    gi = torch.randint(-64, 65, (1, C, 368, 368), generator=g).float()
    return small, large, gi


@DTS
@pytest.mark.parametrize("form", ["2x", "generic"])
def test_upsample_wraps_the_grid(form, dt):
    small, _, gi = big_maps(dt)
    C = small.shape[1]
    assert 368 * 368 * C // (16 // (2 if dt == BF16 else 4)) == 2166784 > 8192 * 256
    check(run_upsample(dt, small, 2, form), R.upsample_ref(small, 2), f"upsample forward past the grid cap, {form}")
    # the backward runs one thread per INPUT vector: 541 696 of them, no second trip; same shape for the record
    check(run_upsample_bwd(dt, gi, 2, form, 184, 184), R.upsample_bwd_ref(gi, 2).float(), f"upsample backward at the same shape, {form}")


# ================================================================== max-pool

def pool_ref(form, x, last_max=False):
    return R.maxpool2x2_ref(x, form[1], last_max) if form[0] == "2x2" else R.maxpool_ref(x, *form[1:], last_max)


def pool_geom(form):
    """k, stride, pad of the window arithmetic, most windows per pixel"""
    k, s, pad = (2, form[1], 0) if form[0] == "2x2" else form[1:]
    return k, s, pad, (-(-k // s)) ** 2


def pool_fwd(dt, form, x, sliced):
    """-> output slice, idx as [B, C, Ho, Wo] on the CPU, the device idx buffer"""
    L = _lib.lib()
    B, C, Hh, W = x.shape
    k, s, pad, _ = pool_geom(form)
    Ho, Wo = ((Hh // 2, W // 2) if s == 2 else (Hh, W)) if form[0] == "2x2" else (R.pool_out(Hh, k, s, pad), R.pool_out(W, k, s, pad))
    xs = Slice.of(dt, x, *((8, 8) if sliced else (0, 0)), junk=1000.0)
    ys = Slice.out(dt, B, Ho, Wo, C, *((16, 8) if sliced else (0, 0)))
    n = B * Ho * Wo * C
    raw, ib = guarded(n, torch.uint8)
    if form[0] == "2x2":
        L.check(L.maxpool2x2_fwd(dt, xs.ptr, xs.ld, ys.ptr, ys.ld, ib.data_ptr(), B, Hh, W, C, s, st()), "maxpool2x2_fwd")
    else:
        L.check(L.maxpool_fwd(dt, xs.ptr, xs.ld, ys.ptr, ys.ld, ib.data_ptr(), B, Hh, W, C, k, s, pad, st()), "maxpool_fwd")
    torch.cuda.synchronize()
    assert guards_ok(raw, n), "idx written outside its buffer"
    return ys, ib.view(B, Ho, Wo, C).permute(0, 3, 1, 2).contiguous().cpu(), ib


def pool_bwd(dt, form, dy, idx_dev, Hh, W, sliced):
    L = _lib.lib()
    B, C = dy.shape[:2]
    k, s, pad, _ = pool_geom(form)
    dys = Slice.of(dt, dy, *((16, 8) if sliced else (0, 0)), junk=77.0)
    dxs = Slice.out(dt, B, Hh, W, C, *((8, 8) if sliced else (0, 0)))
    if form[0] == "2x2":
        L.check(L.maxpool2x2_bwd(dt, dys.ptr, dys.ld, idx_dev.data_ptr(), dxs.ptr, dxs.ld, B, Hh, W, C, s, st()), "maxpool2x2_bwd")
    else:
        L.check(L.maxpool_bwd(dt, dys.ptr, dys.ld, idx_dev.data_ptr(), dxs.ptr, dxs.ld, B, Hh, W, C, k, s, pad, st()), "maxpool_bwd")
    return dxs


def check_idx(got, want, live, what):
    bad = (got != want) & live
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} idx elements differ, first at [b, c, oh, ow] = {i}: got {int(got[i])}, want {int(want[i])}")


def run_pool(dt, form, x, sliced, what, made_up_idx=True):
    """forward (y, idx), backward with that idx, backward with an idx made here"""
    B, C, Hh, W = x.shape
    k, s, pad, n = pool_geom(form)
    assert torch.equal(R.bits(R.rnd(x, dt)), R.bits(x)), "the input must hold numbers of the element type"
    y, idx = pool_ref(form, x)
    ys, got_idx, idx_dev = pool_fwd(dt, form, x, sliced)
    check(ys, y, f"{what}: y")
    live = y != NINF                                               # a window of only -inf: idx is not asserted (module docstring)
    check_idx(got_idx, idx, live, what)
    dy = H.int_grad(y.shape, n, k * 10 + s)
    if form[0] != "2x2":
        dy = dy * live
    dx = R.maxpool_bwd_ref(dy, idx, Hh, W, k, s, pad).float()
    assert float(dx.abs().max()) <= 256
    check(pool_bwd(dt, form, dy, idx_dev, Hh, W, sliced), dx, f"{what}: dx")
    if not made_up_idx:
        return
    # every legal position, 4 (2x2: the padding won) and a value no position equals: those gradients go nowhere
    g = torch.Generator().manual_seed(k * 100 + s)
    pick = torch.randint(0, k * k + 2, y.shape, generator=g)
    pick[pick == k * k] = 4 if form[0] == "2x2" else R.NONE
    pick[pick == k * k + 1] = R.NONE
    pick = pick.to(torch.uint8)
    dy2 = H.int_grad(y.shape, n, k * 10 + s + 1)
    dev = pick.permute(0, 2, 3, 1).contiguous().cuda()
    check(pool_bwd(dt, form, dy2, dev, Hh, W, sliced), R.maxpool_bwd_ref(dy2, pick, Hh, W, k, s, pad).float(), f"{what}: dx of a made-up idx")


POOL_KINDS = [k for k in H.POOL_KINDS if k != "nan"]               # (NaN: test_maxpool_nan)


@DTS
@pytest.mark.parametrize("stride,Hh,W", H.POOL2_SHAPES)
def test_maxpool2x2(stride, Hh, W, dt):
    for kind in POOL_KINDS:
        x = H.pool_input(kind, 2, 16, Hh, W)
        for sliced in (True, False):
            run_pool(dt, ("2x2", stride), x, sliced, f"maxpool2x2 stride {stride} {Hh}x{W} {kind} {'slices' if sliced else 'dense'}")


@DTS
@pytest.mark.parametrize("k,s", H.POOL_KS)
def test_maxpool_generic(k, s, dt):
    Hh, W = H.POOL_HW
    for kind in POOL_KINDS:
        x = H.pool_input(kind, 2, 16, Hh, W)
        for sliced in (True, False):
            run_pool(dt, ("gen", k, s, (k - 1) // 2), x, sliced, f"maxpool k {k} s {s} {kind} {'slices' if sliced else 'dense'}")


def test_generic_2x2_is_the_2x2_kernel():
    """the two forms of the stride-2 2x2 pool write the same y and idx"""
    x = H.pool_input("plateau", 2, 16, 13, 13)
    a, ia, _ = pool_fwd(BF16, ("2x2", 2), x, True)
    b, ib, _ = pool_fwd(BF16, ("gen", 2, 2, 0), x, True)
    assert torch.equal(R.bits(a.buf), R.bits(b.buf)) and torch.equal(ia, ib)


NAN_FORMS = [("2x2", 2), ("2x2", 1), ("gen", 2, 2, 0), ("gen", 3, 1, 1), ("gen", 3, 2, 1), ("gen", 4, 2, 1)]


@DTS
@pytest.mark.parametrize("form", NAN_FORMS, ids=str)
def test_maxpool_nan(form, dt):
    """torch's rule `v > best || isnan(v)`: a window that holds a NaN outputs NaN, idx is its LAST NaN in scan order and the gradient goes
    there; windows without one are unchanged.  pool_input("nan"): by 2x2 block one NaN at each position, two NaN, only NaN, none; NaN on
    the last row and column, which at stride 1 meet the zero padding.

    With `if (x > best)` (the kernels before this test existed) a NaN never wins: the maximum of the other values comes out, -inf from a
    window of only NaN.  That build fails all twelve cases here on an MI355X, for example
        AssertionError: maxpool ('2x2', 2) 13x13 NaN slices: y: 1008 elements differ, first at [b, h, w, c] = (0, 0, 0, 0): got 1.2265625, want nan
    (1008 = 2 images x 16 channels x 36 windows x 7 / 8 patterns), while the finite cases of test_maxpool2x2 pass on both builds."""
    Hh, W = (13, 13) if form[0] == "2x2" else H.POOL_HW
    x = H.pool_input("nan", 2, 16, Hh, W)
    y, idx = pool_ref(form, x)
    assert bool(torch.isnan(y).any())
    if form in (("2x2", 2), ("gen", 2, 2, 0)):                     # the patterns, spelled out (the last row / column of an odd size is in no window)
        code = H.nan_codes(16, Hh, W).expand(2, -1, -1, -1)
        assert torch.equal(torch.isnan(y), code < 7) and torch.equal(idx[code < 7], H.NAN_IDX[code[code < 7]].to(torch.uint8))
    if form == ("2x2", 1):
        assert bool(torch.isnan(y[:, :, Hh - 1, W - 1]).all()) and bool((idx[:, :, Hh - 1, W - 1] == 0).all())
    for sliced in (True, False):
        run_pool(dt, form, x, sliced, f"maxpool {form} {Hh}x{W} NaN {'slices' if sliced else 'dense'}", made_up_idx=False)


@DTS
@pytest.mark.parametrize("stride", [2, 1])
def test_maxpool2x2_wraps_the_grid(stride, dt):
    """368 x 368 x 128 (64): the backward has 2 166 784 vectors at both strides and wraps; the forward wraps at stride 1 (same count) and
    does not at stride 2 (541 696)."""
    _, large, gi = big_maps(dt)
    form = ("2x2", stride)
    y, idx = pool_ref(form, large)
    ys, got_idx, idx_dev = pool_fwd(dt, form, large, True)
    check(ys, y, f"maxpool2x2 stride {stride} at 368 x 368: y")
    check_idx(got_idx, idx, torch.ones_like(idx, dtype=torch.bool), f"maxpool2x2 stride {stride} at 368 x 368")
    dy = gi[:, :, :y.shape[2], :y.shape[3]].contiguous()           # |d| <= 64: four terms at stride 1
    check(pool_bwd(dt, form, dy, idx_dev, 368, 368, True), R.maxpool_bwd_ref(dy, idx, 368, 368, 2, stride, 0).float(),
          f"maxpool2x2 stride {stride} at 368 x 368: dx")


# ================================================================== weight pack

# Cout, Cin, k, with the data-gradient operand, with a bias: the list of test_batched_pack_equals_the_single_layer_pack, then a 1x1 layer of
# exactly one fast tile (16 x 64), its 3x3 sibling without wd, and a 3x3 layer whose Cin = 96 is no multiple of 64 (generic path, ragged
# last tile).  The bf16 fast tiles also need 16-byte aligned OIHW rows: the 5x5 layer (12 525 floats with its bias) is there to bring the
# two after it to a float offset that is a multiple of 4; the 256 x 128 and 512 x 1024 layers before it sit at offset 3 mod 4 and take
# the generic path, the 1024 x 512 and 128 x 384 layers are aligned and take the fast one.
PACK_SHAPES = [(32, 3, 3, True, False), (255, 1024, 1, True, True), (64, 32, 3, True, False), (1024, 512, 3, True, False), (16, 3, 7, False, False),
               (128, 384, 1, True, False), (72, 40, 3, True, False), (7, 64, 1, True, True), (256, 128, 3, True, False), (512, 1024, 1, True, False),
               (25, 20, 5, True, True), (16, 64, 1, True, False), (16, 64, 3, False, False), (32, 96, 3, True, True)]
PACK_ALIGNED = {3: True, 5: True, 8: False, 9: False, 11: True, 12: True}
SPECIAL_LAYERS = (6, 11, 12, 13)                                   # these hold NaN, +-inf and values that round to inf in bf16


@functools.lru_cache(maxsize=None)
def pack_params():
    """one flat fp32 parameter buffer, first tensor at an ODD float offset, no padding between tensors; -> flat, [(w view, bias view or None)]"""
    g = torch.Generator().manual_seed(5)
    total = sum(co * ci * k * k + (co if b else 0) for co, ci, k, d, b in PACK_SHAPES) + 1
    flat = torch.randn(total, generator=g)
    sp = torch.tensor([float("nan"), float("inf"), NINF, 3.4e38, -3.4e38, 3.3895e38, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0])
    off, views = 1, []
    for i, (co, ci, k, d, b) in enumerate(PACK_SHAPES):
        n = co * ci * k * k
        w = flat[off:off + n].view(co, ci, k, k)
        off += n
        if i in SPECIAL_LAYERS:
            at = torch.randperm(n, generator=g)[:4 * sp.numel()]
            w.view(-1)[at] = sp.repeat(4)
        bias = None
        if b:
            bias = flat[off:off + co]
            off += co
        views.append((w, bias))
    return flat, views


@DTS
def test_pack_against_the_definition(dt):
    """mdcv_pack_weights layer by layer and mdcv_pack_weights_batched in one launch (records built as engine.Plan.finish_pack builds them)
    against pack_ref: wf[n][tap][ci], wd[ci][tap][co], padding written as +0 over a sentinel, nothing before or behind, bias copied."""
    L = _lib.lib()
    flat, views = pack_params()
    dev = flat.cuda()
    base = flat.data_ptr()
    es = 2 if dt == BF16 else 4
    recs, outs, eq = [], [], 1
    for i, ((co, ci, k, need_d, has_b), (w, bias)) in enumerate(zip(PACK_SHAPES, views)):
        cop, cip, kk = pad8(co), pad8(ci), k * k
        wptr = dev.data_ptr() + (w.data_ptr() - base)
        assert i not in PACK_ALIGNED or (wptr % 16 == 0) == PACK_ALIGNED[i], (i, wptr % 16)
        bptr = dev.data_ptr() + (bias.data_ptr() - base) if has_b else 0
        nf = cop * kk * cip
        single = (guarded(nf, TD[dt]), guarded(nf, TD[dt]) if need_d else None)
        batched = (guarded(nf, TD[dt]), guarded(nf, TD[dt]) if need_d else None)
        bp = guarded(cop, torch.float32) if has_b else None
        for raw, view in [t for t in single + batched if t is not None]:
            assert view.data_ptr() % 16 == 0 and raw.numel() * es == (nf + 2 * GUARD) * es
        L.check(L.pack_weights(dt, wptr, single[0][1].data_ptr(), single[1][1].data_ptr() if need_d else None, co, ci, k, k, cop, cip, st()), "pack_weights")
        recs.append(struct.pack("<QQQiiiiiiiiQQ", wptr, batched[0][1].data_ptr(), batched[1][1].data_ptr() if need_d else 0, co, ci, kk, cop, cip, 0, 0, 0,
                                bptr, bp[1].data_ptr() if has_b else 0))
        outs.append((single, batched, bp))
        eq = max(eq, (min(64, cip) * kk + 63) // 64)
    assert len(recs[0]) == 72
    table = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).cuda()
    L.check(L.pack_weights_batched(dt, table.data_ptr(), len(PACK_SHAPES), eq, st()), "pack_weights_batched")
    torch.cuda.synchronize()
    for shp, (w, bias), (single, batched, bp) in zip(PACK_SHAPES, views, outs):
        co, ci, k, need_d, has_b = shp
        cop, cip = pad8(co), pad8(ci)
        wf, wd = R.pack_ref(w, cop, cip, dt)
        for name, (f, d) in (("pack_weights", single), ("pack_weights_batched", batched)):
            check_flat(f[1], wf.view(-1), f"{name} {shp}: wf")
            assert guards_ok(f[0], wf.numel()), f"{name} {shp}: written outside wf"
            if need_d:
                check_flat(d[1], wd.view(-1), f"{name} {shp}: wd")
                assert guards_ok(d[0], wd.numel()), f"{name} {shp}: written outside wd"
        if has_b:
            check_flat(bp[1][:co], bias, f"bias copy {shp}")
            assert bool(_is_sentinel(bp[1][co:]).all()) and guards_ok(bp[0], cop), f"bias copy {shp}: written past Cout"


# ================================================================== the comparisons can fail

def test_a_wrong_kernel_would_fail():
    """Each reference in a deliberately wrong variant; the device result must NOT compare equal to it (and does to the right one)."""
    # the last maximum of a plateau instead of the first
    x = H.pool_input("plateau", 2, 16, 13, 13)
    for form in (("2x2", 2), ("gen", 3, 1, 1)):
        y, idx = pool_ref(form, x)
        y2, idx2 = pool_ref(form, x, last_max=True)
        assert torch.equal(y, y2)
        ys, got, _ = pool_fwd(BF16, form, x, True)
        everywhere = torch.ones_like(idx, dtype=torch.bool)
        check_idx(got, idx, everywhere, "first maximum")
        with pytest.raises(AssertionError, match="idx elements differ"):
            check_idx(got, idx2, everywhere, "last maximum")
    # pad channels written as junk
    xl = layout_input(2, 3, 5, 6)
    s = run_to_nhwc(BF16, xl, 32, 8, 8)
    want = R.nhwc_of(xl, 32, BF16)
    check_nhwc(s, want, "pad channels zero")
    live_pad = want.clone()
    live_pad[0, 4, 5, 31] = 1.0
    with pytest.raises(AssertionError, match="1 elements differ"):
        check_nhwc(s, live_pad, "a live pad channel")
    # the vectors on both sides of the wrap boundary (the last of the first trip, the first of the second) exchanged
    xb, wantb = big_layout(BF16)
    sb = run_to_nhwc(BF16, xb, 64, 8, 8)
    moved = wantb.clone()
    v = moved.view(-1, 8)
    assert v.shape[0] > 8192 * 256
    v[8192 * 256 - 1], v[8192 * 256] = wantb.view(-1, 8)[8192 * 256].clone(), wantb.view(-1, 8)[8192 * 256 - 1].clone()
    with pytest.raises(AssertionError, match="elements differ"):
        check_nhwc(sb, moved, "a vector moved over the wrap boundary")
