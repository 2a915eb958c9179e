"""-m gpu: every bf16 convolution kernel family through the C ABI against a float64 reference with `==`, element for element.

tests/test_gpu_kernels.py compares these kernels with a tolerance of a few per cent of an output (a whole term of the K sum at K = 9 x 256);
here the data are integers (tests/helpers/conv_exact.py) chosen so that every product and partial sum is exact in fp32 and every bf16 output is
representable, so a dropped or duplicated term, a wrong tap, a wrong halo pixel or a lost split changes an output by >= 1 quantum and fails.
tests/test_conv_exact_host.py proves, without a GPU, that the reference alone satisfies the exactness conditions at every shape used here.
The fused BatchNorm forms run with the leaky slope 0.5 and dyadic coefficients; scale*y + shift is never 0 (the generator moves y off the root).

Every output buffer is pre-filled with the bit pattern 0x5A5A...; at least one case per group writes a channel slice (offset 8 or 24) of a wider
buffer: pad channels inside the slice must be exact zeros, everything outside the slice untouched.

  entry point                  code                 case (table)                         code path it is there for
  mdcv_conv2d mode 0 / 1       0                    CONV_CASES, both dtypes              default dispatch: narrow / wide im2col tiles, 1x1, 7x7, dilated, stride 2
  mdcv_conv2d mode 0 / 1       1..12, 101..112      VARIANT_CASES, both dtypes           every forced tile configuration (register-staged, LDS-DMA), uniform-tap and generic addresses
  mdcv_conv2d mode 0 / 1       30 / 31              NARROW_CASES                         128x64 tiles of 33..64-channel outputs: 2-stage / 3-stage ring
  mdcv_conv2d mode 0 / 1       2001 / 2000          NARROW_CASES                         256x64, 256x32, 256x16 tiles from 1024 positions / never
  mdcv_conv2d mode 0 / 1       60 / 68              DEEP_SMALL_CASES                     > 64 channels, >= 8 K steps: 2-stage 128x64 tiles / 3-stage ring
  mdcv_conv2d_dgrad_bnsums     92 / 93              FUSE1X1_CASE (dx 256 channels)       fused 1x1 data gradient: heuristic tiles / 128x64 on the 3-stage ring
  mdcv_conv2d mode 0 / 1       0                    SHIFT_CASES                          3x3 shift kernel: 256 / 128-row tiles (192-row tiles need more than 128 tiles: DENSE_CASES), images straddling tiles, wide rows, narrow column
  mdcv_conv2d mode 0 / 1       -8 -9 -12 -30 -31 -201 -3 -4 -17 -18 -19 -15 -14   SHIFT_CASES[:4]   tile plans, K-loop forms, 384-row tiles, ring depth, narrow column, chunk rows
  mdcv_conv2d mode 1           -64 / -63            SHIFT_WIDE_DGRAD                     64-wide data-gradient tiles on / off: 128 x 64 ([0]) and 256 x 64 ([1])
  mdcv_conv2d mode 0 / 1       -15 / -14            SHIFT_W70                            rows of 63..80 pixels: 2-D tiles / the 1-D stream's four-DMA chunk
  mdcv_conv2d mode 0 / 1       -28 (default)        SHIFT_2D                             2-D pixel tiles, ragged right / bottom tiles
  mdcv_conv2d mode 0 / 1       -20 / -21            SHIFT_DIL2                           dilation 2 on the shift kernel / im2col
  mdcv_conv2d mode 1, _dgrad_bnsums   17/16, 15/14, 4001   S2_CASES[1] (even, dx 128 channels)   stride-2 data gradient in ONE launch (ALLCLS): two workgroups per tile (17, 15) / one (4001) ; four launches (16, 14)
  mdcv_conv2d mode 1, _dgrad_bnsums   any           S2_CASES[0] (odd)                    four parity-class launches
  mdcv_conv2d mode 1, _dgrad_bnsums   -60 / -29     S2D_CASES                            shift kernel's stride-2 form / per-class im2col; plain, addsrc, addsrc + sums
  mdcv_conv2d_xstats, mdcv_pw_conv_fwd_xstats   0   XSTATS_CASES, PW_CASES[1]            exact accumulators == the integer sums
  mdcv_conv2d_wgrad            4 5 8 9 10 11        WGRAD_GENERIC                        generic kernel families, accumulate onto an integer dW
  mdcv_conv2d_wgrad            0, 8, 9              WGRAD_SHIFT_CASES, WGRAD_KWSHARED_CASES   LDS-ring kernel (it comes first for every WGRAD_SHIFT_CASES layer, under 8 too) / kw-shared kernel (8, WGRAD_KWSHARED_CASES) / generic (9)
  mdcv_conv2d_wgrad            0 30003 30005 34021 34020 34051 34050   WGRAD_STREAM_CASES, WGRAD_DIRECT_CASES   LDS-ring kernel: light / tiled, table, slab-free; channel slices
  mdcv_conv2d_wgrad            34061/34060, 34071..34073   WGRAD_S2_CASES                parity-plane ring kernel, prefetch depths
  mdcv_conv2d_wgrad            0, 9                 STEM_CASES                           7x7 stem ring kernel
  mdcv_conv2d_wgrad_bnapply    0                    BNAPPLY_CASES                        BatchNorm apply in the operand load
  mdcv_pw_conv_fwd             0                    PW_CASES                             64 / 32 / 16-pixel tiles (K <= 256 / 512 / 1024); weights resident in LDS where K * N * 2 <= 64 KiB, streamed at PW_CASES[3] (512 -> 256) and, in two chunks, at PW_CASES[4] (1024 -> 512)
  mdcv_pw_bwd + mdcv_wgrad_reduce   0               PWB_CASES, plain and fused           one-launch 1x1 backward
  mdcv_first_conv_stats / _bn_act   0               FIRST_CASES                          first-layer streaming passes
  mdcv_conv2d_affine_act       0                    AFFINE_CASES, both dtypes            inference epilogue
  mdcv_conv2d_dgrad_bnsums     0                    FUSE_CASES                           fused sums of every data-gradient family
  mdcv_conv2d mode 0 / 1, _dgrad_bnsums   0         DENSE_CASES                          grids of more than 256 tiles: 3-slot ring, lockstep K loop (what the 52^2 layers run at batch 32)
  mdcv_conv2d mode 0 / 1, _dgrad_bnsums, mdcv_pw_*   0 / 2001   PROD_CASES, PW_PROD_CASES, PWB_PROD_CASES   the remaining instantiations of the production plans (tests/test_gpu_conv_census.py)

The last column is asserted: every test ends in census_assert(), which holds the instantiations its launches ran (helpers/kernel_census.py) against the
purpose pattern of the case (helpers/conv_exact.py purpose) and against its ledger entry (helpers/conv_census_ledger.py).

The pixels-per-tile and weights-resident codes of csrc/tune.h's 1x1 family (64 / 32 / 16, 1000 / 1001) are not reachable through the C ABI (no
entry point of pw_block.hip reads a variant code); the tile sizes are reached through K instead.
"""
import contextlib
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import test_gpu_kernels as K  # noqa: E402
from test_gpu_kernels import to_nhwc, to_nchw, pack, pad8, F32, BF16, TD, st  # noqa: E402,F401
from variant_lib import VariantLib  # noqa: E402
import conv_exact as X  # noqa: E402
import kernel_census as KC  # noqa: E402
import conv_census_ledger as LG  # noqa: E402
from mdcv import _lib  # noqa: E402

torch.set_num_threads(16)
SLOPE = X.SLOPE
DTS = pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])


def test_tables_are_the_kernel_file_tables():
    """The shapes come from tests/test_gpu_kernels.py; the copies in helpers/conv_exact.py (which the host test walks) must not drift."""
    assert X.CONV_CASES == K.CONV_CASES and X.VARIANT_CASES == K.VARIANT_CASES and X.FUSE_CASES == K.FUSE_CASES
    assert X.WGRAD_SHIFT_CASES == K.WGRAD_SHIFT_CASES[:-2] and X.WGRAD_S2_CASES == K.WGRAD_S2_CASES[:-1]
    assert X.PW_CASES == [c for c in K.PW_CASES if c[0] != 70000] and X.PWB_CASES == [c for c in K.PWB_CASES if c[0] != 86528]
    assert X.AFFINE_CASES == K.AFFINE_CASES and set(X.S2D_CASES) <= set(K.S2D_CASES) and set(X.SHIFT_2D) <= set(K.T2D_CASES)
    keep = [c for c in K.WGRAD_STREAM_CASES if c[0] * c[3] * c[4] <= 12800 or c == (1, 64, 128, 104, 104, 1)]
    assert X.WGRAD_STREAM_CASES == keep
    assert X.FIRST_CASES == K.FIRST_CONV_CASES[1:]


@pytest.mark.parametrize("case", [X.CONV_CASES[8], X.CONV_CASES[3]], ids=str)
def test_a_wrong_kernel_would_fail(case):
    """The comparison on the device, not only on the host: the kernel is handed weights with the last 8-channel chunk of ONE tap zeroed (what a K loop
    that stops a chunk early computes) and its result must NOT compare equal to the true reference -- while it does equal the mutated one."""
    L = VariantLib()
    c = plain(case)
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    w = c["w"].clone()
    w[:, Ci - 8:, k - 1, k // 2] = 0
    cm = dict(c, w=w, _y=X.ref_fwd(c, w=w), _dxa=X.ref_dgrad(c, True, w=w))
    run_fwd(L, BF16, cm)
    run_dgrad(L, BF16, cm)
    for run in (run_fwd, run_dgrad):
        with pytest.raises(AssertionError, match="elements differ"):
            run(L, BF16, dict(cm, _y=c["_y"], _dxa=c["_dxa"]), **({"stats": False} if run is run_fwd else {}))
    census_assert()


# ---- device buffers: operands inside wider buffers whose other channels hold junk, outputs pre-filled with a sentinel

def _fill_sentinel(buf):
    if buf.element_size() == 2:
        buf.view(torch.int16).fill_(0x5A5A)
    else:
        buf.view(torch.int32).fill_(0x5A5A5A5A)
    return buf


def _is_sentinel(t):
    return (t.view(torch.int16) == 0x5A5A) if t.element_size() == 2 else (t.view(torch.int32) == 0x5A5A5A5A)


class Slice:
    """A [B, H, W, Cp] channel slice at channel `off` of a [B, H, W, off + Cp + extra] device buffer (Cp = pad8(C))."""

    def __init__(self, dt, B, H, W, C, off=0, extra=0):
        self.dt, self.C, self.Cp, self.off = dt, C, pad8(C), off
        self.ld = off + self.Cp + extra
        self.buf = torch.empty(B, H, W, self.ld, dtype=TD[dt], device="cuda")
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()

    @classmethod
    def of(cls, dt, t, off=0, extra=0, junk=3.0):
        """operand: the NCHW float64 CPU tensor `t` in the slice, pad channels zero, `junk` in every channel outside the slice"""
        B, C, H, W = t.shape
        s = cls(dt, B, H, W, C, off, extra)
        s.buf.fill_(junk)
        s.buf[..., off:off + s.Cp] = 0
        s.buf[..., off:off + C] = t.permute(0, 2, 3, 1).to(TD[dt]).cuda()
        return s

    @classmethod
    def out(cls, dt, B, H, W, C, off=0, extra=0):
        s = cls(dt, B, H, W, C, off, extra)
        _fill_sentinel(s.buf)
        return s

    def check(self, want_nchw, what, tile=128, pad_zero=True, extra=""):
        """the slice == want (exact), its pad channels == 0, everything outside untouched"""
        torch.cuda.synchronize()
        b = self.buf
        X.assert_same(b[..., self.off:self.off + self.C].double().cpu(), want_nchw.permute(0, 2, 3, 1), what, "nhwc", tile, extra)
        if self.Cp > self.C and pad_zero:
            assert not bool(b[..., self.off + self.C:self.off + self.Cp].float().ne(0).any()), f"{what}: pad channels of the slice are not exact zeros"
        outside = torch.cat((b[..., :self.off], b[..., self.off + self.Cp:]), -1)
        assert bool(_is_sentinel(outside.contiguous()).all()), f"{what}: written outside the channel slice"


# ---- which instantiation ran (helpers/kernel_census.py): every run_* helper re-issues its call once inside the in-library profiler, AFTER the
# unprofiled launch has been checked, into the same buffers; the outputs must come out bit for bit the same and the parsed symbols are the census.

_SEEN = []                       # the instantiations the current test's profiled launches ran
_NODE = [None]


@pytest.fixture(autouse=True)
def _census_scope(request):
    _SEEN.clear()
    _NODE[0] = request.node
    yield
    _NODE[0] = None


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def relaunch(L, go, outs, what):
    """`go()` once more under the profiler: every tensor of `outs` bit-identical afterwards; returns (and notes for census_assert) the parsed instantiations"""
    torch.cuda.synchronize()
    first = [_bits(o).clone() for o in outs]
    with KC.launched(L) as syms:
        go()
    for i, (a, o) in enumerate(zip(first, outs)):
        assert torch.equal(a, _bits(o)), f"{what}: output {i} of the second (profiled) launch differs from the first in {int((a != _bits(o)).sum())} elements"
    inst = KC.conv_instantiations(syms)
    assert inst, f"{what}: the profiler saw no convolution kernel ({syms})"
    _SEEN.extend(inst)
    return inst


def census_assert():
    """last statement of every test: the purpose pattern of the case (helpers/conv_exact.py purpose) and its ledger entry (helpers/conv_census_ledger.py)"""
    node = _NODE[0]
    params = dict(node.callspec.params) if hasattr(node, "callspec") else {}
    seen = set(_SEEN)
    recording = bool(os.environ.get("MDCV_CENSUS_RECORD"))
    if recording:                                       # regenerating the ledger: note what ran even where the purpose below fails
        LG.check(node.name, seen)
    need, forbid = X.purpose(node.originalname, params)
    shown = sorted(map(KC.show, seen))
    for pat in need:
        assert any(KC.matches(i, pat) for i in seen), f"{node.name} is there for {pat} and launched none of it: {shown}"
    for pat in forbid:
        hit = [KC.show(i) for i in seen if KC.matches(i, pat)]
        assert not hit, f"{node.name} is there for a path without {pat} and launched {hit}"
    if not recording:
        LG.check(node.name, seen)


def fvec(v, n=None, fill=0.0):
    out = torch.full((n or v.numel(),), fill, dtype=torch.float32)
    out[:v.numel()] = v.float()
    return out.cuda()


def check_rows(part, Cout, sums, what):
    """fp32 partial rows [rows][2][Cp], summed in float64 on the host, == the integer sums of the reference (exactly); pad channels 0"""
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all()), f"{what}: a promised row was not written"
    tot = part.double().sum(0).cpu()
    for i, (s, nm) in enumerate(zip(sums, ("first sum", "second sum"))):
        X.assert_same(tot[i, :Cout], s, f"{what}: {nm} of the partial rows", "rows")
    assert not bool(tot[:, Cout:].ne(0).any()), f"{what}: statistics of pad channels"


def nanrows(rows, Cp):
    return torch.full((rows, 2, Cp), float("nan"), dtype=torch.float32, device="cuda")


def run_fwd(L, dt, c, off=(0, 0), extra=(0, 0), stats=True, tile=128, tag=""):
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    Ho, Wo = c["Ho"], c["Wo"]
    xs = Slice.of(dt, c["x"], off[0], extra[0])
    wf, _ = pack(dt, c["w"].float(), need_d=False)
    ys = Slice.out(dt, B, Ho, Wo, Co, off[1], extra[1])
    bp = fvec(c["bias"], ys.Cp) if c["bias"] is not None else None
    part = None
    if stats:
        rows = L.conv2d_stats_rows_geom(dt, B, Ho, Wo, xs.Cp, ys.Cp, k, k, s, p, d, xs.ld)
        part = nanrows(rows, ys.Cp)

    def go():
        L.check(L.conv2d(dt, 0, xs.ptr, xs.ld, wf.data_ptr(), ys.ptr, ys.ld, bp.data_ptr() if bp is not None else None, None, 0,
                         part.data_ptr() if stats else None, B, H, W, xs.Cp, Ho, Wo, ys.Cp, k, k, s, p, d, st()), "conv fwd")
    go()
    y = c["_y"] if "_y" in c else X.ref_fwd(c)
    ys.check(y, f"forward y {c['geom']} {tag}", tile)
    if stats:
        check_rows(part, Co, (y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))), f"forward statistics {c['geom']} {tag}")
    return relaunch(L, go, [ys.buf] + ([part] if stats else []), f"forward {c['geom']} {tag}")


def run_dgrad(L, dt, c, off=(0, 0), extra=(0, 0), with_add=True, tile=128, tag=""):
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    Ho, Wo = c["Ho"], c["Wo"]
    dys = Slice.of(dt, c["dy"], off[0], extra[0])
    _, wd = pack(dt, c["w"].float())
    dxs = Slice.out(dt, B, H, W, Ci, off[1], extra[1])
    adds = Slice.of(dt, c["addsrc"], 8, 8) if with_add else None

    def go():
        L.check(L.conv2d(dt, 1, dys.ptr, dys.ld, wd.data_ptr(), dxs.ptr, dxs.ld, None, adds.ptr if with_add else None, adds.ld if with_add else 0, None,
                         B, Ho, Wo, dys.Cp, H, W, dxs.Cp, k, k, s, p, d, st()), "conv dgrad")
    go()
    key = "_dxa" if with_add else "_dx"
    dxs.check(c[key] if key in c else X.ref_dgrad(c, with_add), f"data gradient{' + addsrc' if with_add else ''} {c['geom']} {tag}", tile)
    return relaunch(L, go, [dxs.buf], f"data gradient {c['geom']} {tag}")


def run_dgrad_fused(L, dt, c, code, with_add=True, tile=128, tag="", off=(0, 0), extra=(0, 0)):
    """mdcv_conv2d_dgrad_bnsums: dx exact, partial rows == sum g, sum g (y - mean) with the producer tensors c['bn_in']"""
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    Ho, Wo = c["Ho"], c["Wo"]
    bn = c["bn_in"]
    dys = Slice.of(dt, c["dy"], off[0], extra[0])
    _, wd = pack(dt, c["w"].float())
    dxs = Slice.out(dt, B, H, W, Ci, off[1], extra[1])
    adds = Slice.of(dt, c["addsrc"], 8, 0) if with_add else None
    fy = Slice.of(dt, bn["y"], 0, 8)
    rows = L.conv2d_dgrad_bnsums_rows(dt, B, Ho, Wo, dys.Cp, H, W, dxs.Cp, k, k, s, p, d, dys.ld)
    assert rows > 0, "the geometry does not take the fused path"
    part = nanrows(rows, dxs.Cp)
    sc, sh, mn = fvec(bn["scale"], dxs.Cp), fvec(bn["shift"], dxs.Cp), fvec(bn["mean"], dxs.Cp)

    def go():
        L.check(L.conv2d_dgrad_bnsums(dt, dys.ptr, dys.ld, wd.data_ptr(), dxs.ptr, dxs.ld, adds.ptr if with_add else None, adds.ld if with_add else 0,
                                      B, Ho, Wo, dys.Cp, H, W, dxs.Cp, k, k, s, p, d, fy.ptr, fy.ld, sc.data_ptr(), sh.data_ptr(), mn.data_ptr(), code, SLOPE,
                                      part.data_ptr(), st()), "fused dgrad")
    go()
    key = "_dxa" if with_add else "_dx"
    dz = c[key] if key in c else X.ref_dgrad(c, with_add)
    dxs.check(dz, f"fused data gradient {c['geom']} act {code} {tag}", tile)
    _, sg, sgx = X.ref_bn_sums(bn, dz, code)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part[:, :, :Ci]).all()), "a promised row was not written"
    tot = part.double().sum(0).cpu()
    X.assert_same(tot[0, :Ci], sg, f"fused sums {c['geom']} {tag}: sum g", "rows")
    X.assert_same(tot[1, :Ci], sgx, f"fused sums {c['geom']} {tag}: sum g (y - mean)", "rows")
    return relaunch(L, go, [dxs.buf, part], f"fused data gradient {c['geom']} {tag}")


def run_wgrad(L, dt, c, accumulate=1, off=(0, 0), extra=(0, 0), tag="", ci_real=None, co_real=None, cpad_x=None, guard=0):
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    Ho, Wo = c["Ho"], c["Wo"]
    if cpad_x:                                          # the stem: 3 real channels in a 16-channel buffer whose other channels are zeros
        xs = Slice.of(dt, c["x"], 0, cpad_x - pad8(Ci), junk=0.0)
        xs.Cp = cpad_x
    else:
        xs = Slice.of(dt, c["x"], off[0], extra[0])
    dys = Slice.of(dt, c["dy"], off[1], extra[1])
    cr, orr = ci_real or Ci, co_real or Co
    splits = L.conv2d_wgrad_splits_geom(dt, B, H, W, xs.Cp, Ho, Wo, dys.Cp, k, k, s, p, d, dys.ld, xs.ld)
    assert splits >= 1
    n = splits * dys.Cp * k * k * xs.Cp
    ws = torch.full((n + guard,), float("nan"), dtype=torch.float32, device="cuda")
    g = torch.Generator().manual_seed(7)
    init = torch.randint(-5, 6, (orr, cr, k, k), generator=g).float() if accumulate else torch.full((orr, cr, k, k), 7.0)
    dw = init.cuda()

    def go():
        L.check(L.conv2d_wgrad(dt, dys.ptr, dys.ld, xs.ptr, xs.ld, ws.data_ptr(), splits, dw.data_ptr(), accumulate, B, H, W, xs.Cp, cr,
                               Ho, Wo, dys.Cp, orr, k, k, s, p, d, st()), "wgrad")
    go()
    torch.cuda.synchronize()
    want = (c["_dw"] if "_dw" in c else X.ref_wgrad(c))[:orr, :cr]
    if accumulate:
        want = want + init.double()
    X.assert_same(dw.double().cpu(), want, f"weight gradient {c['geom']} {tag} splits {splits}", "oihw")
    if guard:
        assert bool(torch.isnan(ws[n:]).all()), "slabs written past the end"
    got = dw.clone()
    dw.copy_(init)                                      # the same call: dW as it stood before the first one (it accumulates)
    relaunch(L, go, [], f"weight gradient {c['geom']} {tag}")
    assert torch.equal(_bits(got), _bits(dw)), f"weight gradient {c['geom']} {tag}: the second (profiled) launch differs from the first"
    return splits


def plain(case):
    """the case with its references, computed once in the helper and shared by the parametrized variants (never modified)"""
    return X.conv_refs(case)


def variant(L, code, family="conv"):
    class _Ctx:
        def __enter__(self_):
            (L.conv2d_set_variant if family == "conv" else L.conv2d_wgrad_set_variant)(code)

        def __exit__(self_, *a):
            L.conv = L.wgrad = 0
    return _Ctx()


# ================================================================== group A: generic implicit-GEMM kernels

@DTS
@pytest.mark.parametrize("case", X.CONV_CASES, ids=str)
def test_a_conv_cases(case, dt):
    L = VariantLib()
    c = plain(case)
    i = X.CONV_CASES.index(case)
    off = ((0, 0), (8, 24), (24, 8))[i % 3]             # every third case plain, the others as channel slices of wider buffers (ldc > C)
    ex = ((0, 0), (16, 8), (8, 16))[i % 3]
    run_fwd(L, dt, c, off, ex)
    run_dgrad(L, dt, c, off, ex)
    run_wgrad(L, dt, c, 1)
    census_assert()


@DTS
@pytest.mark.parametrize("code", list(range(12)) + list(range(100, 112)))
def test_a_tile_variants(code, dt):
    L = VariantLib()
    for i, case in enumerate(X.VARIANT_CASES):
        c = plain(case)
        with variant(L, code):
            run_fwd(L, dt, c, (8, 0) if i == 0 else (0, 0), (8, 8) if i == 0 else (0, 0), tag=f"code {code}")
            run_dgrad(L, dt, c, (0, 24) if i == 1 else (0, 0), (0, 8) if i == 1 else (0, 0), tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [30, 31, 2000, 2001])
@pytest.mark.parametrize("case", X.NARROW_CASES, ids=str)
def test_a_narrow_output_codes(case, code):
    """Outputs of <= 64 channels with >= 1024 positions (helpers/conv_exact.py NARROW_CASES).  30 / 31: the 3-stage ring of the 128 x 64 tiles never / from
    one K step (the default) -- it exists for 33..64 channels, i.e. NARROW_CASE.  2001 / 2000: the 256-row tiles (256 x 64, 256 x 32, 256 x 16) from 1024
    positions / never; the default threshold of 256 Ki positions is far above any test shape, so only 2001 runs them."""
    L = VariantLib()
    c = plain(case)
    with variant(L, code):
        run_fwd(L, BF16, c, tag=f"code {code}")
        run_dgrad(L, BF16, c, tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [60, 68])
@pytest.mark.parametrize("case", X.DEEP_SMALL_CASES, ids=str)
def test_a_deep_small_codes(case, code):
    """Outputs of > 64 channels on a sparse grid with >= 8 K steps forward: 68 (= the default) takes the 3-stage ring, 60 the 2-stage 128 x 64 tiles."""
    L = VariantLib()
    c = plain(case)
    with variant(L, code):
        run_fwd(L, BF16, c, tag=f"code {code}")
        run_dgrad(L, BF16, c, tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [92, 93])
def test_a_fused_1x1_tiles(code):
    """The fused data gradient of a 1x1 layer whose dx has 256 channels: 93 (default) 128 x 64 tiles on the 3-stage ring, 92 the heuristic's tiles."""
    L = VariantLib()
    c = plain(X.FUSE1X1_CASE)
    with variant(L, code):
        run_dgrad_fused(L, BF16, c, 1, tag=f"code {code}")
    census_assert()


# ================================================================== group B: the 3x3 stride-1 shift kernel

@pytest.mark.parametrize("case", X.SHIFT_CASES, ids=str)
def test_b_shift_default(case):
    L = VariantLib()
    c = plain(X.c3(case, bias=case == X.SHIFT_CASES[0]))
    sl = case == X.SHIFT_CASES[1]
    run_fwd(L, BF16, c, (8, 24) if sl else (0, 0), (8, 8) if sl else (0, 0))
    run_dgrad(L, BF16, c, (24, 8) if sl else (0, 0), (8, 8) if sl else (0, 0))
    census_assert()


@pytest.mark.parametrize("code", X.SHIFT_CODES)
@pytest.mark.parametrize("case", X.SHIFT_CASES[:4], ids=str)
def test_b_shift_codes(case, code):
    L = VariantLib()
    c = plain(X.c3(case, bias=case == X.SHIFT_CASES[0]))
    with variant(L, code):
        run_fwd(L, BF16, c, tag=f"code {code}", tile=384 if code == -201 else 128)
        run_dgrad(L, BF16, c, tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [-15, -14])
def test_b_shift_rows_of_63_to_80_pixels(code):
    """-15 / -14 (shift_wmax 62 / 80) decide only for rows of 63..80 pixels: W = 70 runs the 1-D stream's four-DMA chunk under -14 and 2-D tiles under -15."""
    L = VariantLib()
    c = plain(X.c3(X.SHIFT_W70))
    with variant(L, code):
        run_fwd(L, BF16, c, tag=f"code {code}")
        run_dgrad(L, BF16, c, tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [-64, -63])
@pytest.mark.parametrize("case", X.SHIFT_WIDE_DGRAD, ids=str)
def test_b_shift_wide_dgrad_tiles(case, code):
    L = VariantLib()
    B, Ci, H, W, Co = case
    c = X.gen_case(X.seed_of(case), B, Ci, H, W, Co, 3)
    with variant(L, code):
        run_dgrad(L, BF16, c, tag=f"code {code}", tile=256)
    census_assert()


@pytest.mark.parametrize("case", X.SHIFT_2D, ids=str)
def test_b_shift_2d_tiles(case):
    L = VariantLib()
    c = plain(X.c3(case))
    with variant(L, -28):                               # (-28 is the default: these widths run the 2-D tiles without a code)
        run_fwd(L, BF16, c, tag="2-D tiles (8 x 30), default")
        run_dgrad(L, BF16, c, tag="2-D tiles (8 x 30), default")
    census_assert()


@pytest.mark.parametrize("code", [-20, -21])
@pytest.mark.parametrize("case", X.SHIFT_DIL2, ids=str)
def test_b_shift_dilation2(case, code):
    L = VariantLib()
    c = plain(X.c3(case, dil=2))
    with variant(L, code):
        run_fwd(L, BF16, c, tag=f"code {code}")
        run_dgrad(L, BF16, c, tag=f"code {code}")
    census_assert()


# ================================================================== group C: stride-2 data gradients

@pytest.mark.parametrize("code", [17, 16, 15, 14, 4001])
@pytest.mark.parametrize("case", X.S2_CASES, ids=str)
def test_c_stride2_dgrad_forms(case, code):
    """(2, 64, 17, 19, 128): odd sizes, four parity-class launches under every code.  (2, 128, 16, 20, 128): even sizes and a 128-channel dx (64 / 32
    channels would run the shift kernel's stride-2 form) -- ONE launch for the four classes (conv_glds_kernel ALLCLS) with two workgroups per tile
    under 17 / 15 (the defaults: 2 tiles of 128 x 128 < conv_s2_split = 512), ONE launch with one workgroup per tile under 4001 (conv_s2_split = 1:
    the form grids of >= 512 tiles take), four launches under 16 and under 14 (csrc/conv_igemm.hip:44, conv_gemm.h dispatch_dgrad_s2_all).  Plain, with
    addsrc in channel slices, and with the fused sums."""
    L = VariantLib()
    B, Ci, H, W, Co = case
    c = plain((B, Ci, H, W, Co, 3, 2, 1, 1, False))
    with variant(L, code):
        run_dgrad(L, BF16, c, (8, 24), (8, 8), tag=f"code {code}, channel slices")
        run_dgrad(L, BF16, c, with_add=False, tag=f"code {code}")
        run_dgrad_fused(L, BF16, c, 1, tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("form", ["plain", "addsrc", "addsrc+bnsums"])
@pytest.mark.parametrize("code", [-60, -29])
@pytest.mark.parametrize("case", X.S2D_CASES, ids=str)
def test_c_shift_stride2_dgrad(case, code, form):
    L = VariantLib()
    B, Cdy, Hd, Wd, Cdx = case
    c = plain((B, Cdx, 2 * Hd, 2 * Wd, Cdy, 3, 2, 1, 1, False))
    with variant(L, code):
        if code == -60:
            assert L.conv2d_dgrad_s2_form_ok(BF16, B, Hd, Wd, Cdy, 2 * Hd, 2 * Wd, Cdx, 3, 3, 2, 1, 1, Cdy) == 1
        if form == "addsrc+bnsums":
            run_dgrad_fused(L, BF16, c, 1, tag=f"code {code}", tile=248)
        else:
            run_dgrad(L, BF16, c, with_add=form == "addsrc", tag=f"code {code}", tile=248)
    census_assert()


# ================================================================== group D: forward statistics through the exact accumulators
# (the partial rows of stats_partial are compared exactly in EVERY forward run of groups A, B and F: check_rows)

XSTATS_CASES = [(X.CONV_CASES[1], 0), (X.CONV_CASES[2], 0), (X.CONV_CASES[4], 0), (X.VARIANT_CASES[0], 8), (X.c3(X.SHIFT_CASES[0], True), 0),
                (X.c3(X.SHIFT_CASES[3]), 0), (X.c3(X.SHIFT_CASES[3]), -201), (X.c3(X.SHIFT_2D[0]), 0), (X.c3(X.SHIFT_DIL2[0], dil=2), 0)]


def digits_to_int(acc, reps, Cp):
    d = acc.reshape(reps, 3, 2, Cp).sum(0).cpu().numpy().astype(object)
    return d[0] + d[1] * (1 << 40) + d[2] * (1 << 80)           # python integers in units of 2^-70


@pytest.mark.parametrize("case,code", XSTATS_CASES, ids=str)
def test_d_conv_xstats_digits(case, code):
    L = VariantLib()
    c = plain(case)
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    Ho, Wo = c["Ho"], c["Wo"]
    sl = case in (X.VARIANT_CASES[0], X.c3(X.SHIFT_CASES[3]))          # a generic and a shift-kernel case as channel slices of wider buffers
    xs = Slice.of(BF16, c["x"], 8 if sl else 0, 8 if sl else 0)
    wf, _ = pack(BF16, c["w"].float(), need_d=False)
    ys = Slice.out(BF16, B, Ho, Wo, Co, 24 if sl else 0, 8 if sl else 0)
    bp = fvec(c["bias"], ys.Cp) if c["bias"] is not None else None
    with variant(L, code):
        rows = L.conv2d_stats_rows_geom(BF16, B, Ho, Wo, xs.Cp, ys.Cp, k, k, s, p, d, xs.ld)
        reps = L.xstats_reps(rows, ys.Cp)
        acc = torch.zeros(L.xstats_words(reps, ys.Cp), dtype=torch.int64, device="cuda")
        xstats_call = L.conv2d_xstats

    def go():
        L.check(xstats_call(BF16, xs.ptr, xs.ld, wf.data_ptr(), ys.ptr, ys.ld, bp.data_ptr() if bp is not None else None, acc.data_ptr(), reps,
                            B, H, W, xs.Cp, Ho, Wo, ys.Cp, k, k, s, p, d, st()), "conv_xstats")
    go()
    y = c["_y"]
    ys.check(y, f"conv_xstats y {case}")
    tot = digits_to_int(acc, reps, ys.Cp)
    s1, s2 = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    for ch in range(ys.Cp):
        want = (int(s1[ch]) << 70, int(s2[ch]) << 70) if ch < Co else (0, 0)
        assert (int(tot[0, ch]), int(tot[1, ch])) == want, (case, ch, int(tot[0, ch]) / 2 ** 70, int(tot[1, ch]) / 2 ** 70, float(s1[min(ch, Co - 1)]))
    first = acc.clone()
    acc.zero_()                                         # the same call: the accumulators as they stood before the first one
    relaunch(L, go, [ys.buf], f"conv_xstats {case}")
    assert torch.equal(first, acc), f"conv_xstats {case}: the accumulators of the second (profiled) launch differ from the first"
    census_assert()


# ================================================================== group E: weight gradients (dW fp32, ==)

WGRAD_GENERIC = [X.CONV_CASES[1], X.CONV_CASES[3], X.CONV_CASES[7], X.VARIANT_CASES[1], X.c3(X.WGRAD_SHIFT_CASES[0]), (3, 64, 26, 20, 64, 3, 1, 1, 1, False)]


@pytest.mark.parametrize("code", [4, 5, 8, 9, 10, 11])
@pytest.mark.parametrize("case", WGRAD_GENERIC, ids=str)
def test_e_wgrad_family_codes(case, code):
    L = VariantLib()
    c = plain(case)
    with variant(L, code, "wgrad"):
        run_wgrad(L, BF16, c, 1, tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [0, 8, 9])
@pytest.mark.parametrize("case", X.WGRAD_SHIFT_CASES + X.WGRAD_KWSHARED_CASES, ids=str)
def test_e_wgrad_shift(case, code):
    L = VariantLib()
    c = plain(X.c3(case))
    with variant(L, code, "wgrad"):
        run_wgrad(L, BF16, c, 0, tag=f"code {code}")
        run_wgrad(L, BF16, c, 1, tag=f"code {code}, accumulate")
    census_assert()


def stream10(t):
    B, Ci, Co, H, W, dil = t
    return (B, Ci, H, W, Co, 3, 1, dil, dil, False)


@pytest.mark.parametrize("code", [0, 30003, 30005, 34021, 34020, 34050])
@pytest.mark.parametrize("case", X.WGRAD_STREAM_CASES, ids=str)
def test_e_wgrad_stream(case, code):
    L = VariantLib()
    c = wide_case(stream10(case))
    with variant(L, code, "wgrad"):
        run_wgrad(L, BF16, c, 1, tag=f"code {code}")
        if code in (0, 34020):
            run_wgrad(L, BF16, c, 0, (8, 16), (16, 0), tag=f"code {code}, x and dy as channel slices")
    census_assert()


def wide_case(case10):
    """plain() where the reference fits the cap, else (the two listed 512 -> 1024 layers at 13 x 13) the weight-gradient reference alone, cached"""
    if X.macs(case10) <= X.MACS_CAP:
        return plain(case10)
    if case10 not in _WIDE:
        _WIDE.clear()
        B, Ci, H, W, Co, k, s, p, d, _ = case10
        c = X.gen_case(X.seed_of(case10), B, Ci, H, W, Co, k, s, p, d)
        c["_dw"] = X.ref_wgrad(c)
        _WIDE[case10] = c
    return _WIDE[case10]


_WIDE = {}


@pytest.mark.parametrize("code", [34051, 34050])
@pytest.mark.parametrize("case", X.WGRAD_DIRECT_CASES, ids=str)
def test_e_wgrad_slab_free(case, code):
    """One split of 64 co x 32 ci tiles fills the chip: the kernel writes OIHW rows itself (34051, the default) / the slab form (34050); cropped real channels."""
    L = VariantLib()
    c = wide_case(stream10(case))
    with variant(L, code, "wgrad"):
        splits = run_wgrad(L, BF16, c, 1, tag=f"code {code}")
        assert (splits == 1) == (code == 34051)
        run_wgrad(L, BF16, c, 0, tag=f"code {code}, cropped", ci_real=500, co_real=1020)
    census_assert()


@pytest.mark.parametrize("code", [34061, 34060, 34071, 34072, 34073])
@pytest.mark.parametrize("case", X.WGRAD_S2_CASES, ids=str)
def test_e_wgrad_stride2(case, code):
    L = VariantLib()
    B, Ci, Co, Ho, Wo, extra = case
    c = plain((B, Ci, 2 * Ho, 2 * Wo, Co, 3, 2, 1, 1, False))
    with variant(L, code, "wgrad"):
        run_wgrad(L, BF16, c, 1, (extra, 2 * extra), (2 * extra, 0), tag=f"code {code}")
    census_assert()


@pytest.mark.parametrize("code", [0, 9])
@pytest.mark.parametrize("case", X.STEM_CASES, ids=str)
def test_e_wgrad_stem_7x7(case, code):
    L = VariantLib()
    B, H, W = case
    c = plain((B, 3, H, W, 16, 7, 1, 3, 1, False))
    with variant(L, code, "wgrad"):
        run_wgrad(L, BF16, c, 1, tag=f"code {code}", cpad_x=16, guard=4096)
    census_assert()


@pytest.mark.parametrize("case", X.BNAPPLY_CASES, ids=str)
def test_e_wgrad_bnapply(case):
    """dy = cA g + cB y + cC is formed in the operand load and rounded to bf16: with dyadic coefficients that value is a bf16 number (host test), so dW is exact."""
    L = _lib.lib()
    dt = BF16
    B, Ci, H, W, Co, k, s, p, code = case
    c = plain((B, Ci, H, W, Co, k, s, p, 1, False))
    Ho, Wo = c["Ho"], c["Wo"]
    bn = c["bn_out"]
    xs, dzs, ys = Slice.of(dt, c["x"]), Slice.of(dt, c["dy"]), Slice.of(dt, bn["y"])
    geom = (B, H, W, xs.Cp, Ho, Wo, dzs.Cp, k, k, s, p, 1)
    assert L.conv2d_wgrad_bnapply_ok(dt, *geom, dzs.ld, ys.ld, xs.ld) == 1
    splits = L.conv2d_wgrad_splits_geom(dt, *geom, dzs.ld, xs.ld)
    ws = torch.full((splits * dzs.Cp * k * k * xs.Cp,), float("nan"), device="cuda")
    init = torch.randint(-5, 6, (Co, Ci, k, k), generator=torch.Generator().manual_seed(3)).float()
    dw = init.cuda()
    v = [fvec(bn[n], dzs.Cp) for n in ("scale", "shift", "cA", "cB", "cC")]

    def go():
        L.check(L.conv2d_wgrad_bnapply(dt, dzs.ptr, dzs.ld, ys.ptr, ys.ld, *[t.data_ptr() for t in v], code, SLOPE, xs.ptr, xs.ld, ws.data_ptr(), splits,
                                       dw.data_ptr(), 1, B, H, W, xs.Cp, Ci, Ho, Wo, dzs.Cp, Co, k, k, s, p, 1, st()), "wgrad_bnapply")
    go()
    torch.cuda.synchronize()
    want = X.ref_wgrad(c, dy=X.ref_bn_apply(bn, c["dy"], code)) + init.double()
    X.assert_same(dw.double().cpu(), want, f"wgrad_bnapply {case} splits {splits}", "oihw")
    got = dw.clone()
    dw.copy_(init)
    relaunch(L, go, [], f"wgrad_bnapply {case}")
    assert torch.equal(_bits(got), _bits(dw)), f"wgrad_bnapply {case}: the second (profiled) launch differs from the first"
    census_assert()


# ================================================================== group F: the 1x1 block

def mat(dt, t2d, extra=0, junk=3.0):
    """[M, C] float64 -> device [M, C + extra] with junk in the extra columns"""
    M, C = t2d.shape
    b = torch.full((M, C + extra), junk, dtype=TD[dt], device="cuda")
    b[:, :C] = t2d.to(TD[dt]).cuda()
    return b


@pytest.mark.parametrize("case", X.PW_CASES, ids=str)
def test_f_pw_forward(case):
    _pw_forward(case)
    census_assert()


def _pw_forward(case):
    L = _lib.lib()
    M, Kc, N, xs_, with_r, code = case
    r = X.pw_refs(case)
    bn, c = r["bn"], r["c"]
    ldy, ldz, ldo = Kc + xs_, Kc + 2 * xs_, N + xs_
    y = mat(BF16, bn["y"][0, :, :, 0].t(), xs_)
    res = mat(BF16, r["resid"][0, :, :, 0].t(), xs_) if with_r else None
    wf, _ = pack(BF16, c["w"].float(), need_d=False)
    bias = fvec(c["bias"], pad8(N)) if c["bias"] is not None else None
    sc, sh = fvec(bn["scale"]), fvec(bn["shift"])
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    for xstats in (False, True):
        if xstats and case != X.PW_CASES[1] and case != X.PW_CASES[4]:
            continue
        z = _fill_sentinel(torch.empty(M, ldz, dtype=torch.bfloat16, device="cuda"))
        o = _fill_sentinel(torch.empty(M, ldo, dtype=torch.bfloat16, device="cuda"))
        rows = L.pw_rows(M, Kc)
        if xstats:
            reps = L.xstats_reps(rows, N)
            acc = torch.zeros(L.xstats_words(reps, N), dtype=torch.int64, device="cuda")

            def go():
                L.check(L.pw_conv_fwd_xstats(BF16, y.data_ptr(), ldy, sc.data_ptr(), sh.data_ptr(), P(res), ldy, code, SLOPE, z.data_ptr(), ldz, wf.data_ptr(),
                                             P(bias), o.data_ptr(), ldo, acc.data_ptr(), reps, M, Kc, N, st()), "pw_conv_fwd_xstats")
        else:
            part = nanrows(rows, N)

            def go():
                L.check(L.pw_conv_fwd(BF16, y.data_ptr(), ldy, sc.data_ptr(), sh.data_ptr(), P(res), ldy, code, SLOPE, z.data_ptr(), ldz, wf.data_ptr(),
                                      P(bias), o.data_ptr(), ldo, part.data_ptr(), M, Kc, N, st()), "pw_conv_fwd")
        go()
        torch.cuda.synchronize()
        X.assert_same(z[:, :Kc].double().cpu(), r["z"], f"pw forward z {case}", "rows")
        X.assert_same(o[:, :N].double().cpu(), r["out"], f"pw forward out {case}", "rows")
        assert bool(_is_sentinel(z[:, Kc:].contiguous()).all()) and bool(_is_sentinel(o[:, N:].contiguous()).all()), "written between the rows"
        s1, s2 = r["out"].sum(0), (r["out"] * r["out"]).sum(0)
        if xstats:
            tot = digits_to_int(acc, reps, N)
            for ch in range(N):
                assert int(tot[0, ch]) == int(s1[ch] * 4) << 68 and int(tot[1, ch]) == int(s2[ch] * 4) << 68, (case, ch)
        else:
            check_rows(part, N, (s1, s2), f"pw forward statistics {case}")
        if xstats:
            first = acc.clone()
            acc.zero_()
        relaunch(L, go, [z, o] + ([] if xstats else [part]), f"pw forward {case}")
        assert not xstats or torch.equal(first, acc), f"pw forward {case}: the accumulators of the second (profiled) launch differ from the first"


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bnsums"])
@pytest.mark.parametrize("case", X.PWB_CASES, ids=str)
def test_f_pw_backward(case, fused):
    _pw_backward(case, fused)
    census_assert()


def _pw_backward(case, fused):
    L = _lib.lib()
    M, Kc, Kr, N, xs_, with_add = case
    r = X.pwb_refs(case)
    c, bn = r["c"], r["c"]["bn_in"]
    ldk, ldn = Kc + xs_, N + xs_
    dy2 = torch.zeros(M, Kc, dtype=torch.float64)
    dy2[:, :Kr] = c["dy"][0, :, :, 0].t()
    dy = mat(BF16, dy2, xs_)
    x = mat(BF16, c["x"][0, :, :, 0].t(), xs_)
    add = mat(BF16, c["addsrc"][0, :, :, 0].t(), xs_) if with_add else None
    fy = mat(BF16, bn["y"][0, :, :, 0].t(), xs_)
    _, wd = pack(BF16, c["w"].float())
    sc, sh, mn = fvec(bn["scale"]), fvec(bn["shift"]), fvec(bn["mean"])
    P = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    slabs = L.pw_bwd_slabs(BF16, M, N, Kc, ldk, ldn, ldn, ldn if with_add else 8, ldn if fused else 8)
    assert slabs >= 1
    ws = torch.full((slabs, Kc, N), float("nan"), device="cuda")
    part = torch.full((slabs, 2, N), float("nan"), device="cuda")
    dx = _fill_sentinel(torch.empty(M, ldn, dtype=torch.bfloat16, device="cuda"))
    init = torch.randint(-5, 6, (Kr, N, 1, 1), generator=torch.Generator().manual_seed(5)).float()
    dw = init.cuda()

    def go():
        L.check(L.pw_bwd(BF16, dy.data_ptr(), ldk, x.data_ptr(), ldn, wd.data_ptr(), dx.data_ptr(), ldn, P(add), ldn, ws.data_ptr(), slabs,
                         fy.data_ptr() if fused else None, ldn, sc.data_ptr(), sh.data_ptr(), mn.data_ptr(), 1, SLOPE, part.data_ptr(), M, N, Kc, st()), "pw_bwd")
        L.check(L.wgrad_reduce(ws.data_ptr(), slabs, dw.data_ptr(), 1, Kc, Kr, N, N, 1, st()), "wgrad_reduce")
    go()
    torch.cuda.synchronize()
    dz = r["dxa"] if with_add else r["dx"]
    X.assert_same(dx[:, :N].double().cpu(), dz[0, :, :, 0].t(), f"pw backward dx {case}", "rows")
    assert bool(_is_sentinel(dx[:, N:].contiguous()).all()), "written between the rows"
    X.assert_same(dw.double().cpu(), r["dw"] + init.double(), f"pw backward dW {case} slabs {slabs}", "oihw")
    if fused:
        _, sg, sgx = X.ref_bn_sums(bn, dz, 1)
        assert bool(torch.isfinite(part).all())
        tot = part.double().sum(0).cpu()
        X.assert_same(tot[0], sg, f"pw backward {case}: sum g", "rows")
        X.assert_same(tot[1], sgx, f"pw backward {case}: sum g (y - mean)", "rows")
    got = dw.clone()
    dw.copy_(init)
    relaunch(L, go, [dx, ws] + ([part] if fused else []), f"pw backward {case}")
    assert torch.equal(_bits(got), _bits(dw)), f"pw backward {case}: dW of the second (profiled) launch differs from the first"


# ================================================================== group G: first-layer and inference forms

@pytest.mark.parametrize("case", X.FIRST_CASES, ids=str)
def test_g_first_conv(case):
    L = _lib.lib()
    dt = BF16
    B, Ci, H, W, code = case
    r = X.first_refs(case)
    c = r["c"]
    xs = Slice.of(dt, c["x"])
    assert xs.Cp == 8 and L.first_conv_ok(dt, B, H, W, 8, 32, 3, 3, 1, 1, 1, 8) == 1
    wf, _ = pack(dt, c["w"].float(), need_d=False)
    rows = L.first_conv_rows(B, H)
    part = nanrows(rows, 32)

    def go_stats():
        L.check(L.first_conv_stats(dt, xs.ptr, 8, wf.data_ptr(), part.data_ptr(), B, H, W, st()), "first_conv_stats")
    go_stats()
    y = r["y"]
    check_rows(part, 32, (y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))), f"first_conv_stats {case}")
    sc, sh = fvec(r["scale"]), fvec(r["shift"])
    ys, zs = Slice.out(dt, B, H, W, 32), Slice.out(dt, B, H, W, 32, 8, 8)

    def go_act():
        L.check(L.first_conv_bn_act(dt, xs.ptr, 8, wf.data_ptr(), sc.data_ptr(), sh.data_ptr(), code, SLOPE, ys.ptr, ys.ld, zs.ptr, zs.ld, B, H, W, st()), "first_conv_bn_act")
    go_act()
    ys.check(y, f"first conv y {case}", tile=4 * W)
    zs.check(r["z"], f"first conv z {case}", tile=4 * W)
    relaunch(L, go_stats, [part], f"first_conv_stats {case}")
    relaunch(L, go_act, [ys.buf, zs.buf], f"first_conv_bn_act {case}")
    census_assert()


@DTS
@pytest.mark.parametrize("case", X.AFFINE_CASES, ids=str)
def test_g_affine_act(case, dt):
    _affine_act(case, dt)
    census_assert()


def _affine_act(case, dt, variant_code=0):
    L = VariantLib()
    if variant_code:
        L.conv2d_set_variant(variant_code)
    B, Ci, H, W, Co, k, s, with_r, code = case
    r = X.affine_refs(case)
    c = r["c"]
    Ho, Wo = c["Ho"], c["Wo"]
    p = (k - 1) // 2
    xs = Slice.of(dt, c["x"], 8, 8)
    wf, _ = pack(dt, c["w"].float(), need_d=False)
    rs = Slice.of(dt, c["resid"], 0, 8) if with_r else None
    os_ = Slice.out(dt, B, Ho, Wo, Co, 24, 8)
    sc, sh = fvec(r["scale"], os_.Cp), fvec(r["shift"], os_.Cp)

    def go():
        L.check(L.conv2d_affine_act(dt, xs.ptr, xs.ld, wf.data_ptr(), os_.ptr, os_.ld, sc.data_ptr(), sh.data_ptr(), rs.ptr if with_r else None,
                                    rs.ld if with_r else 0, code, SLOPE, B, H, W, xs.Cp, Ho, Wo, os_.Cp, k, k, s, p, 1, st()), "affine_act")
    go()
    os_.check(r["out"], f"affine_act {case}")
    relaunch(L, go, [os_.buf], f"affine_act {case}")


# ================================================================== group H: data gradients with the fused BatchNorm sums

@pytest.mark.parametrize("code,with_add", [(1, True), (0, False), (2, True)])
@pytest.mark.parametrize("case", X.FUSE_CASES, ids=str)
def test_h_dgrad_bnsums(case, code, with_add):
    L = VariantLib()
    B, Ci, H, W, Co, k, s, p = case
    d = 2 if (k == 3 and p == 2) else 1
    c = plain((B, Ci, H, W, Co, k, s, p, d, False))
    sl = X.FUSE_CASES.index(case) % 2 == 1               # every other case: dy and dx as channel slices of wider buffers
    run_dgrad_fused(L, BF16, c, code, with_add, off=(8, 24) if sl else (0, 0), extra=(8, 8) if sl else (0, 0))
    census_assert()


# ================================================================== group I: dense grids -- the instantiations the production plans launch
# (helpers/conv_exact.py DENSE_CASES: more than 256 tiles, so that the DEFAULT code takes the 3-slot ring and the lockstep K loop; tests/test_gpu_conv_census.py)

@pytest.mark.parametrize("case", [X.DENSE_FWD, X.DENSE_FWD256], ids=str)
def test_i_dense_forward(case):
    L = VariantLib()
    c = X.dense_refs(case)
    sl = case == X.DENSE_FWD                              # y as a channel slice of a wider buffer
    run_fwd(L, BF16, c, (8, 24) if sl else (0, 0), (8, 8) if sl else (0, 0), tile=192 if sl else 256, tag="dense grid, default code")
    census_assert()


@pytest.mark.parametrize("form", ["plain", "addsrc", "bnsums"])
def test_i_dense_dgrad(form):
    L = VariantLib()
    c = X.dense_refs(X.DENSE_DGRAD)
    if form == "bnsums":                                  # dy and dx as channel slices of wider buffers; the partial rows are checked in run_dgrad_fused
        run_dgrad_fused(L, BF16, c, 1, True, tile=256, tag="dense grid, default code", off=(8, 24), extra=(8, 8))
    else:
        run_dgrad(L, BF16, c, with_add=form == "addsrc", tile=192, tag="dense grid, default code")
    census_assert()


@pytest.mark.parametrize("pc", X.PROD_CASES, ids=lambda pc: pc["id"])
def test_i_production_forms(pc):
    """helpers/conv_exact.py PROD_CASES: the instantiations the production plans launch and no other table reaches, each at the smallest geometry found"""
    L = VariantLib()
    c = X.prod_refs(pc)
    off, ex = ((8, 24), (8, 8)) if pc.get("slices") else ((0, 0), (0, 0))
    with (variant(L, pc["code"]) if pc["code"] else contextlib.nullcontext()):     # 0: the default dispatch, no variant code in the call
        if "f" in pc["run"]:
            run_fwd(L, BF16, c, off, ex, tile=256, tag=pc["id"])
        if "d" in pc["run"]:
            run_dgrad(L, BF16, c, off, ex, tile=256, tag=pc["id"])
        if "b" in pc["run"]:
            run_dgrad_fused(L, BF16, c, 1, True, tile=256, tag=pc["id"])
    census_assert()


@pytest.mark.parametrize("case,code", X.AFFINE_PROD_CASES, ids=str)
def test_i_affine_production(case, code):
    """the inference epilogue on the tiles the 608^2 detector and KeypointNet inference run (x, the residual and the output are channel slices, as in group G)"""
    _affine_act(case, BF16, code)
    census_assert()


@pytest.mark.parametrize("case", X.WGRAD_STREAM_PROD, ids=str)
def test_i_wgrad_stream_production(case):
    L = VariantLib()
    c = plain(stream10(case))
    run_wgrad(L, BF16, c, 1, tag="default")
    run_wgrad(L, BF16, c, 0, (8, 16), (16, 0), tag="x and dy as channel slices")
    census_assert()


@pytest.mark.parametrize("case", X.PW_PROD_CASES, ids=str)
def test_i_pw_forward_production(case):
    _pw_forward(case)
    census_assert()


@pytest.mark.parametrize("case", X.PWB_PROD_CASES, ids=str)
def test_i_pw_backward_production(case):
    _pw_backward(case, True)
    census_assert()


def test_i_dense_wrong_kernel_would_fail():
    """test_a_wrong_kernel_would_fail on the dense grid: weights with the last 8-channel chunk of one tap zeroed must NOT compare equal to the true
    reference, while they do equal the mutated one (= the true one minus that chunk's term, a 1/36 of the reference's cost)."""
    L = VariantLib()
    c = X.dense_refs(X.DENSE_FWD)
    B, Ci, H, W, Co, k, s, p, d = c["geom"]
    w = c["w"].clone()
    w[:, Ci - 8:, k - 1, k // 2] = 0
    wt = torch.zeros(Co, 8, k, k, dtype=torch.float64)
    wt[:, :, k - 1, k // 2] = c["w"][:, Ci - 8:, k - 1, k // 2]
    ym = c["_y"] - torch.nn.functional.conv2d(c["x"][:, Ci - 8:], wt, None, padding=p)
    assert int((ym != c["_y"]).sum()) > 0
    cm = dict(c, w=w, _y=ym)
    run_fwd(L, BF16, cm, tile=192)
    with pytest.raises(AssertionError, match="elements differ"):
        run_fwd(L, BF16, dict(cm, _y=c["_y"]), stats=False, tile=192)
    census_assert()
