// Host side of the conv family: the C ABI of mdcv_conv2d and its variants (forward, data gradient, fused statistics / BatchNorm sums, inference
// epilogue) and of the weight gradients.  Nothing here runs on the GPU: conv2d_impl chooses between the implicit-GEMM kernels (conv_gemm.h) and the
// 3x3 shift kernel (conv_shift.hip); choose_wgrad_family chooses between the weight-gradient kernel families (wgrad_stream.hip, wgrad_shift.hip,
// wgrad_stream_s2.hip, wgrad_gemm.hip), whose slabs wgrad_reduce.hip sums.
#include "conv_gemm.h"
#include "conv_shift.h"
#include "wgrad_gemm.h"
#include "wgrad_shift.h"
#include "wgrad_stream.h"

extern "C" {

static int conv2d_impl(int dtype, int mode, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc,
                       const float* bias, const void* addsrc, int add_ldc, float* stats_partial,
                       int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout,
                       int KH, int KW, int stride, int pad, int dil, const BnFuseArgs* fuse, void* stream, const EpiArgs* epi = nullptr,
                       const XAccArgs* xacc = nullptr) {
  if (!in || !w_packed || !out) return MDCV_EARG;
  if (xacc && (mode != 0 || stats_partial || fuse || epi || !xacc->acc || xacc->reps < 1 || (xacc->reps & (xacc->reps - 1)))) return MDCV_EARG;
  if (epi && (mode != 0 || stats_partial || fuse)) return MDCV_EARG;        // the inference epilogue is a forward-only, statistics-free path
  if ((Cin & 7) || (Nout & 7) || (in_ldc & 7) || (out_ldc & 7) || (addsrc && (add_ldc & 7))) return MDCV_EARG;
  if (stride != 1 && stride != 2) return MDCV_EARG;
  if (mode != 0 && mode != 1) return MDCV_EARG;
  ConvArgs a;
  a.in = in; a.w = w_packed; a.out = out; a.bias = bias; a.addsrc = addsrc; a.stats = stats_partial;
  a.in_ldc = in_ldc; a.out_ldc = out_ldc; a.add_ldc = add_ldc;
  a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.Hout = Hout; a.Wout = Wout; a.Nout = Nout;
  a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.dil = dil;
  a.M = B * Hout * Wout; a.Ktot = KH * KW * Cin; a.tiles_n = 0; a.sshift = stride == 2 ? 1 : 0; a.tiles_total = 0; a.xcd_chunk = 0;
  a.ph = a.pw = a.kh0 = a.kw0 = 0; a.Hs = Hout; a.Ws = Wout; a.nkh = KH; a.nkw = KW; a.cls_split = 0;
  a.fuse = fuse ? *fuse : BnFuseArgs{};
  a.epi = epi ? *epi : EpiArgs{nullptr, 0, 0.f};
  a.xacc = xacc ? *xacc : XAccArgs{nullptr, 1};
  if (a.M <= 0) return MDCV_OK;
  hipStream_t st = (hipStream_t)stream;
  // stride-2 data gradient: 4 launches, one per output-parity class, each visiting only its live taps (no masked MACs)
  const int es = dtype == MDCV_BF16 ? 2 : 4;
  const bool small = conv_operands_small((long long)B * Hin * Win * in_ldc * es, (long long)Nout * KH * KW * Cin * es);
  if (mode == 1 && stride == 2 && dil == 1 && small && (TUNE().conv_variant != 0 || fuse)) {
    // 32- / 64-channel outputs (208 -> 416, 104 -> 208: HBM-bound): the shift kernel's stride-2 form, whole output rows per store (conv_shift.hip MODE 3)
    if (!bias && KH == 3 && KW == 3 && pad == 1 && Hout == 2 * Hin && Wout == 2 * Win && TUNE().conv_variant < 0 &&
        mdcv_shift_s2_dgrad_eligible(dtype, B, Hin, Win, Cin, Nout, in_ldc))
      return mdcv_shift_conv(3, in, in_ldc, w_packed, out, out_ldc, nullptr, addsrc, add_ldc, nullptr, B, Hin, Win, Cin, Nout, fuse, st, nullptr, 1);
    if (TUNE().conv_s2_allcls && dtype == MDCV_BF16 && KH == 3 && KW == 3 && pad == 1 && !(Hout & 1) && !(Wout & 1) && (Cin % 32) == 0 && TUNE().conv_deep_s2 &&
        TUNE().conv_tall_s2) {
      ConvArgs c = a;                              // every class: Hs x Ws = Hout/2 x Wout/2 positions; taps and Ktot are set per class in the kernel
      c.Hs = Hout / 2; c.Ws = Wout / 2;
      c.M = B * c.Hs * c.Ws;
      c.fuse.row_base = 0;
      const int rc = mdcv_cd_bf16_s2_all(c, st, B);
      if (rc != MDCV_EARG) return rc;              // (geometries without an all-class instantiation fall through to the four launches)
    }
    int row_base = 0;
    for (int cls = 0; cls < 4; ++cls) {
      ConvArgs c = a;
      c.ph = cls >> 1; c.pw = cls & 1;
      c.Hs = (Hout - c.ph + 1) / 2; c.Ws = (Wout - c.pw + 1) / 2;
      c.kh0 = (c.ph + pad) & 1; c.kw0 = (c.pw + pad) & 1;
      c.nkh = (KH - c.kh0 + 1) / 2; c.nkw = (KW - c.kw0 + 1) / 2;
      c.M = B * c.Hs * c.Ws;
      c.Ktot = c.nkh * c.nkw * Cin;
      if (c.M <= 0) continue;
      c.fuse.row_base = row_base;                 // (fused BatchNorm sums: one partial row per 128 pixels of each parity class)
      row_base += cdiv(c.M, 128);
      int rc;
      if (c.nkh <= 0 || c.nkw <= 0) { c.nkh = c.nkh > 0 ? c.nkh : 0; c.nkw = c.nkw > 0 ? c.nkw : 0; c.Ktot = 0; }
      if (dtype == MDCV_BF16) rc = mdcv_cd_bf16_s2(c, st, B);
      else if (dtype == MDCV_F32) rc = mdcv_cd_f32_s2(c, st, B);
      else return MDCV_EARG;
      if (rc) return rc;
    }
    return MDCV_OK;
  }
  // 3x3 / stride 1 / pad 1 on wide layers: nine shifted GEMMs over one LDS-resident activation chunk (conv_shift.hip)
  const bool shift_ok = Hin == Hout && Win == Wout && mdcv_shift_eligible(dtype, B, Hout, Wout, Cin, Nout, KH, KW, stride, pad, dil, in_ldc);
  if (shift_ok && (TUNE().conv_variant < 0 || fuse))
    return mdcv_shift_conv(mode, in, in_ldc, w_packed, out, out_ldc, bias, addsrc, add_ldc, stats_partial, B, Hout, Wout, Cin, Nout, fuse, st, epi, dil, xacc);
  if (fuse) {                                     // the fused store loop lives in the LDS-DMA kernels: never fall back to the staged ones
    if (!small) return MDCV_EARG;
    MdcvTune t2 = TUNE();
    if (t2.conv_variant >= 0 && t2.conv_variant < 6) t2.conv_variant = -1;
    const TuneScope lds_dma_only(t2);
    return dtype == MDCV_BF16 ? mdcv_cd_bf16_dgrad(a, st, B) : (dtype == MDCV_F32 ? mdcv_cd_f32_dgrad(a, st, B) : MDCV_EARG);
  }
  if (shift_ok && stats_partial) {   // forced generic kernel on a shift-eligible geometry (A/B runs): the caller sized the partial
    const int r0 = cdiv(a.M, 128), r1 = mdcv_shift_fwd_stats_rows(B, Hout, Wout, Nout, dil);   // rows for the shift kernel; zero the unused tail
    if (r1 > r0) {
      hipError_t e = hipMemsetAsync(stats_partial + (size_t)r0 * 2 * Nout, 0, (size_t)(r1 - r0) * 2 * Nout * sizeof(float), st);
      if (e != hipSuccess) return (int)e;
    }
  }
  if (dtype == MDCV_BF16) return mode == 0 ? mdcv_cd_bf16_fwd(a, st, B) : mdcv_cd_bf16_dgrad(a, st, B);
  if (dtype == MDCV_F32) return mode == 0 ? mdcv_cd_f32_fwd(a, st, B) : mdcv_cd_f32_dgrad(a, st, B);
  return MDCV_EARG;
}

int mdcv_conv2d(int dtype, int mode, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc,
                const float* bias, const void* addsrc, int add_ldc, float* stats_partial,
                int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout,
                int KH, int KW, int stride, int pad, int dil, void* stream) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  return conv2d_impl(dtype, mode, in, in_ldc, w_packed, out, out_ldc, bias, addsrc, add_ldc, stats_partial, B, Hin, Win, Cin, Hout, Wout, Nout,
                     KH, KW, stride, pad, dil, nullptr, stream);
}

// Forward conv whose BatchNorm statistics (per output channel: sum, sum of squares) are ADDED to exact accumulators (exact_acc.h:
// [reps][3][2][Nout] 64-bit words, zero before the launch; mdcv_xstats_words) instead of written as partial rows.  Every forward kernel takes
// it (both dtypes); the consumer (mdcv_bn_act_fwd_xstats) finishes the statistics in its prologue and no finalize launch runs in between.
int mdcv_xstats_words(int reps, int C) { return reps * XACC_DIGITS * 2 * C; }
int mdcv_conv2d_xstats(int dtype, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc, const float* bias, void* xacc,
                       int reps, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride, int pad, int dil,
                       void* stream) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  const XAccArgs x{reinterpret_cast<long long*>(xacc), reps};
  return conv2d_impl(dtype, 0, in, in_ldc, w_packed, out, out_ldc, bias, nullptr, 0, nullptr, B, Hin, Win, Cin, Hout, Wout, Nout, KH, KW,
                     stride, pad, dil, nullptr, stream, nullptr, &x);
}

/* Inference forward: out = act(conv(in) * scale[n] + shift[n]) (+ addsrc).  BatchNorm with running statistics (scale/shift from
 * mdcv_bn_eval_coeffs) and the activation run in the conv's store path: the raw conv output never goes to HBM. */
int mdcv_conv2d_affine_act(int dtype, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc, const float* scale,
                           const float* shift, const void* addsrc, int add_ldc, int act, float slope, int B, int Hin, int Win, int Cin,
                           int Hout, int Wout, int Nout, int KH, int KW, int stride, int pad, int dil, void* stream) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  if (act < 0 || act > 2) return MDCV_EARG;
  const EpiArgs e{scale, act, slope};
  return conv2d_impl(dtype, 0, in, in_ldc, w_packed, out, out_ldc, shift, addsrc, add_ldc, nullptr, B, Hin, Win, Cin, Hout, Wout, Nout,
                     KH, KW, stride, pad, dil, nullptr, stream, &e);
}

// Data gradient (mode 1 of mdcv_conv2d, same geometry arguments) that ALSO writes the BatchNorm-backward partial sums of the
// layer that produced the tensor whose gradient this is:  partial[row][0][c] = sum g, partial[row][1][c] = sum g*(y - mean),
// g = dz * act'(scale*y + shift), one row per 128 output positions.  rows() returns how many rows are written for a geometry,
// or 0 when this geometry cannot take the fused path (the caller then keeps mdcv_conv2d + mdcv_bn_act_bwd_reduce).
int mdcv_conv2d_dgrad_bnsums_rows(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride,
                                  int pad, int dil, int in_ldc) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  const int es = 2;
  if (dtype != MDCV_BF16) return 0;     // production dtype only: not every fp32 tile variant carries the fused store loop
  if (!conv_operands_small((long long)B * Hin * Win * in_ldc * es, (long long)Nout * KH * KW * Cin * es)) return 0;
  if (Hin == Hout && Win == Wout && mdcv_shift_eligible(dtype, B, Hout, Wout, Cin, Nout, KH, KW, stride, pad, dil, in_ldc))
    return mdcv_shift_stats_rows(B, Hout, Wout, dil, Nout);
  if (stride == 2 && dil == 1 && KH == 3 && KW == 3 && pad == 1 && Hout == 2 * Hin && Wout == 2 * Win && TUNE().conv_variant < 0 &&
      mdcv_shift_s2_dgrad_eligible(dtype, B, Hin, Win, Cin, Nout, in_ldc))
    return mdcv_shift_s2_rows(B, Hin, Win);             // the shift kernel's stride-2 form: one row per tile of 8 x 31 dY positions
  if (stride == 2 && dil == 1) {
    int rows = 0;
    for (int cls = 0; cls < 4; ++cls) {
      const int ph = cls >> 1, pw = cls & 1;
      const int m = B * ((Hout - ph + 1) / 2) * ((Wout - pw + 1) / 2);
      if (m > 0) rows += cdiv(m, 128);
    }
    return rows;
  }
  return cdiv(B * Hout * Wout, 128);
}

int mdcv_conv2d_dgrad_bnsums(int dtype, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc, const void* addsrc,
                             int add_ldc, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride,
                             int pad, int dil, const void* y, int ldy, const float* scale, const float* shift, const float* mean, int act,
                             float slope, float* partial, void* stream) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  if (!y || !scale || !shift || !mean || !partial || (ldy & 7)) return MDCV_EARG;
  if (mdcv_conv2d_dgrad_bnsums_rows(dtype, B, Hin, Win, Cin, Hout, Wout, Nout, KH, KW, stride, pad, dil, in_ldc) <= 0) return MDCV_EARG;
  BnFuseArgs f;
  f.y = y; f.scale = scale; f.shift = shift; f.mean = mean; f.partial = partial; f.ldy = ldy; f.act = act; f.row_base = 0;
  f.slope = act == 2 ? 0.f : slope;
  return conv2d_impl(dtype, 1, in, in_ldc, w_packed, out, out_ldc, nullptr, addsrc, add_ldc, nullptr, B, Hin, Win, Cin, Hout, Wout, Nout,
                     KH, KW, stride, pad, dil, &f, stream);
}

// 1 when the data gradient of this geometry runs as the stride-2 form of the 3x3 shift kernel (conv_shift.hip MODE 3: whole output rows from LDS,
// one partial row of fused sums per 8 x 31 tile): the plan fuses the BatchNorm-backward sums into it at every size.
int mdcv_conv2d_dgrad_s2_form_ok(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride,
                                 int pad, int dil, int in_ldc) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  return dtype == MDCV_BF16 && stride == 2 && dil == 1 && KH == 3 && KW == 3 && pad == 1 && Hout == 2 * Hin && Wout == 2 * Win &&
         TUNE().conv_variant < 0 && (long long)B * Hin * Win * in_ldc * 2 < (1LL << 31) &&
         mdcv_shift_s2_dgrad_eligible(dtype, B, Hin, Win, Cin, Nout, in_ldc);
}

// number of rows of the [rows][2][Nout] BatchNorm partial-statistics buffer mdcv_conv2d writes (one per 128 output pixels)
int mdcv_conv2d_stats_rows(int M) { return cdiv(M, 128); }
// rows for a given forward geometry: the 3x3 stride-1 shift kernel walks a padded position stream and writes more rows
int mdcv_conv2d_stats_rows_geom(int dtype, int B, int Hout, int Wout, int Cin, int Nout, int KH, int KW, int stride, int pad, int dil,
                                int in_ldc) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_CONV);
  if (mdcv_shift_eligible(dtype, B, Hout, Wout, Cin, Nout, KH, KW, stride, pad, dil, in_ldc)) return mdcv_shift_fwd_stats_rows(B, Hout, Wout, Nout, dil);
  return cdiv(B * Hout * Wout, 128);
}

// choose the pixel split of the weight-gradient kernel; returns the number of fp32 slabs.
// ~2 blocks per CU in flight, but never less than 4 steps (512 bf16 pixels) per split so the fp32 epilogue stays amortised.
int mdcv_conv2d_wgrad_splits(int dtype, int M, int Cout, int Ktot) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_WGRAD);
  const int bp = dtype == MDCV_BF16 ? 128 : 64;
  const int tiles = cdiv(Cout, 128) * cdiv(Ktot, 128);
  const int slots = TUNE().wgrad_slots;   // resident blocks: 2 per CU (wide tile 66 KiB; narrow tile 4 x 20 KiB ring)
  int s = slots / tiles;                  // never spill into a second, nearly empty round
  const int max_s = cdiv(M, bp * 4);
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  int pps = cdiv(cdiv(M, s), bp) * bp;
  return cdiv(M, pps);
}

// ---- which kernel family takes a weight gradient.  The candidates in their fixed order: the 7x7 stem, the LDS-ring kernel for 16..128-channel 3x3
// layers, the kw-shared-tile kernel, the stride-2 parity-plane kernel, and the generic kernels, which take everything.
//   * mdcv_conv2d_wgrad_splits_geom and mdcv_conv2d_wgrad_bnapply_ok take the FIRST ELIGIBLE family (splits == 0 below).
//   * mdcv_conv2d_wgrad takes the first eligible family WHOSE *_splits_ok ACCEPTS THE CALLER'S `splits` and otherwise moves on down the list: a caller
//     that sized `ws` with the geometry-blind mdcv_conv2d_wgrad_splits gets the generic kernel, not an error, and a workspace sized by splits_geom is
//     written by the very family that sized it.
// A new family is one more enumerator, in its place in the order, and one case in each of the three switches below.
enum WgradFamily { WG_STEM, WG_STREAM, WG_SHIFT, WG_S2, WG_GENERIC };

// wgrad_variant 9 keeps every layer on the generic kernels, 10 all but the kw-shared-tile kernel's; 8 and 11 widen that kernel's share (below)
static bool wgrad_eligible(WgradFamily f, const WgradGeom& g) {
  const int v = TUNE().wgrad_variant;
  if (f == WG_GENERIC) return true;
  if (v == 9 || (v == 10 && f != WG_SHIFT)) return false;
  const bool same = g.Hin == g.Hout && g.Win == g.Wout;
  switch (f) {
    case WG_STEM:     // 7x7 stem with the input padded to 16 channels: LDS-ring kernel
      return same && mdcv_wgrad_stem_eligible(g.dtype, g.B, g.Hout, g.Wout, g.Cin, g.Cout, g.KH, g.KW, g.stride, g.pad, g.dil, g.dy_ldc, g.x_ldc);
    case WG_STREAM:   // 16..128-channel 3x3 stride-1 layers (dilation 1 or 2): all nine taps read one activation window kept in an LDS ring (wgrad_stream.hip)
      return same && mdcv_wgrad_stream_eligible(g.dtype, g.B, g.Hout, g.Wout, g.Cin, g.Cout, g.KH, g.KW, g.stride, g.pad, g.dil, g.dy_ldc, g.x_ldc);
    case WG_S2:       // 3x3 / stride-2 down-sampling layers: the input's four parity planes as one LDS ring (wgrad_stream_s2.hip)
      return mdcv_wgrad_s2_eligible(g.dtype, g.B, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.Cout, g.KH, g.KW, g.stride, g.pad, g.dil, g.dy_ldc, g.x_ldc);
    default: break;
  }
  // WG_SHIFT: 3x3 / stride 1 / pad 1 with 128-multiple channel counts: the three kw taps of a kernel row share one activation tile.
  // The kw-shared-tile kernel (wgrad_shift.hip) is used where it measured faster than the generic one on MI355X inside the
  // training step: long pixel runs per block (>= 128 steps of 64 positions, i.e. RektNet's 80x80 layers: 740 -> 680 us).
  // On YOLOv3's 52x52 / 26x26 layers at batch 32 the generic kernel's larger grid wins by 5-10%; on 13x13 512->1024 the new
  // kernel is faster alone (126 -> 116 us) but the step is 0.5% slower with it (one fat block per CU leaves less room for the
  // main stream's kernels that run beside the weight gradients).  Variant 8 forces it wherever eligible, 9 disables it.
  if (!same || !mdcv_wgrad_shift_eligible(g.dtype, g.B, g.Hout, g.Wout, g.Cin, g.Cout, g.KH, g.KW, g.stride, g.pad, g.dil, g.dy_ldc, g.x_ldc)) return false;
  if (v == 8) return true;
  const long long Mq = (long long)g.B * (g.Hout + 1) * (g.Wout + 1);
  const int s = mdcv_wgrad_shift_splits(g.B, g.Hout, g.Wout, g.Cin, g.Cout);
  if (Mq / (64LL * s) >= 128) return true;
  return v == 11 && mdcv_conv2d_wgrad_splits(g.dtype, g.B * g.Hout * g.Wout, g.Cout, g.KH * g.KW * g.Cin) == 1;   // A/B: also the split-less layers
}

static int wgrad_family_splits(WgradFamily f, const WgradGeom& g) {
  switch (f) {
    case WG_STEM:   return mdcv_wgrad_stem_splits(g.B, g.Hout, g.Wout);
    case WG_STREAM: return mdcv_wgrad_stream_splits(g.B, g.Hout, g.Wout, g.Cin, g.Cout, g.dil);
    case WG_SHIFT:  return mdcv_wgrad_shift_splits(g.B, g.Hout, g.Wout, g.Cin, g.Cout);
    case WG_S2:     return mdcv_wgrad_s2_splits(g.B, g.Hout, g.Wout, g.Cin, g.Cout);
    default:        return mdcv_conv2d_wgrad_splits(g.dtype, g.B * g.Hout * g.Wout, g.Cout, g.KH * g.KW * g.Cin);
  }
}

static bool wgrad_family_splits_ok(WgradFamily f, const WgradGeom& g, int splits) {
  switch (f) {
    case WG_STEM:   return mdcv_wgrad_stem_splits_ok(splits, g.B, g.Hout, g.Wout);
    case WG_STREAM: return mdcv_wgrad_stream_splits_ok(splits, g.B, g.Hout, g.Wout, g.Cin, g.Cout, g.dil);
    case WG_SHIFT:  return mdcv_wgrad_shift_splits_ok(splits, g.B, g.Hout, g.Wout);
    case WG_S2:     return mdcv_wgrad_s2_splits_ok(splits, g.B, g.Hout, g.Wout);
    default:        return true;          // (the generic launch checks its own split, launch_wgrad_gemm)
  }
}

// splits == 0: the first eligible family; splits >= 1: the first eligible family that can run with this many slabs
static WgradFamily choose_wgrad_family(const WgradGeom& g, int splits) {
  for (int f = WG_STEM; f < WG_GENERIC; ++f)
    if (wgrad_eligible((WgradFamily)f, g) && (splits == 0 || wgrad_family_splits_ok((WgradFamily)f, g, splits))) return (WgradFamily)f;
  return WG_GENERIC;
}

// geometry-aware variant: the kernel mdcv_conv2d_wgrad will pick for this layer decides the split (use this one to size `ws`)
int mdcv_conv2d_wgrad_splits_geom(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int KH, int KW, int stride,
                                  int pad, int dil, int dy_ldc, int x_ldc) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_WGRAD);
  const WgradGeom g{dtype, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dil, dy_ldc, x_ldc};
  return wgrad_family_splits(choose_wgrad_family(g, 0), g);
}

int mdcv_conv2d_wgrad(int dtype, const void* dy, int dy_ldc, const void* x, int x_ldc, float* ws, int splits,
                      float* dw_oihw, int accumulate, int B, int Hin, int Win, int Cin, int Cin_real,
                      int Hout, int Wout, int Cout, int Cout_real, int KH, int KW, int stride, int pad, int dil, void* stream) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_WGRAD);
  if (!dy || !x || !ws || !dw_oihw) return MDCV_EARG;
  if ((Cin & 7) || (Cout & 7) || (dy_ldc & 7) || (x_ldc & 7) || splits < 1) return MDCV_EARG;
  const WgradGeom g{dtype, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dil, dy_ldc, x_ldc};
  hipStream_t st = (hipStream_t)stream;
  int rc, KK = 9, wrote_dw = 0;
  switch (choose_wgrad_family(g, splits)) {
    case WG_STEM:   KK = 49; rc = mdcv_wgrad_stem(dy, dy_ldc, x, x_ldc, ws, splits, B, Hout, Wout, st); break;
    case WG_STREAM: rc = mdcv_wgrad_stream(dy, dy_ldc, x, x_ldc, ws, splits, B, Hout, Wout, Cin, Cout, dil, st, dw_oihw, Cin_real, Cout_real, accumulate,
                                           &wrote_dw); break;
    case WG_SHIFT:  rc = mdcv_wgrad_shift(dy, dy_ldc, x, x_ldc, ws, splits, B, Hout, Wout, Cin, Cout, st); break;
    case WG_S2:     rc = mdcv_wgrad_s2(dy, dy_ldc, x, x_ldc, ws, splits, B, Hout, Wout, Cin, Cout, st); break;
    default:        KK = KH * KW; rc = launch_wgrad_gemm(g, dy, x, ws, splits, st); break;
  }
  if (rc || wrote_dw) return rc;                             // (the slab-free form of the LDS-ring kernel wrote the OIHW gradient itself)
  return launch_wgrad_reduce(ws, dw_oihw, splits, Cout, Cout_real, Cin, Cin_real, KK, accumulate, st);
}

// ---- weight gradient of a conv -> BatchNorm -> activation layer whose INPUT needs no gradient (the first layer), straight from (dz, y): the
// BatchNorm-backward apply pass is folded into the operand load of the narrow kernel (conv_wgrad_dma_narrow_kernel BNA, wgrad_gemm.hip).  _ok() = 1 when
// the geometry takes that kernel (bf16, Cout_pad <= 32, not one of the other families); splits = mdcv_conv2d_wgrad_splits_geom of the same geometry.
int mdcv_conv2d_wgrad_bnapply_ok(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int KH, int KW, int stride,
                                 int pad, int dil, int dz_ldc, int y_ldc, int x_ldc) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_WGRAD);
  if (dtype != MDCV_BF16 || Cout > 32 || (Cin & 7) || (Cout & 7) || (dz_ldc & 7) || (y_ldc & 7) || (x_ldc & 7) || TUNE().wgrad_variant != 0) return 0;
  const WgradGeom g{dtype, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dil, dz_ldc, x_ldc};
  if (choose_wgrad_family(g, 0) != WG_GENERIC) return 0;
  const long long M = (long long)B * Hout * Wout;
  const int ldmax = dz_ldc > y_ldc ? dz_ldc : y_ldc;
  return M * ldmax * 2 < (1LL << 31) && (long long)B * Hin * Win * x_ldc * 2 < (1LL << 31) && TUNE().conv_variant != 0 &&
         (long long)B * Hin * Win + 256 < (1LL << 24) && M + 256 < (1 << 24) && Wout >= 8 && x_ldc < (1 << 23) && ldmax < (1 << 23);
}
int mdcv_conv2d_wgrad_bnapply(int dtype, const void* dz, int dz_ldc, const void* y, int y_ldc, const float* scale, const float* shift,
                              const float* cA, const float* cB, const float* cC, int act, float slope, const void* x, int x_ldc, float* ws,
                              int splits, float* dw_oihw, int accumulate, int B, int Hin, int Win, int Cin, int Cin_real, int Hout, int Wout,
                              int Cout, int Cout_real, int KH, int KW, int stride, int pad, int dil, void* stream) {
  MDCV_TUNE_ENTRY(dtype, MDCV_TUNE_WGRAD);
  if (!dz || !y || !scale || !shift || !cA || !cB || !cC || !x || !ws || !dw_oihw || splits < 1) return MDCV_EARG;
  if (!mdcv_conv2d_wgrad_bnapply_ok(dtype, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dil, dz_ldc, y_ldc, x_ldc)) return MDCV_EARG;
  const WgradGeom g{dtype, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dil, dz_ldc, x_ldc};
  const int rc = launch_wgrad_gemm_bnapply(g, dz, y, y_ldc, scale, shift, cA, cB, cC, act, slope, Cout_real, x, ws, splits, (hipStream_t)stream);
  if (rc) return rc;
  return launch_wgrad_reduce(ws, dw_oihw, splits, Cout, Cout_real, Cin, Cin_real, KH * KW, accumulate, (hipStream_t)stream);
}

}  // extern "C"
