// NHWC implicit-GEMM convolution kernels for gfx950 (MFMA), forward and data gradient: the register-staged conv_igemm_kernel, the LDS-DMA
// conv_glds_kernel, their launchers and the tile dispatch.  Included by the three units that instantiate them (conv_gemm_bf16_fwd.hip,
// conv_gemm_bf16_dgrad.hip, conv_gemm_f32.hip) and by the host unit conv_igemm.hip, which fills ConvArgs and calls the mdcv_cd_* functions.
//
// Replaces the nn.Conv2d calls on the reference hot path (CVC-YOLOv3/models.py:59-65,
// RektNet/keypoint_net.py:17,25, RektNet/resnet.py:12-19) and their autograd backward.
//
// GEMM view (fwd):   Y[m, n] = sum_k  Xcol[m, k] * W[n, k]      m = (img, ho, wo)   n = cout   k = (kh, kw, ci)
//      (dgrad):      dX[m, n] = sum_k dYcol[m, k] * Wt[n, k]    m = (img, hi, wi)   n = cin    k = (kh, kw, co)
//      (wgrad):      dW[co, k] = sum_m dY[m, co] * Xcol[m, k]   reduction over pixels, split over the grid (wgrad_gemm.hip)
//
// Activations are NHWC with an explicit channel stride (ldc) so route-concat is a strided write, channels padded
// to a multiple of 8 (pad lanes are exactly zero).  Element type T is bf16 (production: v_mfma_f32_16x16x32_bf16)
// or fp32 (parity mode: v_mfma_f32_16x16x4_f32, bit-exact fmaf chains).  Accumulation is always fp32.
//
// Tiling: 256 threads = 4 waves; K tile = 64 bytes per row (32 bf16 / 16 fp32); global->register->LDS staging with
// the next tile's loads issued before the current tile's MFMAs (one barrier per K tile, 2 LDS buffers);
// LDS rows padded to 80 bytes; epilogue staged through LDS for 16-byte coalesced stores; BatchNorm batch statistics
// (sum, sum of squares per output channel) are produced from the fp32 accumulators in the epilogue.
#pragma once
#include "common.h"
#include "bn_fuse.h"
#include "exact_acc.h"

struct ConvArgs {
  const void* in; const void* w; void* out; const float* bias; const void* addsrc; float* stats;
  int in_ldc, out_ldc, add_ldc;
  int Hin, Win, Cin, Hout, Wout, Nout;
  int KH, KW, stride, pad, dil;
  int M, Ktot, tiles_n, sshift, tiles_total, xcd_chunk;
  int ph, pw, Hs, Ws, kh0, kw0, nkh, nkw;     // MODE 2 (stride-2 data gradient, one output-parity class per launch)
  int cls_split;                              // ALLCLS: 1 = two workgroups per tile, the 4-tap class and the 1+2+2-tap classes (sparse grids)
  BnFuseArgs fuse;                            // BatchNorm-backward sums folded into the store loop of a data gradient (fuse.y == NULL: off)
  EpiArgs epi;                                // inference epilogue act(acc * oscale + bias) (oscale == NULL and act == 0: off)
  XAccArgs xacc;                              // forward statistics added to exact accumulators instead of written as rows (exact_acc.h; acc == NULL: off)
};

// the dispatch entry points, each defined by exactly one of the instantiation units (conv_gemm_bf16_fwd.hip, conv_gemm_bf16_dgrad.hip, conv_gemm_f32.hip)
int mdcv_cd_bf16_fwd(const ConvArgs& a, hipStream_t st, int B);
int mdcv_cd_bf16_dgrad(const ConvArgs& a, hipStream_t st, int B);
int mdcv_cd_bf16_s2(const ConvArgs& a, hipStream_t st, int B);
int mdcv_cd_bf16_s2_all(const ConvArgs& a, hipStream_t st, int B);
int mdcv_cd_f32_fwd(const ConvArgs& a, hipStream_t st, int B);
int mdcv_cd_f32_dgrad(const ConvArgs& a, hipStream_t st, int B);
int mdcv_cd_f32_s2(const ConvArgs& a, hipStream_t st, int B);

// the LDS-DMA kernels address operands through 32-bit buffer offsets: both operands (activation and weight bytes) must be < 2 GiB
inline bool conv_operands_small(long long in_bytes, long long w_bytes) { return in_bytes < (1LL << 31) && w_bytes < (1LL << 31); }

namespace {

// One K tile of MFMAs for a wave: FM x FN fragments of 16x16, KT k-steps of 64 bytes per LDS row (row pitch RB bytes).
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
  template <int FM, int FN, int KT, int RB>
  __device__ static __forceinline__ void mma(const unsigned char* sa, const unsigned char* sb, int lane, f32x4_t (&acc)[FM][FN]) {
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      bf16x8_t a[FM], b[FN];
      const int off = (lane & 15) * RB + ks * 64 + (lane >> 4) * 16;
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(sa + i * 16 * RB + off);
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(sb + j * 16 * RB + off);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
};
template <> struct Frag<float> {
  template <int FM, int FN, int KT, int RB>
  __device__ static __forceinline__ void mma(const unsigned char* sa, const unsigned char* sb, int lane, f32x4_t (&acc)[FM][FN]) {
#pragma unroll
    for (int ks = 0; ks < 4 * KT; ++ks) {
      float a[FM], b[FN];
      const int off = (lane & 15) * RB + (ks * 4 + (lane >> 4)) * 4;
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const float*>(sa + i * 16 * RB + off);
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const float*>(sb + j * 16 * RB + off);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
};

// MODE 0: forward gather  hi = ho*stride - pad + kh*dil
// MODE 1: data gradient   hi = (h + pad - kh*dil) / stride when divisible   (stride is 1 or 2)
// Block = WM x WN waves, tile BM x BN, K tile = KT*64 bytes per row.
template <typename T, int MODE, int BM, int BN, int WM, int WN, int KT>
__global__ __launch_bounds__(WM * WN * 64) void conv_igemm_kernel(ConvArgs a) {
  constexpr int NT = WM * WN * 64;
  constexpr int VEC = ET<T>::VEC;
  constexpr int VPR = 4 * KT;                 // 16-byte vectors per LDS row
  constexpr int BK = VPR * VEC;
  constexpr int RB = 64 * KT + 16;            // LDS row pitch (bytes): +16 keeps ds_read_b128 fragments conflict-light
  constexpr int RPP = NT / VPR;               // tile rows staged per pass
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  constexpr int NPA = BM / RPP, NPB = (BN + RPP - 1) / RPP;
  constexpr int PIPE = 2 * (BM + BN) * RB;
  constexpr int SROW = BN * (int)sizeof(T) + 16;
  constexpr int STAGE = BM * SROW;
  constexpr int STAT_OFF = PIPE > STAGE ? PIPE : STAGE;
  static_assert(BM % RPP == 0, "tile rows must be a multiple of the staging pass");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  // XCD-aware tile order: block b runs on XCD b%8 (observed dispatch); give every XCD one contiguous run of tiles so
  // that the tile_n variants of a row panel and its halo neighbours share that XCD's L2.  Pure speed, not correctness.
  const int logical = (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3);
  if (logical >= a.tiles_total) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tile_m = logical / a.tiles_n, tile_n = logical % a.tiles_n;
  const int arow = tid / VPR, kv = tid % VPR;
  const T* __restrict__ in = reinterpret_cast<const T*>(a.in);
  const T* __restrict__ w = reinterpret_cast<const T*>(a.w);

  // per-row pixel decomposition (fixed for the whole K loop)
  int bh[NPA], bw[NPA], ib[NPA];
  bool rv[NPA];
  const int HWo = a.Hout * a.Wout;
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int m = tile_m * BM + arow + p * RPP;
    rv[p] = m < a.M;
    const int mm = rv[p] ? m : 0;
    const int img = mm / HWo, rem = mm - img * HWo;
    const int ho = rem / a.Wout, wo = rem - ho * a.Wout;
    ib[p] = img * a.Hin * a.Win;
    if (MODE == 0) { bh[p] = ho * a.stride - a.pad; bw[p] = wo * a.stride - a.pad; }
    else           { bh[p] = ho + a.pad;            bw[p] = wo + a.pad; }
  }
  // per-thread K cursor: k = kt*BK + kv*VEC  ->  (kh, kw, c)
  int kc, kh, kw;
  {
    const int k0 = kv * VEC, tap = k0 / a.Cin;
    kc = k0 - tap * a.Cin; kh = tap / a.KW; kw = tap - kh * a.KW;
  }
  const int smask = a.stride - 1;

  uint4 ra[NPA], rb[NPB];
  auto load_tile = [&](int kt) {
    const bool kvalid = kh < a.KH;
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      int hi, wi; bool ok = rv[p] && kvalid;
      if (MODE == 0) { hi = bh[p] + kh * a.dil; wi = bw[p] + kw * a.dil; }
      else {
        const int th = bh[p] - kh * a.dil, tw = bw[p] - kw * a.dil;
        ok = ok && th >= 0 && tw >= 0 && (((th | tw) & smask) == 0);
        hi = th >> a.sshift; wi = tw >> a.sshift;
      }
      ok = ok && (unsigned)hi < (unsigned)a.Hin && (unsigned)wi < (unsigned)a.Win;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ok) v = *reinterpret_cast<const uint4*>(in + ((size_t)(ib[p] + hi * a.Win + wi) * a.in_ldc + kc));
      ra[p] = v;
    }
    const int k = kt * BK + kv * VEC;
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const int brow = arow + p * RPP;
      const int n = tile_n * BN + brow;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (brow < BN && n < a.Nout && k < a.Ktot) v = *reinterpret_cast<const uint4*>(w + ((size_t)n * a.Ktot + k));
      rb[p] = v;
    }
  };
  auto advance = [&]() {
    kc += BK;
    while (kc >= a.Cin) { kc -= a.Cin; if (++kw == a.KW) { kw = 0; ++kh; } }
  };
  auto store_tile = [&](int buf) {
    unsigned char* sA = smem + buf * (BM + BN) * RB;
    unsigned char* sB = sA + BM * RB;
#pragma unroll
    for (int p = 0; p < NPA; ++p) *reinterpret_cast<uint4*>(sA + (arow + p * RPP) * RB + kv * 16) = ra[p];
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const int brow = arow + p * RPP;
      if (brow < BN) *reinterpret_cast<uint4*>(sB + brow * RB + kv * 16) = rb[p];
    }
  };

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.Ktot + BK - 1) / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) { advance(); load_tile(kt + 1); }
    const unsigned char* sA = smem + cur * (BM + BN) * RB + wm * TM * RB;
    const unsigned char* sB = smem + cur * (BM + BN) * RB + BM * RB + wn * TN * RB;
    Frag<T>::template mma<FM, FN, KT, RB>(sA, sB, lane, acc);
    if (kt + 1 < nk) store_tile(cur ^ 1);
    __syncthreads();
  }

  // ---------------- epilogue ----------------
  const int n0 = tile_n * BN + wn * TN, m0 = tile_m * BM + wm * TM;
  if (a.bias) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + j * 16 + (lane & 15);
      const float bv = n < a.Nout ? a.bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += bv;
    }
  }
  float* sstat = reinterpret_cast<float*>(smem + STAT_OFF);   // [WM][2][BN]
  const bool want_stats = a.stats || a.xacc.acc;
  if (want_stats) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + i * 16 + (lane >> 4) * 4 + r;
          const float v = m < a.M ? acc[i][j][r] : 0.f;
          s += v; q += v * v;
        }
      s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
      s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
      if (lane < 16) {
        sstat[(wm * 2 + 0) * BN + wn * TN + j * 16 + lane] = s;
        sstat[(wm * 2 + 1) * BN + wn * TN + j * 16 + lane] = q;
      }
    }
  }
  // stage the tile as T (the K loop ended with a barrier, so the pipeline buffers are free)
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * TM + i * 16 + (lane >> 4) * 4 + r, col = wn * TN + j * 16 + (lane & 15);
        ET<T>::st(reinterpret_cast<T*>(smem + row * SROW) + col, acc[i][j][r]);
      }
  __syncthreads();
  // statistics rows are per 128 pixels regardless of the tile height (one row per group of wave-rows)
  constexpr int G = BM / 128, WPG = WM / G;
  if (want_stats && tid < BN * G) {
    const int g = tid / BN, col = tid - g * BN;
    const int n = tile_n * BN + col, srow = tile_m * G + g;
    if (n < a.Nout && srow * 128 < a.M) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int r = 0; r < WPG; ++r) { s += sstat[((g * WPG + r) * 2 + 0) * BN + col]; q += sstat[((g * WPG + r) * 2 + 1) * BN + col]; }
      if (a.xacc.acc) {                                     // fire-and-forget exact accumulation (exact_acc.h): no rows, no finalize launch
        long long* xp = a.xacc.acc + (size_t)(srow & (a.xacc.reps - 1)) * (XACC_DIGITS * 2) * a.Nout + n;
        xacc_add(xp, 2 * (size_t)a.Nout, s);
        xacc_add(xp + a.Nout, 2 * (size_t)a.Nout, q);
      } else {
        a.stats[((size_t)srow * 2 + 0) * a.Nout + n] = s;
        a.stats[((size_t)srow * 2 + 1) * a.Nout + n] = q;
      }
    }
  }
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const T* __restrict__ addsrc = reinterpret_cast<const T*>(a.addsrc);
  constexpr int VPRO = BN / VEC;
  for (int v = tid; v < BM * VPRO; v += NT) {
    const int row = v / VPRO, cv = v - row * VPRO;
    const int m = tile_m * BM + row, n = tile_n * BN + cv * VEC;
    if (m < a.M && n < a.Nout) {
      uint4 d = *reinterpret_cast<const uint4*>(smem + row * SROW + cv * 16);
      if (addsrc) {
        float x[VEC], y[VEC];
        ET<T>::unpack(d, x);
        ET<T>::unpack(*reinterpret_cast<const uint4*>(addsrc + ((size_t)m * a.add_ldc + n)), y);
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] += y[e];
        d = ET<T>::pack(x);
      }
      *reinterpret_cast<uint4*>(out + ((size_t)m * a.out_ldc + n)) = d;
    }
  }
}

template <typename T, int MODE, int BM, int BN, int WM, int WN, int KT>
int launch_conv(const ConvArgs& a0, hipStream_t st) {
  if (a0.epi.oscale || a0.epi.act) return MDCV_EARG;          // the register-staged kernels carry no inference epilogue

  ConvArgs a = a0;
  constexpr int RB = 64 * KT + 16;
  constexpr int PIPE = 2 * (BM + BN) * RB;
  constexpr int STAGE = BM * (BN * (int)sizeof(T) + 16);
  constexpr int LDS = (PIPE > STAGE ? PIPE : STAGE) + WM * 2 * BN * 4;
  static_assert(LDS <= 160 * 1024, "tile does not fit the 160 KiB LDS");
  static DynLds dyn_lds;
  auto kern = conv_igemm_kernel<T, MODE, BM, BN, WM, WN, KT>;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds, reinterpret_cast<const void*>(kern), LDS); e != hipSuccess) return (int)e;
  a.tiles_n = cdiv(a.Nout, BN);
  a.tiles_total = cdiv(a.M, BM) * a.tiles_n;
  a.xcd_chunk = cdiv(a.tiles_total, 8);
  MDCV_LAUNCH(kern, dim3((unsigned)(a.xcd_chunk * 8)), dim3(WM * WN * 64), LDS, st, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant: tiles go HBM -> LDS directly (buffer_load_dwordx4 ... lds), no VGPR staging and no ds_write pass.
// An LDS-DMA writes lane-linear: 64 lanes x 16 B = one 1 KiB chunk = 16 tile rows of 64 B (4 lanes per row), so rows are NOT
// padded; bank conflicts of the ds_read_b128 fragment reads are removed by swizzling on the SOURCE side instead: the lane that
// fills 16-byte slot s of row r fetches logical k-vector  s ^ f(r),  f(r) = (-(r >> 2)) & 3, and the fragment read of
// k-vector q goes to slot q ^ f(r).  With this f every 16-lane service group of ds_read_b128 touches 16 distinct slots.
// Out-of-image taps / tail rows use an out-of-range buffer offset: the hardware range check returns zeros into LDS.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swz(int row) { return (-(row >> 2)) & 3; }

template <typename T> struct FragSwz;
template <> struct FragSwz<bf16_t> {
  // split form: fragment reads first, MFMAs later, so independent work (DMA address arithmetic) can sit under the LDS latency
  template <int FM, int FN>
  __device__ static __forceinline__ void load(const unsigned char* sa, const unsigned char* sb, int lane, bf16x8_t (&a)[FM], bf16x8_t (&b)[FN]) {
    const int r = lane & 15;
    const int off = r * 64 + (((lane >> 4) ^ swz(r)) << 4);
#pragma unroll
    for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(sa + i * 1024 + off);
#pragma unroll
    for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(sb + j * 1024 + off);
  }
  template <int FM, int FN>
  __device__ static __forceinline__ void compute(const bf16x8_t (&a)[FM], const bf16x8_t (&b)[FN], f32x4_t (&acc)[FM][FN]) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }
  template <int FM, int FN>
  __device__ static __forceinline__ void mma(const unsigned char* sa, const unsigned char* sb, int lane, f32x4_t (&acc)[FM][FN]) {
    bf16x8_t a[FM], b[FN];
    const int r = lane & 15;
    const int off = r * 64 + (((lane >> 4) ^ swz(r)) << 4);
#pragma unroll
    for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(sa + i * 1024 + off);
#pragma unroll
    for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(sb + j * 1024 + off);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  }
};
template <> struct FragSwz<float> {
  template <int FM, int FN>
  __device__ static __forceinline__ void mma(const unsigned char* sa, const unsigned char* sb, int lane, f32x4_t (&acc)[FM][FN]) {
    const int r = lane & 15;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      float a[FM], b[FN];
      const int off = r * 64 + ((ks ^ swz(r)) << 4) + (lane >> 4) * 4;
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const float*>(sa + i * 1024 + off);
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const float*>(sb + j * 1024 + off);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
};

typedef __attribute__((address_space(3))) void lds_void_t;

// ALLCLS (MODE 2 only): the workgroup computes ALL FOUR output-parity classes of its tile of dY positions, one after the other (classes
// have 1, 2, 2 and 4 taps: every workgroup gets the same 9 taps of work, and the dY rows a tile reads come from HBM once instead of
// once per class launch -- 177 MB of dY per launch at 208^2 x 64 channels).  Needs even Hout / Wout (all classes share one Hs x Ws grid).
template <typename T, int MODE, int BM, int BN, int WM, int WN, int STAGES, bool UT, bool FUSE, bool EPI = false, bool ALLCLS = false>
__global__ __launch_bounds__(WM * WN * 64) void conv_glds_kernel(ConvArgs a0, unsigned in_bytes, unsigned w_bytes) {
  constexpr int NW = WM * WN, NT = NW * 64;
  constexpr int VEC = ET<T>::VEC;
  constexpr int BK = 4 * VEC;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  constexpr int CA = BM / 16, CB = BN / 16;               // 1 KiB chunks per operand tile
  constexpr int NPA = (CA + NW - 1) / NW, NPB = (CB + NW - 1) / NW;
  // The deep ring waits with counted vmcnt, so every wave must issue the same number of DMAs per K tile: when an operand tile has
  // fewer 1 KiB chunks than there are waves (32- and 16-channel weight tiles), the surplus waves fill a 1 KiB sink with zeros.
  constexpr bool UNEVEN = STAGES > 2 && (CA % NW != 0 || CB % NW != 0);
  constexpr int SINK = STAGES * (BM + BN) * 64;
  constexpr int PIPE = SINK + (UNEVEN ? 1024 : 0);
  constexpr int GD = NPA + NPB;                           // LDS-DMA instructions every wave issues per K tile (deep pipeline: exact)
  constexpr int SROW = BN * (int)sizeof(T) + 16;
  constexpr int STAGE = BM * SROW;
  constexpr int STAT_OFF = PIPE > STAGE ? PIPE : STAGE;
  constexpr unsigned OOB = 0x80000000u;                   // >= num_records of any descriptor we build (sizes are < 2 GiB)
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];

  static_assert(!ALLCLS || MODE == 2, "ALLCLS is a stride-2 data-gradient form");
  const int logical = (int)(blockIdx.x & 7) * a0.xcd_chunk + (int)(blockIdx.x >> 3);
  if (logical >= a0.tiles_total) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  // ALLCLS with cls_split: the tile's work is cut into two workgroups of 4 and 5 tap-GEMMs -- class (1,1) alone and classes (0,0), (0,1),
  // (1,0) -- that sit next to each other in the launch order (same XCD: the dY rows they both read meet in its L2).  The 26->52 and
  // 13->26 layers at batch 32 give only 338 / 172 tiles of 128 x 128: one workgroup per tile walked its nine tap-GEMMs on a
  // half-empty chip, four class launches did the same one class at a time.
  int tile_id = logical, cls_lo = 0, cls_hi = ALLCLS ? 4 : 1;
  if constexpr (ALLCLS) {
    if (a0.cls_split) { tile_id = logical >> 1; if (logical & 1) cls_hi = 3; else cls_lo = 3; }
  }
  const int tile_m = tile_id / a0.tiles_n, tile_n = tile_id % a0.tiles_n;
  const int lrow = lane >> 2;                              // row inside a chunk this lane fills
  const int kv = (lane & 3) ^ swz(lrow);                   // logical k-vector it fetches for that slot
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a0.in), 0, in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a0.w), 0, w_bytes, 0x00020000);
#pragma unroll 1
  for (int cls = cls_lo; cls < cls_hi; ++cls) {
  ConvArgs a = a0;
  if constexpr (ALLCLS) {                                  // class (ph, pw): its live taps kh = kh0 + 2i, kw = kw0 + 2j (see conv2d_impl)
    a.ph = cls >> 1; a.pw = cls & 1;
    a.kh0 = (a.ph + a.pad) & 1; a.kw0 = (a.pw + a.pad) & 1;
    a.nkh = (a.KH - a.kh0 + 1) / 2; a.nkw = (a.KW - a.kw0 + 1) / 2;
    a.Ktot = a.nkh * a.nkw * a.Cin;
    a.fuse.row_base = cls * ((a.M + 127) >> 7);
    if (cls != cls_lo) __syncthreads();                    // the previous class's epilogue is done with the LDS
  }

  int bh[NPA], bw[NPA], ib[NPA];
  bool rv[NPA];
  // MODE 2 enumerates only the output pixels (h,w) = (ph + 2a, pw + 2b) of one parity class and only the taps whose
  // parity matches (kh = kh0 + 2i, kw = kw0 + 2j): every tap it visits is a real MAC.
  const int HWo = MODE == 2 ? a.Hs * a.Ws : a.Hout * a.Wout;
  const int Wrow = MODE == 2 ? a.Ws : a.Wout;
  const int KWn = MODE == 2 ? a.nkw : a.KW, KHn = MODE == 2 ? a.nkh : a.KH;
#pragma unroll
  for (int p = 0; p < NPA; ++p) {
    const int chunk = wave + p * NW;
    const int m = tile_m * BM + chunk * 16 + lrow;
    rv[p] = chunk < CA && m < a.M;
    const int mm = rv[p] ? m : 0;
    const int img = mm / HWo, rem = mm - img * HWo;
    const int ho = rem / Wrow, wo = rem - ho * Wrow;
    ib[p] = img * a.Hin * a.Win;
    if (MODE == 0) { bh[p] = ho * a.stride - a.pad; bw[p] = wo * a.stride - a.pad; }
    else if (MODE == 1) { bh[p] = ho + a.pad;       bw[p] = wo + a.pad; }
    else { bh[p] = 2 * ho + a.ph + a.pad - a.kh0;   bw[p] = 2 * wo + a.pw + a.pad - a.kw0; }   // always even
  }
  int kc, kh, kw;
  {
    const int k0 = kv * VEC, tap = k0 / a.Cin;
    kc = k0 - tap * a.Cin; kh = tap / KWn; kw = tap - kh * KWn;
  }
  const int smask = a.stride - 1;

  // ---- UT (uniform tap): Cin % BK == 0, so a K tile never straddles a tap and the whole wave walks the taps together.
  // The tap cursor then lives in SGPRs and each DMA needs only: 2 adds + 2 unsigned compares + 1 select per pixel row.
  int rowoff[NPA], rowh[NPA], roww[NPA], nboff[NPB];
  bool nv[NPB];
  if (UT) {
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      rowh[p] = MODE == 2 ? (bh[p] >> 1) : bh[p];
      roww[p] = MODE == 2 ? (bw[p] >> 1) : bw[p];
      rowoff[p] = ((ib[p] + rowh[p] * a.Win + roww[p]) * a.in_ldc + kv * VEC) * (int)sizeof(T);
    }
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const int chunk = wave + p * NW;
      const int n = tile_n * BN + chunk * 16 + lrow;
      nv[p] = chunk < CB && n < a.Nout;
      nboff[p] = (n * (a.KH * a.KW * a.Cin) + kv * VEC) * (int)sizeof(T);
    }
  }
  int s_c0 = 0, s_kh = 0, s_kw = 0;       // wave-uniform tap cursor (UT)
  auto issue_tile_ut = [&](int kt, int buf) {
    unsigned char* sA = smem + buf * (BM + BN) * 64;
    unsigned char* sB = sA + BM * 64;
    const bool kvalid = s_kh < KHn;
    // tap displacement of the source pixel (in pixels) and in bytes
    const int dh = MODE == 0 ? s_kh * a.dil : -(MODE == 1 ? s_kh * a.dil : s_kh);
    const int dw = MODE == 0 ? s_kw * a.dil : -(MODE == 1 ? s_kw * a.dil : s_kw);
    const int tapoff = ((dh * a.Win + dw) * a.in_ldc + s_c0) * (int)sizeof(T);
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      const int chunk = wave + p * NW;
      if (CA % NW == 0 || chunk < CA) {
        const int hi = rowh[p] + dh, wi = roww[p] + dw;
        const bool ok = rv[p] & kvalid & ((unsigned)hi < (unsigned)a.Hin) & ((unsigned)wi < (unsigned)a.Win);
        const unsigned off = ok ? (unsigned)(rowoff[p] + tapoff) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_void_t*)(sA + chunk * 1024), 16, off, 0, 0, 0);
      } else if (UNEVEN) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_void_t*)(smem + SINK), 16, OOB, 0, 0, 0);
      }
    }
    const int kw_full = MODE == 2 ? ((a.kh0 + 2 * s_kh) * a.KW + a.kw0 + 2 * s_kw) * a.Cin + s_c0 : kt * BK;
    const int koff = kw_full * (int)sizeof(T);
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const int chunk = wave + p * NW;
      if (CB % NW == 0 || chunk < CB) {
        const unsigned off = (nv[p] & kvalid) ? (unsigned)(nboff[p] + koff) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)(sB + chunk * 1024), 16, off, 0, 0, 0);
      } else if (UNEVEN) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)(smem + SINK), 16, OOB, 0, 0, 0);
      }
    }
  };
  auto advance_ut = [&]() {
    s_c0 += BK;
    if (s_c0 >= a.Cin) { s_c0 = 0; if (++s_kw == KWn) { s_kw = 0; ++s_kh; } }
  };
  auto issue_tile_gen = [&](int kt, int buf) {
    unsigned char* sA = smem + buf * (BM + BN) * 64;
    unsigned char* sB = sA + BM * 64;
    const bool kvalid = kh < KHn;
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      const int chunk = wave + p * NW;
      if (CA % NW == 0 || chunk < CA) {
        int hi, wi; bool ok = rv[p] & kvalid;
        if (MODE == 0) { hi = bh[p] + kh * a.dil; wi = bw[p] + kw * a.dil; }
        else if (MODE == 2) { hi = (bh[p] >> 1) - kh; wi = (bw[p] >> 1) - kw; }
        else {
          const int th = bh[p] - kh * a.dil, tw = bw[p] - kw * a.dil;
          ok = ok & (th >= 0) & (tw >= 0) & (((th | tw) & smask) == 0);
          hi = th >> a.sshift; wi = tw >> a.sshift;
        }
        ok = ok & ((unsigned)hi < (unsigned)a.Hin) & ((unsigned)wi < (unsigned)a.Win);
        const unsigned off = ok ? (unsigned)(((ib[p] + hi * a.Win + wi) * a.in_ldc + kc) * (int)sizeof(T)) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_void_t*)(sA + chunk * 1024), 16, off, 0, 0, 0);
      } else if (UNEVEN) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_void_t*)(smem + SINK), 16, OOB, 0, 0, 0);
      }
    }
    // weight row = [KH][KW][Cin] of the FULL kernel; MODE 2 visits the sub-lattice of taps
    const int k = MODE == 2 ? ((a.kh0 + 2 * kh) * a.KW + a.kw0 + 2 * kw) * a.Cin + kc : kt * BK + kv * VEC;
    const int wrow = a.KH * a.KW * a.Cin;
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const int chunk = wave + p * NW;
      if (CB % NW == 0 || chunk < CB) {
        const int n = tile_n * BN + chunk * 16 + lrow;
        const unsigned off = ((n < a.Nout) & kvalid & (k < wrow)) ? (unsigned)((n * wrow + k) * (int)sizeof(T)) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)(sB + chunk * 1024), 16, off, 0, 0, 0);
      } else if (UNEVEN) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)(smem + SINK), 16, OOB, 0, 0, 0);
      }
    }
  };
  auto advance_gen = [&]() {
    kc += BK;
    while (kc >= a.Cin) { kc -= a.Cin; if (++kw == KWn) { kw = 0; ++kh; } }
  };
  auto issue_tile = [&](int kt, int buf) { if (UT) issue_tile_ut(kt, buf); else issue_tile_gen(kt, buf); };
  auto advance = [&]() { if (UT) advance_ut(); else advance_gen(); };

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.Ktot + BK - 1) / BK;
  if (STAGES == 2) {
    issue_tile(0, 0);
    __syncthreads();                                 // (the compiler drains the LDS-DMA queue, vmcnt(0), ahead of the barrier)
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) { advance(); issue_tile(kt + 1, cur ^ 1); }
      const unsigned char* sA = smem + cur * (BM + BN) * 64 + wm * TM * 64;
      const unsigned char* sB = smem + cur * (BM + BN) * 64 + BM * 64 + wn * TN * 64;
      FragSwz<T>::template mma<FM, FN>(sA, sB, lane, acc);
      __syncthreads();
    }
  } else {
    // STAGES-deep ring: tiles kt+1 .. kt+STAGES-2 stay in flight ACROSS the barrier.  Only counted waits (never vmcnt(0) in
    // steady state) and a raw s_barrier, because __syncthreads() would drain the DMA queue.  Order per iteration:
    //   wait(tile kt landed for THIS wave) -> barrier (landed for ALL waves; everyone is done reading the slot reused next)
    //   -> issue tile kt+STAGES-1 into the slot read at iteration kt-1 -> MFMAs on tile kt.
    int issued = 0;
    for (; issued < STAGES - 1 && issued < nk; ++issued) { if (issued) advance(); issue_tile(issued, issued); }
    int slot = 0, islot = issued % STAGES;
    int kt = 0;
    // steady state: every iteration issues exactly one tile, so the wait count is a constant and the body is ONE basic
    // block (no branches): the DMA address arithmetic can be scheduled into the issue gaps between the MFMAs.
    for (const int nmain = nk - (STAGES - 1); kt < nmain; ++kt) {
      // (lgkmcnt(0): this wave's fragment reads of the previous tile are DONE before anyone may refill that slot -- the compiler sinks a
      //  tile's last MFMAs and their LDS waits below this barrier, and an LDS-DMA write is not ordered against queued ds_reads; conv_shift.hip)
      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GD * (STAGES - 2)) : "memory");
      __builtin_amdgcn_s_barrier();
      const unsigned char* sA = smem + slot * (BM + BN) * 64 + wm * TM * 64;
      const unsigned char* sB = smem + slot * (BM + BN) * 64 + BM * 64 + wn * TN * 64;
      if constexpr (sizeof(T) == 2) {
        bf16x8_t fa[FM], fb[FN];
        FragSwz<T>::template load<FM, FN>(sA, sB, lane, fa, fb);
        advance();
        issue_tile(kt + STAGES - 1, islot);
        FragSwz<T>::template compute<FM, FN>(fa, fb, acc);
      } else {
        advance();
        issue_tile(kt + STAGES - 1, islot);
        FragSwz<T>::template mma<FM, FN>(sA, sB, lane, acc);
      }
      islot = islot + 1 == STAGES ? 0 : islot + 1;
      slot = slot + 1 == STAGES ? 0 : slot + 1;
    }
    for (; kt < nk; ++kt) {                              // drain: no more tiles to issue
      const int newer = nk - 1 - kt;                     // tiles issued after tile kt (<= STAGES - 2)
      if (newer >= 2 && STAGES > 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GD * 2) : "memory");
      else if (newer == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(GD) : "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const unsigned char* sA = smem + slot * (BM + BN) * 64 + wm * TM * 64;
      const unsigned char* sB = smem + slot * (BM + BN) * 64 + BM * 64 + wn * TN * 64;
      FragSwz<T>::template mma<FM, FN>(sA, sB, lane, acc);
      slot = slot + 1 == STAGES ? 0 : slot + 1;
    }
    __syncthreads();                                   // the epilogue reuses the ring as staging
  }

  // ---------------- epilogue (same as the register-staged kernel) ----------------
  const int n0 = tile_n * BN + wn * TN, m0 = tile_m * BM + wm * TM;
  if constexpr (EPI) {                                     // inference instantiation (MODE 0): act(acc * scale + shift), once per tile (template
    // parameter: as a runtime branch it cost the training step 2 %)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + j * 16 + (lane & 15);
      const float sc = (a.epi.oscale && n < a.Nout) ? a.epi.oscale[n] : 1.f;
      const float bv = (a.bias && n < a.Nout) ? a.bias[n] : 0.f;
      const float sl = a.epi.act == 1 ? a.epi.slope : (a.epi.act == 2 ? 0.f : 1.f);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = acc[i][j][r] * sc + bv;
          acc[i][j][r] = v > 0.f ? v : v * sl;
        }
    }
  } else if (a.bias) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + j * 16 + (lane & 15);
      const float bv = n < a.Nout ? a.bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] += bv;
    }
  }
  float* sstat = reinterpret_cast<float*>(smem + STAT_OFF);
  const bool want_stats = a.stats || a.xacc.acc;
  if (want_stats) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + i * 16 + (lane >> 4) * 4 + r;
          const float v = m < a.M ? acc[i][j][r] : 0.f;
          s += v; q += v * v;
        }
      s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
      s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
      if (lane < 16) {
        sstat[(wm * 2 + 0) * BN + wn * TN + j * 16 + lane] = s;
        sstat[(wm * 2 + 1) * BN + wn * TN + j * 16 + lane] = q;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * TM + i * 16 + (lane >> 4) * 4 + r, col = wn * TN + j * 16 + (lane & 15);
        ET<T>::st(reinterpret_cast<T*>(smem + row * SROW) + col, acc[i][j][r]);
      }
  __syncthreads();
  constexpr int G = BM / 128 > 0 ? BM / 128 : 1, WPG = WM / G;
  if (want_stats && tid < BN * G) {
    const int g = tid / BN, col = tid - g * BN;
    const int n = tile_n * BN + col, srow = tile_m * G + g;
    if (n < a.Nout && srow * 128 < a.M) {
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int r = 0; r < WPG; ++r) { s += sstat[((g * WPG + r) * 2 + 0) * BN + col]; q += sstat[((g * WPG + r) * 2 + 1) * BN + col]; }
      if (a.xacc.acc) {                                     // fire-and-forget exact accumulation (exact_acc.h): no rows, no finalize launch
        long long* xp = a.xacc.acc + (size_t)(srow & (a.xacc.reps - 1)) * (XACC_DIGITS * 2) * a.Nout + n;
        xacc_add(xp, 2 * (size_t)a.Nout, s);
        xacc_add(xp + a.Nout, 2 * (size_t)a.Nout, q);
      } else {
        a.stats[((size_t)srow * 2 + 0) * a.Nout + n] = s;
        a.stats[((size_t)srow * 2 + 1) * a.Nout + n] = q;
      }
    }
  }
  T* __restrict__ out = reinterpret_cast<T*>(a.out);
  const T* __restrict__ addsrc = reinterpret_cast<const T*>(a.addsrc);
  constexpr int VPRO = BN / VEC;
  if constexpr (FUSE) {
    // data gradient with the BatchNorm-backward sums of the producer layer folded in (bn_fuse.h)
    using Acc = BnFuseAcc<T, BN, NT>;
    Acc fz;
    const int cv = tid % VPRO, n = tile_n * BN + cv * VEC;
    fz.init(a.fuse, n, a.Nout);
    const T* __restrict__ fy = reinterpret_cast<const T*>(a.fuse.y);
    float* fred = sstat;
    constexpr int PPG = 128 / Acc::RPP;                    // passes per 128-pixel group
    // The global loads (addsrc, y) of ALL groups of the tile are issued before the first group is processed (like the shift kernel):
    // they are HBM misses, the accumulators are dead by now, and one batch per group exposed their latency once per group.
    constexpr int NG = BM / 128 > 0 ? BM / 128 : 1;
    long long pixv[NG][PPG]; uint4 aq[NG][PPG], yq[NG][PPG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi)
#pragma unroll
      for (int u = 0; u < PPG; ++u) {
        const int row = gi * 128 + u * Acc::RPP + tid / VPRO;
        const int m = tile_m * BM + row;
        pixv[gi][u] = -1;
        if (m < a.M && n < a.Nout) {
          long long pix = m;
          if (MODE == 2) {
            const int img = m / HWo, rem = m - img * HWo;
            const int ha = rem / Wrow, wb = rem - ha * Wrow;
            pix = ((long long)img * a.Hout + (a.ph + 2 * ha)) * a.Wout + (a.pw + 2 * wb);
          }
          pixv[gi][u] = pix;
          if (addsrc) aq[gi][u] = *reinterpret_cast<const uint4*>(addsrc + (pix * a.add_ldc + n));
          yq[gi][u] = *reinterpret_cast<const uint4*>(fy + (pix * a.fuse.ldy + n));
        }
      }
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      const int g0 = gi * 128;
      uint4 dq[PPG];
#pragma unroll
      for (int u = 0; u < PPG; ++u) dq[u] = *reinterpret_cast<const uint4*>(smem + (g0 + u * Acc::RPP + tid / VPRO) * SROW + cv * 16);
#pragma unroll
      for (int u = 0; u < PPG; ++u) {
        if (pixv[gi][u] >= 0) {
          float x[VEC];
          uint4 d = dq[u];
          ET<T>::unpack(d, x);
          if (addsrc) {
            float y[VEC];
            ET<T>::unpack(aq[gi][u], y);
#pragma unroll
            for (int e = 0; e < VEC; ++e) x[e] += y[e];
            d = ET<T>::pack(x);
            ET<T>::unpack(d, x);
          }
          *reinterpret_cast<uint4*>(out + (pixv[gi][u] * a.out_ldc + n)) = d;
          fz.add(a.fuse, x, yq[gi][u]);
        }
      }
      if (tile_m * BM + g0 < a.M) {                    // block-uniform: a 256-row tile's second group may start past the last pixel,
        if constexpr (Acc::kWaveFold)                    // and that row is not in the caller's buffer
          fz.fold_wave(reinterpret_cast<float*>(smem + (g0 + wave * Acc::WROWS) * SROW), lane);   // the rows this wave read in its first pass: dead, private
        else
          fz.flush(a.fuse, fred, tid, tile_n * BN, a.Nout, (tile_m * BM + g0) >> 7);
      }
    }
    if constexpr (Acc::kWaveFold) {                      // the waves meet once, behind the tile's last store
      static_assert(Acc::WROWS * SROW >= 2 * BN * 4 && SROW % 4 == 0, "a wave's dead staging rows hold its 2*BN sums");
      lds_only_barrier();
      for (int t = tid; t < NG * 2 * BN; t += NT) {
        const int gi = t / (2 * BN), g0 = gi * 128;
        if (tile_m * BM + g0 < a.M)
          Acc::write_row(a.fuse, reinterpret_cast<const float*>(smem + g0 * SROW), Acc::WROWS * SROW / 4, t - gi * 2 * BN, tile_n * BN, a.Nout,
                         (tile_m * BM + g0) >> 7);
      }
    }
  } else {
  for (int v = tid; v < BM * VPRO; v += NT) {
    const int row = v / VPRO, cv = v - row * VPRO;
    const int m = tile_m * BM + row, n = tile_n * BN + cv * VEC;
    if (m < a.M && n < a.Nout) {
      size_t pix = (size_t)m;
      if (MODE == 2) {                                   // class-local index -> full-resolution output pixel
        const int img = m / HWo, rem = m - img * HWo;
        const int ha = rem / Wrow, wb = rem - ha * Wrow;
        pix = ((size_t)img * a.Hout + (a.ph + 2 * ha)) * a.Wout + (a.pw + 2 * wb);
      }
      uint4 d = *reinterpret_cast<const uint4*>(smem + row * SROW + cv * 16);
      if (addsrc) {
        float x[VEC], y[VEC];
        ET<T>::unpack(d, x);
        ET<T>::unpack(*reinterpret_cast<const uint4*>(addsrc + (pix * a.add_ldc + n)), y);
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] += y[e];
        d = ET<T>::pack(x);
      }
      *reinterpret_cast<uint4*>(out + (pix * a.out_ldc + n)) = d;
    }
  }
  }
  }   // class loop
}

template <typename T, int MODE, int BM, int BN, int WM, int WN, int STAGES, bool UT, bool FUSE, bool EPI = false, bool ALLCLS = false>
int launch_conv_glds_f(const ConvArgs& a0, hipStream_t st, int B) {
  ConvArgs a = a0;
  constexpr int NWV = WM * WN;
  constexpr int PIPE = STAGES * (BM + BN) * 64 + ((STAGES > 2 && ((BM / 16) % NWV != 0 || (BN / 16) % NWV != 0)) ? 1024 : 0);   // + the DMA sink
  constexpr int STAGE = BM * (BN * (int)sizeof(T) + 16);
  constexpr int LDS = (PIPE > STAGE ? PIPE : STAGE) + WM * 2 * BN * 4;   // + statistics / fp32 fused-sum scratch (NW*BN floats <= WM*2*BN)
  static DynLds dyn_lds;
  auto kern = conv_glds_kernel<T, MODE, BM, BN, WM, WN, STAGES, UT, FUSE, EPI, ALLCLS>;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds, reinterpret_cast<const void*>(kern), LDS); e != hipSuccess) return (int)e;
  a.tiles_n = cdiv(a.Nout, BN);
  a.tiles_total = cdiv(a.M, BM) * a.tiles_n * ((ALLCLS && a.cls_split) ? 2 : 1);
  a.xcd_chunk = cdiv(a.tiles_total, 8);
  const unsigned in_bytes = (unsigned)((long long)B * a.Hin * a.Win * a.in_ldc * (long long)sizeof(T));
  const unsigned w_bytes = (unsigned)((long long)a.Nout * a.KH * a.KW * a.Cin * (long long)sizeof(T));
  MDCV_LAUNCH(kern, dim3((unsigned)(a.xcd_chunk * 8)), dim3(WM * WN * 64), LDS, st, a, in_bytes, w_bytes);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

template <typename T, int MODE, int BM, int BN, int WM, int WN, int STAGES, bool UT, bool ALLCLS = false>
int launch_conv_glds_ut(const ConvArgs& a, hipStream_t st, int B) {
  if constexpr (ALLCLS) {
    if (a.epi.oscale || a.epi.act) return MDCV_EARG;
    if (a.fuse.y) return launch_conv_glds_f<T, MODE, BM, BN, WM, WN, STAGES, UT, true, false, true>(a, st, B);
    return launch_conv_glds_f<T, MODE, BM, BN, WM, WN, STAGES, UT, false, false, true>(a, st, B);
  }
  if constexpr (MODE != 0) {                    // the fused BatchNorm-backward sums exist for data gradients only
    if (a.fuse.y) return launch_conv_glds_f<T, MODE, BM, BN, WM, WN, STAGES, UT, true>(a, st, B);
  }
  if constexpr (MODE == 0) {                    // inference epilogue (forward only)
    if (a.epi.oscale || a.epi.act) return launch_conv_glds_f<T, MODE, BM, BN, WM, WN, STAGES, UT, false, true>(a, st, B);
  }
  if (a.epi.oscale || a.epi.act) return MDCV_EARG;
  return launch_conv_glds_f<T, MODE, BM, BN, WM, WN, STAGES, UT, false>(a, st, B);
}

template <typename T, int MODE, int BM, int BN, int WM, int WN, int STAGES = 2, bool ALLCLS = false>
int launch_conv_glds(const ConvArgs& a, hipStream_t st, int B) {
  constexpr int BK = 4 * ET<T>::VEC;
  // uniform-tap fast path: K tiles never straddle a tap; the generic stride-2 dgrad (MODE 1, stride 2) keeps the per-lane cursor
  const bool ut = (a.Cin % BK == 0) && !(MODE == 1 && a.stride != 1) && TUNE().conv_no_ut == 0;
  if constexpr (ALLCLS) {                       // (bf16 layers of a Darknet: Cin is a multiple of 32; others keep the four launches)
    if (!ut) return MDCV_EARG;
    return launch_conv_glds_ut<T, MODE, BM, BN, WM, WN, STAGES, true, true>(a, st, B);
  }
  if (ut) return launch_conv_glds_ut<T, MODE, BM, BN, WM, WN, STAGES, true>(a, st, B);
  return launch_conv_glds_ut<T, MODE, BM, BN, WM, WN, STAGES, false>(a, st, B);
}


template <typename T, int MODE>
int dispatch_conv(const ConvArgs& a, hipStream_t st, int B) {
  constexpr bool BF = sizeof(T) == 2;
  const bool small = conv_operands_small((long long)B * a.Hin * a.Win * a.in_ldc * (long long)sizeof(T), (long long)a.Nout * a.Ktot * (long long)sizeof(T));
  if (a.Nout > 64) {
    int v = TUNE().conv_variant;
    if (v < 0) {   // measured on MI355X (scripts/conv_ab.py): tall tiles once the grid is >= 4 waves of CUs, half-width tiles
      const long long t128 = (long long)cdiv(a.M, 128) * cdiv(a.Nout, 128);   // when 128x128 would leave CUs idle
      const int nk = a.Ktot / (4 * ET<T>::VEC);      // long K loops profit from the 3-stage DMA ring (scripts/conv_ab.py)
      v = t128 >= 1024 ? 11 : (nk >= 100 ? 9 : (t128 >= 300 ? 6 : 7));
      if (TUNE().conv_fuse_narrow && MODE == 1 && a.fuse.y && a.KH == 1 && a.KW == 1) v = 10;
      if (TUNE().conv_deep_small && nk >= TUNE().conv_deep_small && (v == 6 || v == 7)) v += 3;   // 3-stage ring for the mid / sparse grids too
    }
    if (!BF && small) v = v == 8 ? 6 : (v == 11 ? 9 : v);   // the 8-wave 256-row tiles exist in bf16 only: fp32 takes the 128x128 LDS-DMA tiles
                                                                           // (the register-staged fallback has no inference epilogue and is slower)
    if (v >= 6 && !small) v = (v == 8 || v == 11) ? 2 : ((v == 7 || v == 10) ? 4 : 0);
    if (v == 6) return launch_conv_glds<T, MODE, 128, 128, 2, 2>(a, st, B);
    if (v == 7) return launch_conv_glds<T, MODE, 128, 64, 2, 2>(a, st, B);
    if (v == 9) return launch_conv_glds<T, MODE, 128, 128, 2, 2, 3>(a, st, B);
    if (v == 10) return launch_conv_glds<T, MODE, 128, 64, 2, 2, 3>(a, st, B);
    if (BF) {   // 8-wave / deep-K tiles only exist in the production dtype
      if (v == 8) return launch_conv_glds<T, MODE, (BF ? 256 : 128), 128, (BF ? 4 : 2), 2>(a, st, B);
      if (v == 11) return launch_conv_glds<T, MODE, (BF ? 256 : 128), 128, (BF ? 4 : 2), 2, 3>(a, st, B);
      if (v == 1) return launch_conv<T, MODE, 128, 128, 2, 2, (BF ? 2 : 1)>(a, st);
      if (v == 2) return launch_conv<T, MODE, (BF ? 256 : 128), 128, (BF ? 4 : 2), 2, 1>(a, st);
      if (v == 3) return launch_conv<T, MODE, (BF ? 256 : 128), 128, (BF ? 4 : 2), 2, (BF ? 2 : 1)>(a, st);
      if (v == 4) return launch_conv<T, MODE, 128, 64, 2, 2, (BF ? 2 : 1)>(a, st);
      if (v == 5) return launch_conv<T, MODE, 128, 64, 2, 2, 1>(a, st);
    } else if (v == 4 || v == 5) {
      return launch_conv<T, MODE, 128, 64, 2, 2, 1>(a, st);
    }
    return launch_conv<T, MODE, 128, 128, 2, 2, 1>(a, st);
  }
  const bool dma = small && TUNE().conv_variant != 0;      // variant 0 forces the register-staged kernels everywhere (A/B)
  if constexpr (BF) {
    if (dma && TUNE().conv_tall_narrow && a.M >= TUNE().conv_tall_narrow * 1024) {   // tall tiles for the narrow layers of large images
      if (a.Nout > 32) return launch_conv_glds<T, MODE, 256, 64, 4, 2, 3>(a, st, B);
      if (a.Nout > 16) return launch_conv_glds<T, MODE, 256, 32, 4, 1>(a, st, B);
      return launch_conv_glds<T, MODE, 256, 16, 4, 1>(a, st, B);
    }
  }
  if (dma && TUNE().conv_deep_narrow && a.Ktot / (4 * ET<T>::VEC) >= TUNE().conv_deep_narrow) {
    if (a.Nout > 32) return launch_conv_glds<T, MODE, 128, 64, 2, 2, 3>(a, st, B);
  }
  if (a.Nout > 32) return dma ? launch_conv_glds<T, MODE, 128, 64, 2, 2>(a, st, B) : launch_conv<T, MODE, 128, 64, 2, 2, (BF ? 2 : 1)>(a, st);
  if (a.Nout > 16) return dma ? launch_conv_glds<T, MODE, 128, 32, 4, 1>(a, st, B) : launch_conv<T, MODE, 128, 32, 4, 1, (BF ? 2 : 1)>(a, st);
  return dma ? launch_conv_glds<T, MODE, 128, 16, 4, 1>(a, st, B) : launch_conv<T, MODE, 128, 16, 4, 1, (BF ? 2 : 1)>(a, st);
}

// all four classes in one launch: same tile choice as the per-class dispatch below (a.M = positions of ONE class)
static int dispatch_dgrad_s2_all(const ConvArgs& a, hipStream_t st, int B) {
  typedef bf16_t T;
  if (TUNE().conv_tall_s2 && TUNE().conv_tall_narrow && a.Nout <= 64 && a.M >= TUNE().conv_tall_narrow * 1024) {
    if (a.Nout > 32) return launch_conv_glds<T, 2, 256, 64, 4, 2, 3, true>(a, st, B);
    if (a.Nout > 16) return launch_conv_glds<T, 2, 256, 32, 4, 1, 2, true>(a, st, B);
    return MDCV_EARG;
  }
  // Measured per layer of yolo_baseline at batch 32 (one launch vs four): 208->416 279 -> 204 us, 104->208 139 -> 125, 52->104 98 -> 86, but
  // 26->52 (338 tiles of 128 x 128: one sparse round of long workgroups) 136 -> 183 and 13->26 140 -> 139: only grids of >= 512 tiles take it.
  const long long t128 = (long long)cdiv(a.M, 128) * cdiv(a.Nout, 128);
  if (a.Nout <= 64) return MDCV_EARG;
  if (t128 < TUNE().conv_s2_split) {                    // sparse grids: two workgroups per tile (4 + 5 tap-GEMMs), see conv_glds_kernel
    if (!TUNE().conv_s2_split_on) return MDCV_EARG;
    ConvArgs c = a;
    c.cls_split = 1;
    return launch_conv_glds<T, 2, 128, 128, 2, 2, 3, true>(c, st, B);
  }
  if (t128 >= 1024) return launch_conv_glds<T, 2, 256, 128, 4, 2, 3, true>(a, st, B);
  return launch_conv_glds<T, 2, 128, 128, 2, 2, 3, true>(a, st, B);
}

template <typename T>
int dispatch_dgrad_s2(const ConvArgs& a, hipStream_t st, int B) {
  if constexpr (sizeof(T) == 2) {
    if (TUNE().conv_tall_s2 && TUNE().conv_tall_narrow && a.Nout <= 64 && a.M >= TUNE().conv_tall_narrow * 1024) {
      if (a.Nout > 32) return launch_conv_glds<T, 2, 256, 64, 4, 2, 3>(a, st, B);
      if (a.Nout > 16) return launch_conv_glds<T, 2, 256, 32, 4, 1>(a, st, B);
      return launch_conv_glds<T, 2, 256, 16, 4, 1>(a, st, B);
    }
  }
  if (TUNE().conv_deep_s2 && a.Nout > 32) {
    const long long t128 = (long long)cdiv(a.M, 128) * cdiv(a.Nout, 128);
    if (a.Nout > 64) {
      if (sizeof(T) == 2 && t128 >= 1024) return launch_conv_glds<T, 2, (sizeof(T) == 2 ? 256 : 128), 128, (sizeof(T) == 2 ? 4 : 2), 2, 3>(a, st, B);
      if (t128 >= 300) return launch_conv_glds<T, 2, 128, 128, 2, 2, 3>(a, st, B);
    }
    return launch_conv_glds<T, 2, 128, 64, 2, 2, 3>(a, st, B);
  }
  if (a.Nout > 64) {
    const long long t128 = (long long)cdiv(a.M, 128) * cdiv(a.Nout, 128);
    if (sizeof(T) == 2 && t128 >= 1024) return launch_conv_glds<T, 2, (sizeof(T) == 2 ? 256 : 128), 128, (sizeof(T) == 2 ? 4 : 2), 2>(a, st, B);
    if (t128 >= 300) return launch_conv_glds<T, 2, 128, 128, 2, 2>(a, st, B);
    return launch_conv_glds<T, 2, 128, 64, 2, 2>(a, st, B);
  }
  if (a.Nout > 32) return launch_conv_glds<T, 2, 128, 64, 2, 2>(a, st, B);
  if (a.Nout > 16) return launch_conv_glds<T, 2, 128, 32, 4, 1>(a, st, B);
  return launch_conv_glds<T, 2, 128, 16, 4, 1>(a, st, B);
}
}  // namespace
