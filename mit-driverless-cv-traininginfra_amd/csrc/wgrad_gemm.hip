// Generic weight-gradient kernels of the conv family for gfx950: conv_wgrad_kernel (register-staged, both dtypes), conv_wgrad_dma_kernel (bf16, LDS-DMA
// and transpose reads) and conv_wgrad_dma_narrow_kernel (Cout <= 32, optionally with the BatchNorm-backward apply in its operand load), with their launchers.
// conv_igemm.hip decides which layers come here (wgrad_gemm.h); the slabs they write are summed by wgrad_reduce.hip.
#include "conv_gemm.h"   // Frag<T>::mma (the register-staged kernel multiplies like the forward one), lds_void_t
#include "wgrad_gemm.h"

namespace {

// ------------------------------------------------------------------------------------------------
// weight gradient: dW[co, k] = sum_m dY[m, co] * Xcol[m, k]; pixels (the reduction) are split across the grid and each
// split writes an fp32 partial slab ws[split][Cout][Ktot]; mdcv_wgrad_reduce sums the slabs into the OIHW fp32 grad.
// Both operands are pixel-major in HBM, so tiles are transposed on the way into LDS ([channel][pixel] rows) with the
// channel<->row permutation  row = j*OQ + oct  (channel = oct*VEC + j)  which keeps the transposing ds_writes 2-way.
// ------------------------------------------------------------------------------------------------
struct WgradArgs {
  const void* dy; const void* x; float* ws;
  int dy_ldc, x_ldc;
  int Hin, Win, Cin, Hout, Wout, Cout;
  int KH, KW, stride, pad, dil;
  int M, Ktot, tiles_k, tiles_ck, pix_per_split, blocks_total, xcd_chunk;
  // BNA form of the narrow kernel (a layer whose input needs no gradient): `dy` holds dz, the operand dy = cA g + cB y + cC is formed in LDS
  const void* y; int y_ldc, act, creal; float slope;
  const float* s1; const float* b1; const float* cA; const float* cB; const float* cC;
};

// 128(co) x 128(k) output tile per block, 4 waves of 64x64.  One step = 128 pixels (bf16; 64 in fp32) = 256 bytes per LDS row:
// every thread issues the 16 global loads of the NEXT step before the 64 MFMAs of the current one (HBM latency is ~2 us under
// load, a 32-pixel step could not cover it), then the tile is transposed into the single LDS buffer between two barriers.
template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int VEC = ET<T>::VEC;
  constexpr int NP = 4;                // staging passes per step
  constexpr int BP = NP * 4 * VEC;     // pixels per step
  constexpr int OQ = 128 / VEC;        // 16-byte vectors per pixel across the 128-wide tile
  constexpr int PPP = 2 * (256 / OQ);  // pixels covered by one pass (two per thread)
  constexpr int RB = 64 * NP + 16;     // LDS row pitch in bytes
  constexpr int FM = 4, FN = 4;        // 2x2 waves, 64x64 per wave
  constexpr int OROW = 132;            // fp32 staging pitch
  static_assert(PPP * NP == BP, "pass geometry");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int logical = (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3);   // XCD-contiguous block order
  if (logical >= a.blocks_total) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int split = logical / a.tiles_ck;
  const int tck = logical - split * a.tiles_ck;
  const int tile_co = tck / a.tiles_k, tile_k = tck - tile_co * a.tiles_k;
  const T* __restrict__ dy = reinterpret_cast<const T*>(a.dy);
  const T* __restrict__ x = reinterpret_cast<const T*>(a.x);

  const int oct = tid % OQ, pp = tid / OQ;           // this thread stages pixels 2pp, 2pp+1 of every pass
  const int co0 = tile_co * 128 + oct * VEC;
  const bool a_ok = co0 < a.Cout;
  const int kcol0 = tile_k * 128 + oct * VEC;
  const bool b_ok = kcol0 < a.Ktot;
  int dh, dw, ci;
  {
    const int kk = b_ok ? kcol0 : 0;
    const int tap = kk / a.Cin;
    ci = kk - tap * a.Cin;
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    dh = kh * a.dil - a.pad; dw = kw * a.dil - a.pad;
  }
  const int p_begin = split * a.pix_per_split;
  const int p_end = min(a.M, p_begin + a.pix_per_split);
  const int HWo = a.Hout * a.Wout;

  uint4 ra[2 * NP], rb[2 * NP];
  auto load_step = [&](int m0) {
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const int m = m0 + ps * PPP + 2 * pp;
      int img = m / HWo, rem = m - img * HWo;
      int ho = rem / a.Wout, wo = rem - ho * a.Wout;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const bool pv = m + e < p_end;
        uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
        if (pv && a_ok) va = *reinterpret_cast<const uint4*>(dy + ((size_t)(m + e) * a.dy_ldc + co0));
        const int hi = ho * a.stride + dh, wi = wo * a.stride + dw;
        if (pv && b_ok && (unsigned)hi < (unsigned)a.Hin && (unsigned)wi < (unsigned)a.Win)
          vb = *reinterpret_cast<const uint4*>(x + ((size_t)((img * a.Hin + hi) * a.Win + wi) * a.x_ldc + ci));
        ra[2 * ps + e] = va; rb[2 * ps + e] = vb;
        if (++wo == a.Wout) { wo = 0; if (++ho == a.Hout) { ho = 0; ++img; } }
      }
    }
  };
  auto store_step = [&]() {
    unsigned char* sA = smem;
    unsigned char* sB = smem + 128 * RB;
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
      const unsigned a0[4] = {ra[2 * ps].x, ra[2 * ps].y, ra[2 * ps].z, ra[2 * ps].w}, a1[4] = {ra[2 * ps + 1].x, ra[2 * ps + 1].y, ra[2 * ps + 1].z, ra[2 * ps + 1].w};
      const unsigned b0[4] = {rb[2 * ps].x, rb[2 * ps].y, rb[2 * ps].z, rb[2 * ps].w}, b1[4] = {rb[2 * ps + 1].x, rb[2 * ps + 1].y, rb[2 * ps + 1].z, rb[2 * ps + 1].w};
      if (sizeof(T) == 2) {
        const int cb = ps * 64 + pp * 4;      // byte column of pixels (2pp, 2pp+1) of this pass
#pragma unroll
        for (int q = 0; q < 4; ++q) {         // channels 2q, 2q+1 of the octet ; word = (pixel 2pp | pixel 2pp+1 << 16)
          *reinterpret_cast<unsigned*>(sA + ((2 * q) * OQ + oct) * RB + cb) = (a0[q] & 0xffffu) | (a1[q] << 16);
          *reinterpret_cast<unsigned*>(sA + ((2 * q + 1) * OQ + oct) * RB + cb) = (a0[q] >> 16) | (a1[q] & 0xffff0000u);
          *reinterpret_cast<unsigned*>(sB + ((2 * q) * OQ + oct) * RB + cb) = (b0[q] & 0xffffu) | (b1[q] << 16);
          *reinterpret_cast<unsigned*>(sB + ((2 * q + 1) * OQ + oct) * RB + cb) = (b0[q] >> 16) | (b1[q] & 0xffff0000u);
        }
      } else {
        const int cb = ps * 64 + pp * 8;
#pragma unroll
        for (int q = 0; q < 4; ++q) {         // channel q of the quad ; two fp32 pixels side by side
          *reinterpret_cast<uint2*>(sA + (q * OQ + oct) * RB + cb) = make_uint2(a0[q], a1[q]);
          *reinterpret_cast<uint2*>(sB + (q * OQ + oct) * RB + cb) = make_uint2(b0[q], b1[q]);
        }
      }
    }
  };

  f32x4_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nt = (p_end - p_begin + BP - 1) / BP;
  if (nt > 0) {
    load_step(p_begin);
    store_step();
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) load_step(p_begin + (t + 1) * BP);
    Frag<T>::template mma<FM, FN, NP, RB>(smem + wm * 64 * RB, smem + 128 * RB + wn * 64 * RB, lane, acc);
    __syncthreads();                              // everyone is done reading the buffer
    if (t + 1 < nt) store_step();
    __syncthreads();
  }
  // stage fp32 tile [co_local][k_local] (undo the row permutation), then coalesced rows into the slab
  float* so = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int Ra = (wm * FM + i) * 16 + (lane >> 4) * 4 + r;
        const int Rb = (wn * FN + j) * 16 + (lane & 15);
        const int col = (Ra % OQ) * VEC + Ra / OQ;
        const int kl = (Rb % OQ) * VEC + Rb / OQ;
        so[col * OROW + kl] = acc[i][j][r];
      }
  __syncthreads();
  float* __restrict__ ws = a.ws + (size_t)split * a.Cout * a.Ktot;
  for (int v = tid; v < 128 * 32; v += 256) {
    const int row = v >> 5, c4 = (v & 31) * 4;
    const int co = tile_co * 128 + row, k = tile_k * 128 + c4;
    if (co < a.Cout && k < a.Ktot)   // Ktot is a multiple of 8, so a float4 never straddles the edge
      *reinterpret_cast<float4*>(ws + (size_t)co * a.Ktot + k) = *reinterpret_cast<const float4*>(so + row * OROW + c4);
  }
}

// ------------------------------------------------------------------------------------------------
// weight gradient, bf16 production kernel: LDS-DMA + hardware transpose reads.
// Operand tiles are DMA'ed in their natural HBM order [pixel][128 channels] (256-byte rows, 4 pixel rows per 1 KiB chunk);
// MFMA fragments need 8 consecutive PIXELS per channel, which ds_read_b64_tr_b16 delivers for free: a 16-lane group reads a
// 4(pixel) x 16(channel) block and lane i receives column i (verified on MI355X with a probe kernel in round 1).  Two such reads make one
// 16x16x32 fragment.  Bank conflicts between the 4 pixel rows of a block (256 B apart = same banks) are removed by a
// source-side XOR of the 16-byte column index with 2*(pixel & 7).  No ds_write, no VGPR staging, one barrier per 64-pixel step.
// ------------------------------------------------------------------------------------------------
// q = n / d, r = n % d for 0 <= n < 2^24 via one float multiply and a +-1 fix-up (an integer divide costs ~35 VALU ops)
__device__ __forceinline__ void fast_divmod(int n, int d, float inv, int& q, int& r) {
  q = (int)((float)n * inv);
  r = n - q * d;
  const int lt = r < 0;       q -= lt; r += lt ? d : 0;       // predicated (v_cndmask), no divergent branches
  const int ge = r >= d;      q += ge; r -= ge ? d : 0;
}

typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;

// Transpose read as inline asm (see wgrad_stream.hip): with the builtin, the compiler -- which cannot tell the ring slots apart --
// puts s_waitcnt vmcnt(0) in front of every LDS read that follows an LDS-DMA, so the fill of tile k+1 never overlapped the MFMAs of
// tile k inside a block.  The asm read is invisible to that hazard pass; the kernels order DMA and reads themselves (barriers,
// counted vmcnt) and wait for the reads with wait_lds_tr<N>(), whose "+v" operands make the MFMAs depend on the wait.
template <int OFF> __device__ __forceinline__ s16x4_t lds_tr16_asm(unsigned addr) {
  s16x4_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ unsigned lds_addr(const unsigned char* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)p;
}
template <int N> __device__ __forceinline__ void wait_lds_tr(bf16x8_t& a0) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a0) : "n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void wait_lds_tr(bf16x8_t& a0, bf16x8_t& a1, bf16x8_t& b0) {
  asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a0), "+v"(a1), "+v"(b0) : "n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void wait_lds_tr(bf16x8_t& a0, bf16x8_t& a1, bf16x8_t& a2, bf16x8_t& a3, bf16x8_t& b0) {
  asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0) : "n"(N) : "memory");
}

template <int BP, int STAGES, bool SAME>
__global__ __launch_bounds__(256) void conv_wgrad_dma_kernel(WgradArgs a, unsigned dy_bytes, unsigned x_bytes) {
  constexpr int NJ = BP / 16;            // chunks (of 4 pixel rows) per operand per wave per step
  constexpr int GD = 2 * NJ;             // LDS-DMA instructions per wave per step
  constexpr int TILE = BP * 256;         // bytes per operand tile
  constexpr int OROW = 132;
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int logical = (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3);
  if (logical >= a.blocks_total) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int split = logical / a.tiles_ck;
  const int tck = logical - split * a.tiles_ck;
  const int tile_co = tck / a.tiles_k, tile_k = tck - tile_co * a.tiles_k;
  const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, x_bytes, 0x00020000);

  // DMA role of this lane: wave w fills chunks w, w+4, w+8, w+12 (4 pixel rows each); inside a chunk the lane fills row
  // r = lane>>4, 16-byte slot q = lane&15, with the data of logical column q ^ 2*(pixel&7); pixel&7 = r + 4*(w&1) for all its chunks
  const int r = lane >> 4, q = lane & 15;
  const int lcol = q ^ (2 * (r + 4 * (wave & 1)));
  const int co0 = tile_co * 128 + lcol * 8;
  const bool a_ok = co0 < a.Cout;
  const int kcol0 = tile_k * 128 + lcol * 8;
  const bool b_ok = kcol0 < a.Ktot;
  int dh, dw, ci;
  {
    const int kk = b_ok ? kcol0 : 0;
    const int tap = kk / a.Cin;
    ci = kk - tap * a.Cin;
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    dh = kh * a.dil - a.pad; dw = kw * a.dil - a.pad;
  }
  const int p_begin = split * a.pix_per_split;
  const int p_end = min(a.M, p_begin + a.pix_per_split);
  const int HWo = a.Hout * a.Wout;
  const float inv_hw = 1.0f / (float)HWo, inv_w = 1.0f / (float)a.Wout;
  // all pixel indices are < 2^24 (checked by the host), so 24-bit multiplies (full rate) address both operands
  const unsigned ldy2 = (unsigned)a.dy_ldc * 2u, lx2 = (unsigned)a.x_ldc * 2u;
  const unsigned lane_a = (unsigned)co0 * 2u;
  // SAME (stride 1, equal input/output size): the source pixel of output pixel m under tap (dh,dw) is simply m + dh*W + dw
  const int lane_b = SAME ? ((dh * a.Win + dw) * a.x_ldc + ci) * 2 : ci * 2;
  const bool taps = a.KH * a.KW > 1 || a.pad != 0;        // 1x1 / pad 0: every source pixel is inside the image

  auto issue = [&](int m0, int buf) {
    unsigned char* sA = smem + buf * 2 * TILE;
    unsigned char* sB = sA + TILE;
    int m = m0 + 4 * wave + r;                            // this lane's pixel in chunk j = 0; chunk j adds 16*j
    int img = 0, ho = 0, wo = 0;
    if (!SAME || taps) {                                  // (uniform) one reciprocal divmod per step, then +16 increments
      int rem;
      fast_divmod(m, HWo, inv_hw, img, rem);
      fast_divmod(rem, a.Wout, inv_w, ho, wo);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int chunk = wave + 4 * j;
      const bool pv = m < p_end;
      const unsigned offa = (pv & a_ok) ? __umul24((unsigned)m, ldy2) + lane_a : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rdy, (lds_void_t*)(sA + chunk * 1024), 16, offa, 0, 0, 0);
      unsigned offb;
      bool ok = pv & b_ok;
      if (SAME) {
        if (taps) ok = ok & ((unsigned)(ho + dh) < (unsigned)a.Hin) & ((unsigned)(wo + dw) < (unsigned)a.Win);
        offb = __umul24((unsigned)m, lx2) + (unsigned)lane_b;
      } else {
        const int hi = ho * a.stride + dh, wi = wo * a.stride + dw;
        ok = ok & ((unsigned)hi < (unsigned)a.Hin) & ((unsigned)wi < (unsigned)a.Win);
        offb = __umul24((unsigned)((img * a.Hin + hi) * a.Win + wi), lx2) + (unsigned)lane_b;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_t*)(sB + chunk * 1024), 16, ok ? offb : OOB, 0, 0, 0);
      if (j + 1 < NJ) {
        m += 16;
        if (!SAME || taps) {                              // predicated wrap of (wo, ho, img); Wout >= 8 so two wraps cover +16
          wo += 16;
          int c = wo >= a.Wout; wo -= c ? a.Wout : 0; ho += c;
          c = wo >= a.Wout;     wo -= c ? a.Wout : 0; ho += c;
          c = ho >= a.Hout;     ho -= c ? a.Hout : 0; img += c;
        }
      }
    }
  };

  // fragment read offsets of this lane inside an operand tile (k-step ks adds ks*32 pixel rows, fragment F adds 32 bytes of columns)
  const int t = lane & 15, kq = lane >> 4;
  // K slot (kq, half, i) of the MFMA <-> pixel row kq*4 + i + 16*half of the 32-row k-step (any bijection works: both operands use
  // it).  Lanes 0-31 (one LDS service group) then read 8 consecutive rows = 8 distinct swizzle classes = all 64 banks; with
  // rows kq*8 + i every transpose read was a 2-way conflict (rocprofv3: SQ_LDS_BANK_CONFLICT = 49 % of SQ_LDS_IDX_ACTIVE).
  const int prow = kq * 4 + (t >> 2);                       // pixel row of the first transpose read (second: +16)
  const int sub = (t & 1) * 8;                              // 8-byte half of the 16-byte column
  const int qlo = (t & 3) >> 1;                             // which 16-byte column of the fragment's pair
  const int g0 = 2 * (prow & 7);                            // swizzle of the two reads (same pixel & 7)
  auto frag = [&](const unsigned char* tile, int ks, int F) -> bf16x8_t {
    const int row0 = ks * 32 + prow;
    const int c = 2 * F + qlo;
    const unsigned ad = lds_addr(tile) + (unsigned)(row0 * 256 + ((c ^ g0) << 4) + sub);      // the row 16 further down has the same swizzle
    const s16x4_t lo = lds_tr16_asm<0>(ad);
    const s16x4_t hi = lds_tr16_asm<16 * 256>(ad);
    typedef __attribute__((ext_vector_type(8))) short s16x8_t;
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nt = (p_end - p_begin + BP - 1) / BP;
  auto compute = [&](int slot) {
    const unsigned char* sA = smem + slot * 2 * TILE;
    const unsigned char* sB = sA + TILE;
#pragma unroll
    for (int ks = 0; ks < BP / 32; ++ks) {
      bf16x8_t fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag(sA, ks, wm * 4 + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = frag(sB, ks, wn * 4 + j);
      // the 16 reads return in order: column j of the 4x4 fragment grid starts as soon as fb[j] is in
      wait_lds_tr<6>(fa[0], fa[1], fa[2], fa[3], fb[0]);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[0], acc[i][0], 0, 0, 0);
      wait_lds_tr<4>(fb[1]);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[1], acc[i][1], 0, 0, 0);
      wait_lds_tr<2>(fb[2]);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[2], acc[i][2], 0, 0, 0);
      wait_lds_tr<0>(fb[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[3], acc[i][3], 0, 0, 0);
    }
  };
  if (STAGES == 2) {
    if (nt > 0) issue(p_begin, 0);
    __syncthreads();
    for (int st = 0; st < nt; ++st) {
      const int cur = st & 1;
      if (st + 1 < nt) issue(p_begin + (st + 1) * BP, cur ^ 1);
      compute(cur);
      __syncthreads();
    }
  } else {       // STAGES-deep DMA ring, counted vmcnt + raw barrier (see conv_glds_kernel)
    int issued = 0;
    for (; issued < STAGES - 1 && issued < nt; ++issued) issue(p_begin + issued * BP, issued);
    int slot = 0, islot = issued % STAGES;
    for (int st = 0; st < nt; ++st) {
      const int newer = issued - 1 - st;
      if (newer >= STAGES - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GD * (STAGES - 2)) : "memory");
      else if (newer == 1 && STAGES > 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GD) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (issued < nt) {
        issue(p_begin + issued * BP, islot);
        ++issued;
        islot = islot + 1 == STAGES ? 0 : islot + 1;
      }
      compute(slot);
      slot = slot + 1 == STAGES ? 0 : slot + 1;
    }
    __syncthreads();
  }
  // fp32 tile -> LDS -> coalesced rows of the split's slab
  float* so = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        so[((wm * 4 + i) * 16 + (lane >> 4) * 4 + rr) * OROW + (wn * 4 + j) * 16 + (lane & 15)] = acc[i][j][rr];
  __syncthreads();
  float* __restrict__ ws = a.ws + (size_t)split * a.Cout * a.Ktot;
  for (int v = tid; v < 128 * 32; v += 256) {
    const int row = v >> 5, c4 = (v & 31) * 4;
    const int co = tile_co * 128 + row, k = tile_k * 128 + c4;
    if (co < a.Cout && k < a.Ktot)
      *reinterpret_cast<float4*>(ws + (size_t)co * a.Ktot + k) = *reinterpret_cast<const float4*>(so + row * OROW + c4);
  }
}

// Narrow-output variant (Cout_pad <= 32: first layers, RektNet's 16/32-channel blocks, heads): output tile 32(co) x 128(k).
// The dY tile is [64 px][32 co] = 64-byte rows, 16 pixel rows per 1 KiB chunk (one chunk per wave), no swizzle needed (the 4 rows
// of a transpose read sit 64 B apart -> distinct banks).  Each wave owns a 32 x 32 slice: 4 MFMAs per 32-pixel k-step instead of
// 16 MFMAs on a tile that would be 75-87 % zero padding.  These layers are HBM-bound; the point is to stop wasting issue slots.
// BNA (round 5): the layer's input needs no gradient (YOLOv3's first conv), so dy = cA g + cB y + cC, g = dz act'(scale y + shift), has this
// kernel as its ONLY reader: it is formed here, in LDS, from the dz and y tiles (two DMAs instead of one; every thread transforms one 16-byte
// vector of the 64 x 32 tile per step, rounding to bf16 exactly as mdcv_bn_act_bwd_apply does -- the results are bit-identical to apply +
// this kernel), and the BatchNorm-apply pass over the largest tensor of the network (416^2 x 32 at batch 32: read 708 MB, write 354 MB, then
// read again here) never runs.  It sat at the exposed tail of the backward: apply 193 us on the main queue, then this kernel 131 us alone.
template <bool SAME, int STAGES, bool BNA = false>
__global__ __launch_bounds__(256) void conv_wgrad_dma_narrow_kernel(WgradArgs a, unsigned dy_bytes, unsigned x_bytes) {
  constexpr int BP = 64, NJ = 4, GD = BNA ? 6 : 5;
  constexpr int TA = BP * 64 * (BNA ? 2 : 1), TB = BP * 256;   // bytes per operand tile (BNA: dz tile + y tile)
  constexpr int OROW = 132;
  constexpr unsigned OOB = 0x80000000u;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int logical = (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3);
  if (logical >= a.blocks_total) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = logical / a.tiles_ck;
  const int tile_k = logical - split * a.tiles_ck;          // tiles_co == 1
  const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, dy_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(BNA ? a.y : a.dy), 0,
                                                                      BNA ? (unsigned)a.M * (unsigned)a.y_ldc * 2u : 0u, 0x00020000);

  // A (dY) DMA role: chunk = wave; lane fills pixel row ra = lane>>2, 16-byte slot lane&3; rows with bit 2 set hold their two
  // 32-byte halves swapped, so the 8 consecutive rows one LDS service group reads (64-byte rows: 4 rows per bank period) hit all banks
  const int ra = lane >> 2;
  const int coA = ((lane & 3) ^ (2 * ((ra >> 2) & 1))) * 8;
  const bool a_ok = coA < a.Cout;
  // B (X) DMA role: as in the wide kernel
  const int r = lane >> 4, q = lane & 15;
  const int lcol = q ^ (2 * (r + 4 * (wave & 1)));
  const int kcol0 = tile_k * 128 + lcol * 8;
  const bool b_ok = kcol0 < a.Ktot;
  int dh, dw, ci;
  {
    const int kk = b_ok ? kcol0 : 0;
    const int tap = kk / a.Cin;
    ci = kk - tap * a.Cin;
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    dh = kh * a.dil - a.pad; dw = kw * a.dil - a.pad;
  }
  const int p_begin = split * a.pix_per_split;
  const int p_end = min(a.M, p_begin + a.pix_per_split);
  const int HWo = a.Hout * a.Wout;
  const float inv_hw = 1.0f / (float)HWo, inv_w = 1.0f / (float)a.Wout;
  const unsigned ldy2 = (unsigned)a.dy_ldc * 2u, lx2 = (unsigned)a.x_ldc * 2u;
  const int lane_b = SAME ? ((dh * a.Win + dw) * a.x_ldc + ci) * 2 : ci * 2;
  const bool taps = a.KH * a.KW > 1 || a.pad != 0;

  auto issue = [&](int m0, int buf) {
    unsigned char* sA = smem + buf * (TA + TB);
    unsigned char* sB = sA + TA;
    {
      const int m = m0 + 16 * wave + ra;
      const unsigned offa = (m < p_end && a_ok) ? __umul24((unsigned)m, ldy2) + (unsigned)coA * 2u : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rdy, (lds_void_t*)(sA + wave * 1024), 16, offa, 0, 0, 0);
      if constexpr (BNA) {
        const unsigned offy = (m < p_end && a_ok) ? __umul24((unsigned)m, (unsigned)a.y_ldc * 2u) + (unsigned)coA * 2u : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ry, (lds_void_t*)(sA + BP * 64 + wave * 1024), 16, offy, 0, 0, 0);
      }
    }
    int m = m0 + 4 * wave + r;
    int img = 0, ho = 0, wo = 0;
    if (!SAME || taps) {
      int rem;
      fast_divmod(m, HWo, inv_hw, img, rem);
      fast_divmod(rem, a.Wout, inv_w, ho, wo);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int chunk = wave + 4 * j;
      bool ok = (m < p_end) & b_ok;
      unsigned offb;
      if (SAME) {
        if (taps) ok = ok & ((unsigned)(ho + dh) < (unsigned)a.Hin) & ((unsigned)(wo + dw) < (unsigned)a.Win);
        offb = __umul24((unsigned)m, lx2) + (unsigned)lane_b;
      } else {
        const int hi = ho * a.stride + dh, wi = wo * a.stride + dw;
        ok = ok & ((unsigned)hi < (unsigned)a.Hin) & ((unsigned)wi < (unsigned)a.Win);
        offb = __umul24((unsigned)((img * a.Hin + hi) * a.Win + wi), lx2) + (unsigned)lane_b;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_t*)(sB + chunk * 1024), 16, ok ? offb : OOB, 0, 0, 0);
      if (j + 1 < NJ) {
        m += 16;
        if (!SAME || taps) {
          wo += 16;
          int c = wo >= a.Wout; wo -= c ? a.Wout : 0; ho += c;
          c = wo >= a.Wout;     wo -= c ? a.Wout : 0; ho += c;
          c = ho >= a.Hout;     ho -= c ? a.Hout : 0; img += c;
        }
      }
    }
  };

  const int t = lane & 15, kq = lane >> 4;
  const int prow = kq * 4 + (t >> 2);                       // conflict-free K-slot <-> pixel-row mapping (see conv_wgrad_dma_kernel)
  const int sub = (t & 1) * 8, qlo = (t & 3) >> 1;
  const int g0 = 2 * (prow & 7);
  typedef __attribute__((ext_vector_type(8))) short s16x8_t;
  auto fragB = [&](const unsigned char* tile, int ks, int F) -> bf16x8_t {
    const int row0 = ks * 32 + prow, c = 2 * F + qlo;
    const unsigned ad = lds_addr(tile) + (unsigned)(row0 * 256 + ((c ^ g0) << 4) + sub);
    const s16x4_t lo = lds_tr16_asm<0>(ad);
    const s16x4_t hi = lds_tr16_asm<16 * 256>(ad);
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
  };
  auto fragA = [&](const unsigned char* tile, int ks, int F) -> bf16x8_t {       // 64-byte rows: F selects the 32-byte half,
    const int row0 = ks * 32 + prow;                                             // stored swapped in rows with bit 2 set
    const int col = (F ^ (kq & 1)) * 32 + (t & 3) * 8;
    const unsigned ad = lds_addr(tile) + (unsigned)(row0 * 64 + col);
    const s16x4_t lo = lds_tr16_asm<0>(ad);
    const s16x4_t hi = lds_tr16_asm<16 * 64>(ad);
    const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
  };

  // BNA transform role: thread tid owns the 16-byte vector at byte tid * 16 of the 64 x 64-byte tile: row tid >> 2 (the row's pixel is m0 + row),
  // physical slot tid & 3 = channels coT .. coT + 7 (the DMA's half swap for rows with bit 2 set)
  const int rowT = tid >> 2, coT = ((tid & 3) ^ (2 * ((rowT >> 2) & 1))) * 8;
  float ts1[BNA ? 8 : 1], tb1[BNA ? 8 : 1], tA[BNA ? 8 : 1], tB[BNA ? 8 : 1], tC[BNA ? 8 : 1];
  if constexpr (BNA) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = coT + e < a.creal;
      ts1[e] = ok ? a.s1[coT + e] : 0.f; tb1[e] = ok ? a.b1[coT + e] : 0.f;
      tA[e] = ok ? a.cA[coT + e] : 0.f; tB[e] = ok ? a.cB[coT + e] : 0.f; tC[e] = ok ? a.cC[coT + e] : 0.f;
    }
  }
  auto transform = [&](int slot, int m0) {                   // dz tile -> dy tile, in place (rows past the split: zeros, not cC)
    unsigned char* sA = smem + slot * (TA + TB);
    const unsigned ad = lds_addr(sA) + (unsigned)(tid * 16);
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t rd, ry4;
    asm volatile("ds_read_b128 %0, %1" : "=v"(rd) : "v"(ad) : "memory");            // (asm: a plain LDS access behind an LDS-DMA gets a compiler-inserted vmcnt(0))
    asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(ry4) : "v"(ad) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rd), "+v"(ry4)::"memory");
    float d[8], v[8], o[8];
    ET<bf16_t>::unpack(make_uint4(rd[0], rd[1], rd[2], rd[3]), d);
    ET<bf16_t>::unpack(make_uint4(ry4[0], ry4[1], ry4[2], ry4[3]), v);
    const bool live = m0 + rowT < p_end;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = live ? mdcv_bn_bwd_dy(d[e], v[e], ts1[e], tb1[e], tA[e], tB[e], tC[e], a.act, a.slope) : 0.f;
    const uint4 qo = ET<bf16_t>::pack(o);
    const u32x4_t wo = {qo.x, qo.y, qo.z, qo.w};
    asm volatile("ds_write_b128 %0, %1" ::"v"(ad), "v"(wo) : "memory");
  };

  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nt = (p_end - p_begin + BP - 1) / BP;
  auto compute = [&](int slot) {
    const unsigned char* sA = smem + slot * (TA + TB);
    const unsigned char* sB = sA + TA;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = fragA(sA, ks, i);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = fragB(sB, ks, wave * 2 + j);
      wait_lds_tr<2>(fa[0], fa[1], fb[0]);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[0], acc[i][0], 0, 0, 0);
      wait_lds_tr<0>(fb[1]);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[1], acc[i][1], 0, 0, 0);
    }
  };
  // these layers are HBM-latency-bound (tiny per-step work): keep STAGES-1 steps of DMA in flight (counted vmcnt, raw barrier)
  int issued = 0;
  for (; issued < STAGES - 1 && issued < nt; ++issued) issue(p_begin + issued * BP, issued);
  int slot = 0, islot = issued % STAGES;
  for (int st = 0; st < nt; ++st) {
    const int newer = issued - 1 - st;
    if (newer >= 3 && STAGES >= 5) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GD * 3) : "memory");
    else if (newer >= 2 && STAGES >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GD * 2) : "memory");
    else if (newer >= 1 && STAGES >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GD) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (issued < nt) {
      issue(p_begin + issued * BP, islot);
      ++issued;
      islot = islot + 1 == STAGES ? 0 : islot + 1;
    }
    if constexpr (BNA) {
      transform(slot, p_begin + st * BP);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                          // the dy tile is complete before any wave's transpose reads
    }
    compute(slot);
    slot = slot + 1 == STAGES ? 0 : slot + 1;
  }
  __syncthreads();
  float* so = reinterpret_cast<float*>(smem);          // [32][OROW]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        so[(i * 16 + (lane >> 4) * 4 + rr) * OROW + (wave * 2 + j) * 16 + (lane & 15)] = acc[i][j][rr];
  __syncthreads();
  float* __restrict__ ws = a.ws + (size_t)split * a.Cout * a.Ktot;
  for (int v = tid; v < 32 * 32; v += 256) {
    const int row = v >> 5, c4 = (v & 31) * 4;
    const int k = tile_k * 128 + c4;
    if (row < a.Cout && k < a.Ktot)
      *reinterpret_cast<float4*>(ws + (size_t)row * a.Ktot + k) = *reinterpret_cast<const float4*>(so + row * OROW + c4);
  }
}


template <int BP, int STAGES, bool SAME>
static int launch_wgrad_dma_t(const WgradArgs& a, unsigned grid, hipStream_t st, unsigned dyb, unsigned xb) {
  constexpr int RING = STAGES * 2 * BP * 256, EPI = 128 * 132 * 4;
  constexpr int LDS = RING > EPI ? RING : EPI;
  static DynLds dyn_lds;
  auto kern = conv_wgrad_dma_kernel<BP, STAGES, SAME>;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds, reinterpret_cast<const void*>(kern), LDS); e != hipSuccess) return (int)e;
  MDCV_LAUNCH(kern, dim3(grid), dim3(256), LDS, st, a, dyb, xb);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}
template <bool SAME, int STAGES, bool BNA = false>
static int launch_wgrad_narrow_t(const WgradArgs& a, unsigned grid, hipStream_t st, unsigned dyb, unsigned xb) {
  constexpr int LDS = STAGES * (64 * 64 * (BNA ? 2 : 1) + 64 * 256);   // 20 (24) KiB per stage (the 32 x 132 fp32 epilogue staging fits inside)
  static DynLds dyn_lds;
  auto kern = conv_wgrad_dma_narrow_kernel<SAME, STAGES, BNA>;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds, reinterpret_cast<const void*>(kern), LDS); e != hipSuccess) return (int)e;
  MDCV_LAUNCH(kern, dim3(grid), dim3(256), LDS, st, a, dyb, xb);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}
static int launch_wgrad_dma(const WgradArgs& a, unsigned grid, hipStream_t st, unsigned dyb, unsigned xb) {
  const bool same = a.stride == 1 && a.Hin == a.Hout && a.Win == a.Wout;
  if (a.Cout <= 32 && TUNE().wgrad_variant != 5)                       // (variant 5: the wide tile for narrow layers too, A/B)
    return same ? launch_wgrad_narrow_t<true, 4>(a, grid, st, dyb, xb) : launch_wgrad_narrow_t<false, 4>(a, grid, st, dyb, xb);
  if (TUNE().wgrad_variant == 4) return launch_wgrad_dma_t<64, 2, false>(a, grid, st, dyb, xb);        // generic address path (A/B)
  return same ? launch_wgrad_dma_t<64, 2, true>(a, grid, st, dyb, xb) : launch_wgrad_dma_t<64, 2, false>(a, grid, st, dyb, xb);
}

// the fields every form of the generic kernels reads; false when `splits` is not the pixel split of bp-pixel steps
bool fill_wgrad_args(WgradArgs& a, const WgradGeom& g, const void* dy, const void* x, float* ws, int splits, int bp) {
  a.dy = dy; a.x = x; a.ws = ws; a.dy_ldc = (int)g.dy_ldc; a.x_ldc = (int)g.x_ldc;
  a.Hin = g.Hin; a.Win = g.Win; a.Cin = g.Cin; a.Hout = g.Hout; a.Wout = g.Wout; a.Cout = g.Cout;
  a.KH = g.KH; a.KW = g.KW; a.stride = g.stride; a.pad = g.pad; a.dil = g.dil;
  a.M = g.B * g.Hout * g.Wout; a.Ktot = g.KH * g.KW * g.Cin;
  a.pix_per_split = cdiv(cdiv(a.M, splits), bp) * bp;
  a.tiles_k = cdiv(a.Ktot, 128);
  return cdiv(a.M, a.pix_per_split) == splits;
}
// the grid: tiles_ck channel tiles per split, laid out in eight XCD chunks
unsigned wgrad_grid(WgradArgs& a, int tiles_ck, int splits) {
  a.tiles_ck = tiles_ck;
  a.blocks_total = a.tiles_ck * splits;
  a.xcd_chunk = cdiv(a.blocks_total, 8);
  return (unsigned)(a.xcd_chunk * 8);
}

}  // namespace

int launch_wgrad_gemm(const WgradGeom& g, const void* dy, const void* x, float* ws, int splits, hipStream_t st) {
  const int dtype = g.dtype;
  WgradArgs a;
  if (!fill_wgrad_args(a, g, dy, x, ws, splits, dtype == MDCV_BF16 ? 128 : 64)) return MDCV_EARG;
  const long long dyb = (long long)a.M * g.dy_ldc * 2, xb = (long long)g.B * g.Hin * g.Win * g.x_ldc * 2;
  const bool use_dma = dtype == MDCV_BF16 && dyb < (1LL << 31) && xb < (1LL << 31) && TUNE().conv_variant != 0 &&
                       (long long)g.B * g.Hin * g.Win + 256 < (1LL << 24) && a.M + 256 < (1 << 24) && g.Wout >= 8 && g.x_ldc < (1 << 23) && g.dy_ldc < (1 << 23);
  const unsigned grid = wgrad_grid(a, a.tiles_k * cdiv(g.Cout, 128), splits);
  const int lds = 256 * (64 * 4 + 16);   // 69632 B: one transposed step; the fp32 epilogue staging (67584 B) reuses it
  static DynLds dyn_lds16, dyn_lds32;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds16, reinterpret_cast<const void*>(conv_wgrad_kernel<bf16_t>), lds); e != hipSuccess) return (int)e;
  if (hipError_t e = mdcv_dyn_lds(dyn_lds32, reinterpret_cast<const void*>(conv_wgrad_kernel<float>), lds); e != hipSuccess) return (int)e;
  if (use_dma) {
    const int rc = launch_wgrad_dma(a, grid, st, (unsigned)dyb, (unsigned)xb);
    if (rc) return rc;
  } else if (dtype == MDCV_BF16) MDCV_LAUNCH(conv_wgrad_kernel<bf16_t>, dim3(grid), dim3(256), lds, st, a);
  else if (dtype == MDCV_F32) MDCV_LAUNCH(conv_wgrad_kernel<float>, dim3(grid), dim3(256), lds, st, a);
  else return MDCV_EARG;
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

int launch_wgrad_gemm_bnapply(const WgradGeom& g, const void* dz, const void* y, int y_ldc, const float* scale, const float* shift, const float* cA,
                              const float* cB, const float* cC, int act, float slope, int Cout_real, const void* x, float* ws, int splits,
                              hipStream_t st) {
  WgradArgs a;
  if (!fill_wgrad_args(a, g, dz, x, ws, splits, 128)) return MDCV_EARG;
  const unsigned grid = wgrad_grid(a, a.tiles_k, splits);
  a.y = y; a.y_ldc = y_ldc; a.act = act; a.slope = act == 2 ? 0.f : slope; a.creal = Cout_real;
  a.s1 = scale; a.b1 = shift; a.cA = cA; a.cB = cB; a.cC = cC;
  const unsigned dyb = (unsigned)((long long)a.M * g.dy_ldc * 2), xb = (unsigned)((long long)g.B * g.Hin * g.Win * g.x_ldc * 2);
  const bool same = g.stride == 1 && g.Hin == g.Hout && g.Win == g.Wout;
  const int stages = TUNE().wgrad_bna_stages;
  if (stages <= 2) return same ? launch_wgrad_narrow_t<true, 2, true>(a, grid, st, dyb, xb) : launch_wgrad_narrow_t<false, 2, true>(a, grid, st, dyb, xb);
  if (stages == 3) return same ? launch_wgrad_narrow_t<true, 3, true>(a, grid, st, dyb, xb) : launch_wgrad_narrow_t<false, 3, true>(a, grid, st, dyb, xb);
  return same ? launch_wgrad_narrow_t<true, 4, true>(a, grid, st, dyb, xb) : launch_wgrad_narrow_t<false, 4, true>(a, grid, st, dyb, xb);
}
