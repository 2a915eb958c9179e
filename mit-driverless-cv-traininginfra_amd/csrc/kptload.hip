// Real key-point crops: ConeDataset.__getitem__ (RektNet/dataset.py:34-56) for a whole batch in one launch.  The host decodes the files and
// packs the crops (uint8, HWC, RGB, any height and width, back to back at unaligned byte offsets); from there to the two tensors the training
// loop reads runs here:
//   images   [B,3,S,S]  prep_image (RektNet/utils.py:73-76): cv2.resize of the 8-bit crop to S x S (resize_u8.h, the rule of
//                       mdcv_crop_resize_u8), then `transpose / 255.0` (dataset.py:54) as (float)((double)v / 255.0); planes in B, G, R order,
//                       because cv2.imread delivers BGR and the reference never swaps
//   heatmaps [B,7,S,S]  prep_label (utils.py:83-96) in float64 (kpt_heatmap.h, shared with synth_crops_kernel); all NaN where a
//                       down-scaled one-hot misses every tap (the reference's 0 / 0)
// One workgroup per output plane: grid (10, B), planes 0-2 the image channels, 3-9 the heat-maps.  A plane's tables (the taps of both axes
// and their coefficients, or the two separable vectors of its key point in both stages) live in LDS, sized from S: 32 * S + 32 bytes.
// The work is store-bound (40 * S * S bytes per crop out, a few KB in): with S % 4 == 0 each lane writes 16 bytes, lanes consecutive
// along x.  Built with -ffp-contract=off like synth.hip: the outputs are compared bit for bit with the numpy oracle.
#include "common.h"
#include "kpt_heatmap.h"
#include "resize_u8.h"
#include "kptload_desc.h"

namespace {

struct KptArgs {
  const int* desc; int B;
  const unsigned char* src; long long src_bytes;
  int S, vec;
  float* images; float* heatmaps;
};

__device__ __forceinline__ float image_value(const unsigned char* r0, const unsigned char* r1, int x0, int x1, int a0, int a1, int b0, int b1) {
  const int d0 = (int)r0[x0] * a0 + (int)r0[x1] * a1;
  const int d1 = (int)r1[x0] * a0 + (int)r1[x1] * a1;
  return blend_rows_u8(b0, d0, b1, d1);
}

__global__ __launch_bounds__(256) void kptload_kernel(KptArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int plane = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, S = A.S;
  const int* d = A.desc + (size_t)b * MDCV_KPTLOAD_DESC;
  const int off = d[KD_SRC_OFF], h = d[KD_H], w = d[KD_W];
  const size_t pl = (size_t)S * S;
  float* __restrict__ out = plane < 3 ? A.images + ((size_t)b * 3 + plane) * pl : A.heatmaps + ((size_t)b * 7 + (plane - 3)) * pl;
  // the host entry validated its copy of the table; the device copy is checked again so that no descriptor can index outside src
  if (!kptload_crop_ok(d, A.src_bytes)) {
    for (size_t i = tid; i < pl; i += 256) out[i] = 0.f;
    return;
  }
  if (plane >= 3) {
    double* rz = reinterpret_cast<double*>(smem);
    double* bl = rz + 2 * S;
    double* sums = bl + 2 * S;
    int* hot = reinterpret_cast<int*>(sums + 2);
    if (tid < 2) hot[tid] = d[KD_HOT + 2 * (plane - 3) + tid];
    __syncthreads();
    kpthm::axes(rz, bl, sums, hot, 1, w, h, S, tid, 256);
    kpthm::store(out, bl, sums, 1, S, tid, 256, A.vec != 0);
    return;
  }
  int* x0 = reinterpret_cast<int*>(smem);                      // byte offset of the tap's channel inside a source row
  int *x1 = x0 + S, *a0 = x0 + 2 * S, *a1 = x0 + 3 * S;
  int *y0 = x0 + 4 * S, *y1 = x0 + 5 * S, *b0 = x0 + 6 * S, *b1 = x0 + 7 * S;   // y0, y1: byte offset of the source row
  const int ch = 2 - plane;                                    // the crop is RGB, the output B, G, R
  for (int i = tid; i < 2 * S; i += 256) {
    int i0, i1, c0, c1;
    if (i < S) {
      make_tap_u8(i, S, w, true, i0, i1, c0, c1);
      x0[i] = i0 * 3 + ch; x1[i] = i1 * 3 + ch; a0[i] = c0; a1[i] = c1;
    } else {
      const int j = i - S;
      make_tap_u8(j, S, h, false, i0, i1, c0, c1);
      y0[j] = i0 * w * 3; y1[j] = i1 * w * 3; b0[j] = c0; b1[j] = c1;
    }
  }
  __syncthreads();
  const unsigned char* __restrict__ src = A.src + off;
  if (A.vec) {
    const int S4 = S >> 2;
    for (int i = tid; i < S * S4; i += 256) {
      const int y = i / S4, x = (i - y * S4) * 4;
      const unsigned char* r0 = src + y0[y];
      const unsigned char* r1 = src + y1[y];
      const int c0 = b0[y], c1 = b1[y];
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = image_value(r0, r1, x0[x + j], x1[x + j], a0[x + j], a1[x + j], c0, c1);
      *reinterpret_cast<f32x4_t*>(out + (size_t)i * 4) = o;
    }
  } else {
    for (int i = tid; i < S * S; i += 256) {
      const int y = i / S, x = i - y * S;
      out[i] = image_value(src + y0[y], src + y1[y], x0[x], x1[x], a0[x], a1[x], b0[y], b1[y]);
    }
  }
}

}  // namespace

extern "C" {

int mdcv_kptload_batch(const int* desc_host, const int* desc, int B, const unsigned char* src, long long src_bytes, int S, float* images,
                       float* heatmaps, void* stream) {
  if (!desc_host || !desc || !src || !images || !heatmaps) return MDCV_EARG;
  if (B <= 0 || B > 65535 || S < MDCV_KPTLOAD_MIN_SIZE || S > MDCV_KPTLOAD_MAX_SIZE || src_bytes <= 0 || src_bytes > 0x7fffffffll) return MDCV_EARG;
  for (int b = 0; b < B; ++b) {
    const int* d = desc_host + (size_t)b * MDCV_KPTLOAD_DESC;
    if (!kptload_crop_ok(d, src_bytes) || d[KD_RES0] != 0 || d[KD_RES1] != 0 || d[KD_RES2] != 0) return MDCV_EARG;
    for (int k = 0; k < 7; ++k) {
      const int x = d[KD_HOT + 2 * k], y = d[KD_HOT + 2 * k + 1];
      if (x < 0 || x >= d[KD_W] || y < 0 || y >= d[KD_H]) return MDCV_EARG;
    }
  }
  const int vec = (S % 4 == 0 && ((uintptr_t)images & 15) == 0 && ((uintptr_t)heatmaps & 15) == 0) ? 1 : 0;
  KptArgs a{desc, B, src, src_bytes, S, vec, images, heatmaps};
  MDCV_LAUNCH(kptload_kernel, dim3(10, (unsigned)B), dim3(256), (size_t)(32 * S + 32), (hipStream_t)stream, a);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
