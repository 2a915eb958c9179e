// The per-frame descriptor of the detect-and-draw kernels (csrc/detect_draw.hip, csrc/kpt_detect.hip; mdcv/yolo/detect.py writes it): a
// decoded frame (uint8, HWC, RGB, rows of 3 * W bytes) where it lies in a device pool, and letterbox()'s ratio and pads.  Its length is the
// public header's MDCV_DETECT_DESC.
#pragma once
#include "../../include/mdcv_hip.h"

constexpr int kDetectMaxSide = 1 << 24;

enum { DD_OFF = 0, DD_W = 1, DD_H = 2, DD_RATIO = 3, DD_PAD_W = 4, DD_PAD_H = 5 };

// a frame descriptor is good when its frame lies inside the pool (64-bit arithmetic) and its pads are ints.  The same test runs on the
// host (MDCV_EARG) and in the kernels (on the device copy, which the host never sees): no descriptor can index outside the pool.
__host__ __device__ inline bool detect_frame_ok(const long long* d, long long pool_bytes) {
  const long long off = d[DD_OFF], W = d[DD_W], H = d[DD_H];
  if (off < 0 || W < 1 || H < 1 || W > kDetectMaxSide || H > kDetectMaxSide) return false;
  if (d[DD_PAD_W] < -kDetectMaxSide || d[DD_PAD_W] > kDetectMaxSide || d[DD_PAD_H] < -kDetectMaxSide || d[DD_PAD_H] > kDetectMaxSide) return false;
  return off <= pool_bytes && 3 * W * H <= pool_bytes - off;
}

__host__ __device__ inline double detect_desc_ratio(const long long* d) {
  union { long long i; double f; } u;
  u.i = d[DD_RATIO];
  return u.f;
}
