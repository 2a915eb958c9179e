// cv2.resize's 8-bit INTER_LINEAR in OpenCV's fixed-point form, shared by the detect -> crop glue (pipeline.hip) and the key-point crop
// loader (kptload.hip); the rule is written out above crop_resize_u8_kernel in pipeline.hip and restated in numpy by
// oracle.pipeline_oracle.resize_bilinear_u8.
#pragma once
#include "common.h"

// tap d of a src -> dst axis: the two source indices and their 11-bit coefficients (x axis: clamp_weights; y axis: rows clamped)
__device__ __forceinline__ void make_tap_u8(int d, int dst, int src, bool clamp_weights, int& i0, int& i1, int& c0, int& c1) {
  const double sc = 1.0 / ((double)dst / (double)src);
  float f = (float)(((double)d + 0.5) * sc - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_weights) {
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
  }
  c0 = (int)rintf((1.f - f) * 2048.f);
  c1 = (int)rintf(f * 2048.f);
  i0 = s < 0 ? 0 : (s < src ? s : src - 1);
  i1 = s + 1 < 0 ? 0 : (s + 1 < src ? s + 1 : src - 1);
}

// VResizeLinear's 8-bit result of two horizontally blended rows d0, d1, then `/ 255.0` in double and one rounding to float
__device__ __forceinline__ float blend_rows_u8(int b0, int d0, int b1, int d1) {
  const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
  return (float)((double)(unsigned char)v / 255.0);
}
