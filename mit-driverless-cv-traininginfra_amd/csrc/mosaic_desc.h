// The per-image descriptor of csrc/mosaic.hip (include/mdcv_aug.h lists the words) and its check, which runs on the host (MDCV_EARG before
// any launch) and again in the kernel on the device copy (a failing image passes through and raises an error bit).
#pragma once

#define MDCV_MOSAIC_DESC 8

namespace {

enum { M_APPLY = 0, M_XC = 1, M_YC = 2, M_S0 = 3, M_RES = 7 };

// Everything that locates memory: the centre splits both axes into two non-empty runs, every source is an image of the batch.  A
// pass-through row (apply == 0) reads nothing but its own image, so its other words are free.
__host__ __device__ inline bool mosaic_row_ok(const int* d, int B, int H, int W) {
  if (d[M_APPLY] == 0) return true;
  if (d[M_APPLY] != 1) return false;
  if (d[M_XC] < 1 || d[M_XC] > W - 1 || d[M_YC] < 1 || d[M_YC] > H - 1) return false;
  for (int q = 0; q < 4; ++q)
    if (d[M_S0 + q] < 0 || d[M_S0 + q] >= B) return false;
  return d[M_RES] == 0;
}

}  // namespace
