// The per-image descriptor of csrc/kptaug.hip (include/mdcv_kptaug.h lists the words) and its check, which runs on the host (MDCV_EARG before
// any launch) and again in the kernel on the device copy (a failing image passes through and raises an error bit).
#pragma once

#define MDCV_KPTAUG_DESC 24

namespace {

enum { KA_FLAGS = 0, KA_INV = 1, KA_FWD = 7, KA_GAIN = 13, KA_BIAS = 16, KA_PAD = 19 };
enum { KA_APPLY = 1, KA_SWAP = 2 };

// Nothing in a row locates memory (the kernel clamps every index it forms), so the check is about meaning: no reserved flag bit, every
// float word finite (exponent field not all ones), the padding zero.  It holds for a pass-through row (apply == 0) as well.
__host__ __device__ inline bool kptaug_row_ok(const int* d) {
  if (d[KA_FLAGS] & ~(KA_APPLY | KA_SWAP)) return false;
  for (int k = KA_INV; k < KA_PAD; ++k)
    if ((d[k] & 0x7f800000) == 0x7f800000) return false;
  for (int k = KA_PAD; k < MDCV_KPTAUG_DESC; ++k)
    if (d[k] != 0) return false;
  return true;
}

}  // namespace
