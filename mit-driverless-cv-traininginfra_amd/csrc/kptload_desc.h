// The per-crop descriptor of the key-point crop loader (csrc/kptload.hip; mdcv/data/crops.py writes it).  Its length and the loader's
// bounds (MDCV_KPTLOAD_DESC, _MIN_SIZE, _MAX_SIZE: the target side S; _MAX_SIDE: decoded crop height and width) are the public header's:
// one definition, and the entry point's definition is checked against its declaration.
#pragma once
#include "../../include/mdcv_hip.h"

enum { KD_SRC_OFF, KD_H, KD_W, KD_RES0, KD_HOT, KD_RES1 = 18, KD_RES2 = 19 };   // KD_HOT + 2 * k: x of key point k, + 1: its y

// The crop a descriptor names lies inside src.  The same test runs on the host (MDCV_EARG) and in the kernel (on the device copy, which the
// host never sees): no descriptor can make the kernel read outside its buffer.  The hot pixels index nothing.
__host__ __device__ inline bool kptload_crop_ok(const int* d, long long src_bytes) {
  if (d[KD_H] < 1 || d[KD_W] < 1 || d[KD_H] > MDCV_KPTLOAD_MAX_SIDE || d[KD_W] > MDCV_KPTLOAD_MAX_SIDE) return false;
  return d[KD_SRC_OFF] >= 0 && (long long)d[KD_SRC_OFF] + 3LL * d[KD_H] * d[KD_W] <= src_bytes;
}
