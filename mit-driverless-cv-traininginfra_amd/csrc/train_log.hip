// The per-step bookkeeping of the reference's training loops in one launch (gfx950, wave64): the row a step's log line is formatted from, and
// the epoch's running sums, without a host read.
//
//   run_epoch     <- CVC-YOLOv3/train.py:54,63-64,74-76,81-90   (epoch_num_targets, epoch_losses[j] += batch_loss, the printed statement)
//   train_model   <- RektNet/train_eval.py:74-78                (total_loss[k] += loss.item())
//
// What the loops compute on Python floats is IEEE double addition of fp32 values, one step after the other.  One thread does exactly those
// additions, in that order, on a device accumulator; the only parallel part is the integer count of labelled targets, whose sum is exact in
// any order.  Contract: include/mdcv_hip.h.
#include <limits.h>

#include "../../include/mdcv_hip.h"
#include "common.h"

namespace {

struct LossSources { const float* p[MDCV_TRAIN_LOG_MAX_LOSSES]; };

// ONE workgroup.  rows: B*T targets of 5 floats; a target counts when more than one of its four box coordinates is > 0 (a NaN is not).
__global__ __launch_bounds__(256) void train_log_step_kernel(LossSources src, int n_losses, const float* __restrict__ targets, int rows,
                                                             double* __restrict__ acc, float* __restrict__ row) {
  __shared__ int red[4];
  const int tid = threadIdx.x;
  int cnt = 0;
  for (int r = tid; r < rows; r += 256) {
    const float* t = targets + (size_t)r * 5;
    const int pos = (t[1] > 0.f) + (t[2] > 0.f) + (t[3] > 0.f) + (t[4] > 0.f);
    cnt += pos > 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = cnt;
  __syncthreads();
  if (tid != 0) return;
  const int count = red[0] + red[1] + red[2] + red[3];
  for (int j = 0; j < MDCV_TRAIN_LOG_ROW; ++j) {
    float v = 0.f;
    if (j < n_losses) {
      v = src.p[j] ? *src.p[j] : 0.f;
      acc[j] += (double)v;
    } else if (j == n_losses) {
      v = (float)count;
      acc[j] += (double)count + 1e-12;
    }
    row[j] = v;
  }
}

}  // namespace

extern "C" {

int mdcv_train_log_step(const float* const* losses, int n_losses, const float* targets, int with_targets, int B, int T, double* acc,
                        float* row, void* stream) {
  if (!losses || !acc || !row || n_losses < 1 || n_losses > MDCV_TRAIN_LOG_MAX_LOSSES || B < 0 || T < 0) return MDCV_EARG;
  const long long rows = with_targets ? (long long)B * T : 0;
  if (rows > INT_MAX || (rows > 0 && !targets)) return MDCV_EARG;
  LossSources src;
  for (int j = 0; j < MDCV_TRAIN_LOG_MAX_LOSSES; ++j) src.p[j] = j < n_losses ? losses[j] : nullptr;
  MDCV_LAUNCH(train_log_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, src, n_losses, targets, (int)rows, acc, row);
  MDCV_CHECK_LAUNCH();
  return MDCV_OK;
}

}  // extern "C"
