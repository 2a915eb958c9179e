// bf16 data-gradient instantiations of the implicit-GEMM kernels (conv_gemm.h): stride 1, the stride-2 parity classes one by one and all in one launch.
#include "conv_gemm.h"

int mdcv_cd_bf16_dgrad(const ConvArgs& a, hipStream_t st, int B) { return dispatch_conv<bf16_t, 1>(a, st, B); }
int mdcv_cd_bf16_s2(const ConvArgs& a, hipStream_t st, int B) { return dispatch_dgrad_s2<bf16_t>(a, st, B); }
int mdcv_cd_bf16_s2_all(const ConvArgs& a, hipStream_t st, int B) { return dispatch_dgrad_s2_all(a, st, B); }
