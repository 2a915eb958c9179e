// fp32 (parity mode) instantiations of the implicit-GEMM kernels (conv_gemm.h): forward and data gradients.
#include "conv_gemm.h"

int mdcv_cd_f32_fwd(const ConvArgs& a, hipStream_t st, int B) { return dispatch_conv<float, 0>(a, st, B); }
int mdcv_cd_f32_dgrad(const ConvArgs& a, hipStream_t st, int B) { return dispatch_conv<float, 1>(a, st, B); }
int mdcv_cd_f32_s2(const ConvArgs& a, hipStream_t st, int B) { return dispatch_dgrad_s2<float>(a, st, B); }
