// bf16 forward instantiations of the implicit-GEMM kernels (conv_gemm.h); a unit of its own so that the three sets of templates build in parallel.
#include "conv_gemm.h"

int mdcv_cd_bf16_fwd(const ConvArgs& a, hipStream_t st, int B) { return dispatch_conv<bf16_t, 0>(a, st, B); }
