// Internal interface between conv_igemm.hip (weight-gradient entry points and family chooser), wgrad_gemm.hip (the generic implicit-GEMM
// weight-gradient kernels) and wgrad_reduce.hip (slabs -> OIHW gradient).
#pragma once
#include <hip/hip_runtime.h>

// geometry of one weight-gradient call, packed once per entry point (channel counts and strides are the padded ones)
struct WgradGeom {
  int dtype, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, dil;
  long long dy_ldc, x_ldc;
};

// generic kernels: every split writes its fp32 slab ws[split][Cout][KH*KW*Cin]; `splits` must be what mdcv_conv2d_wgrad_splits gives for the geometry
int launch_wgrad_gemm(const WgradGeom& g, const void* dy, const void* x, float* ws, int splits, hipStream_t st);
// narrow kernel with the BatchNorm-backward apply in its operand load (bf16, Cout <= 32; g.dy_ldc is the stride of dz)
int launch_wgrad_gemm_bnapply(const WgradGeom& g, const void* dz, const void* y, int y_ldc, const float* scale, const float* shift, const float* cA,
                              const float* cB, const float* cC, int act, float slope, int Cout_real, const void* x, float* ws, int splits,
                              hipStream_t st);
// sums the fp32 slabs ws[splits][Cout_pad][KK*Cin_pad] into the OIHW gradient
int launch_wgrad_reduce(const float* ws, float* dw_oihw, int splits, int Cout_pad, int Cout_real, int Cin_pad, int Cin_real, int KK, int accumulate,
                        hipStream_t st);
