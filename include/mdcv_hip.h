/* libmdcv_hip.so — C ABI of the MI355X (gfx950) hot path of CVC-YOLOv3 + RektNet training.
 *
 * The reference (cv-core/MIT-Driverless-CV-TrainingInfra) has NO native/FFI layer: its hot path is Python calling
 * stock torch ops.  This ABI is therefore the boundary the reference *would* bind if it had one; each entry point
 * names the reference call site(s) it replaces.  Conventions:
 *   - plain C symbols, plain pointers and sizes; the CALLER owns every buffer (device memory), kernels allocate nothing
 *   - enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), no synchronisation inside
 *   - return 0 on success, a negative MDCV_E* for argument errors, or a positive hipError_t
 *   - dtype: 0 = fp32 (parity mode, exact-f32 MFMA), 1 = bf16 (production, fp32 accumulate)
 *   - activations are NHWC with an explicit channel stride `ld*` (elements); channel counts are padded to a multiple
 *     of 8 and pad channels hold exact zeros; weights/gradients at the boundary are OIHW fp32 like torch parameters
 */
#ifndef MDCV_HIP_H
#define MDCV_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define MDCV_OK 0
#define MDCV_EARG (-1)
#define MDCV_F32 0
#define MDCV_BF16 1
/* The library holds NO mutable process state (round 5): a call's result depends on its arguments only.  The dispatch heuristics that were A/B-ed
 * on the training step (csrc/tune.h: one documented knob each) can be overridden PER CALL through the dtype argument of the convolution and
 * weight-gradient entry points: bits 0..7 = MDCV_F32 / MDCV_BF16, the bits above = a signed variant code of that entry point's family (0 =
 * defaults; the code tables are in csrc/tune.h).  Plan-time queries (mdcv_conv2d_stats_rows_geom, mdcv_conv2d_wgrad_splits_geom, ...) take the same
 * tuned dtype as the launch they size buffers for. */
#define MDCV_TUNED(dtype, code) (((dtype) & 0xff) | ((code) * 256))
#define MDCV_ACT_NONE 0
#define MDCV_ACT_LEAKY 1
#define MDCV_ACT_RELU 2

/* ---- convolution (nn.Conv2d fwd/bwd: CVC-YOLOv3/models.py:59-65 ; RektNet/keypoint_net.py:17,25 ; RektNet/resnet.py:12-19)
 * mode 0: forward.  in=[B,Hin,Win,Cin], out=[B,Hout,Wout,Nout], w_packed=[Nout][KH*KW][Cin] (from mdcv_pack_weights w_fwd).
 * mode 1: data gradient.  in=dY [B,Hin,Win,Cin=Cout_pad] on the conv's OUTPUT grid, out=dX on the conv's INPUT grid
 *         [B,Hout,Wout,Nout=Cin_pad], w_packed=[Cin_pad][KH*KW][Cout_pad] (w_dgrad).  stride in {1,2}.
 * bias (fp32[Nout]) is added before statistics; addsrc (same layout as out) is added after (residual / fan-out grads);
 * stats_partial, if given, receives [mdcv_conv2d_stats_rows(M)][2][Nout] fp32 = per-tile (sum, sum^2) per channel. */
int mdcv_conv2d(int dtype, int mode, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc,
                const float* bias, const void* addsrc, int add_ldc, float* stats_partial,
                int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout,
                int KH, int KW, int stride, int pad, int dil, void* stream);
/* Inference forward (Darknet.forward / KeypointNet.forward in eval mode: conv -> BatchNorm(running stats) -> activation, models.py:48-72,
 * resnet.py:22-27): out = act(conv(in) * scale[n] + shift[n]) (+ addsrc, e.g. the shortcut input), scale/shift from mdcv_bn_eval_coeffs
 * (or scale = NULL: bias only).  act: MDCV_ACT_*.  The raw conv output never goes to HBM. */
int mdcv_conv2d_affine_act(int dtype, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc, const float* scale,
                           const float* shift, const void* addsrc, int add_ldc, int act, float slope, int B, int Hin, int Win, int Cin,
                           int Hout, int Wout, int Nout, int KH, int KW, int stride, int pad, int dil, void* stream);
/* Data gradient (mode 1, same geometry arguments as mdcv_conv2d) that also writes the BatchNorm-backward partial sums of the layer
 * whose output gradient it produces: partial[row][0][c] = sum g, partial[row][1][c] = sum g*(y - mean), g = dz * act'(scale*y + shift),
 * one row per 128 output positions (y: that layer's raw conv output, same pixel/channel indexing as the gradient written to `out`).
 * _rows() = number of rows written, or 0 when the geometry / dtype (bf16 only) cannot take the fused path.  Finish with mdcv_bn_bwd_finalize_rows. */
int mdcv_conv2d_dgrad_bnsums_rows(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride,
                                  int pad, int dil, int in_ldc);
int mdcv_conv2d_dgrad_bnsums(int dtype, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc, const void* addsrc,
                             int add_ldc, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride,
                             int pad, int dil, const void* y, int ldy, const float* scale, const float* shift, const float* mean, int act,
                             float slope, float* partial, void* stream);
/* The network's FIRST conv -> BatchNorm(batch statistics) -> activation (CVC-YOLOv3/models.py:57-71 at index 0; 3 -> 32 channels, 3x3 / stride 1 / pad 1) as two
 * streaming launches that never re-read the layer's 354 MB output: the conv is 25 GFLOP on an 88 MB input, so it is computed twice.  _stats: x -> partial rows
 * [mdcv_first_conv_rows(B, H)][2][32] (sum, sum of squares of the fp32 accumulators; finish with mdcv_bn_stats_finalize).  _bn_act: x -> y (raw conv output, bf16, kept
 * for the backward) AND z = act(scale * y + shift) from the y it stores, in one store loop.  _ok: 1 where the geometry takes this form (bf16, 8 padded input
 * channels at stride 8, 32 output channels); elsewhere: mdcv_conv2d + mdcv_bn_act_fwd. */
int mdcv_first_conv_ok(int dtype, int B, int H, int W, int Cin_pad, int Cout_pad, int KH, int KW, int stride, int pad, int dil, int ldx);
int mdcv_first_conv_rows(int B, int H);
int mdcv_first_conv_stats(int dtype, const void* x, int ldx, const void* w_packed, float* partial, int B, int H, int W, void* stream);
int mdcv_first_conv_bn_act(int dtype, const void* x, int ldx, const void* w_packed, const float* scale, const float* shift, int act, float slope,
                           void* y, int ldy, void* z, int ldz, int B, int H, int W, void* stream);
/* 1 when the data gradient of this geometry runs as the stride-2 form of the 3x3 shift kernel (bf16, 3x3 / stride 2 / pad 1, Hout = 2 Hin, 32 or 64
 * output channels): its store loop writes whole output rows from LDS and carries the fused sums at every size (one partial row per 8 x 31 tile). */
int mdcv_conv2d_dgrad_s2_form_ok(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride,
                                 int pad, int dil, int in_ldc);
/* Forward statistics through EXACT ACCUMULATORS (csrc/exact_acc.h): the conv's epilogue adds its per-tile sums (per output channel: sum, sum of
 * squares) to xacc = [reps][3][2][Nout] signed 64-bit words (mdcv_xstats_words; ZERO before the launch) with fire-and-forget integer atomics --
 * three 40-bit digits of a fixed-point number with quantum 2^-70, so every addition is exact and the totals do not depend on the order the
 * atomics land in (bit-reproducible, unlike float atomics).  reps (a power of two; mdcv_xstats_reps(rows, C) for a layer that performs `rows`
 * additions per channel, rows = mdcv_conv2d_stats_rows_geom / mdcv_pw_rows) spreads a word's additions over replicas.  Every forward kernel of
 * mdcv_conv2d carries it (both dtypes), and mdcv_pw_conv_fwd_xstats is mdcv_pw_conv_fwd with the same sink.  Consumer: mdcv_bn_act_fwd_xstats --
 * BatchNorm(batch statistics) + activation (+ residual) whose prologue adds the replicas and forms the statistics; it writes scale / shift /
 * mean / invstd / running statistics as mdcv_bn_stats_finalize does (C <= 1024).  Replaces conv -> mdcv_bn_stats_finalize -> mdcv_bn_act_fwd of
 * the reference's nn.Sequential(conv, BatchNorm2d, LeakyReLU) (CVC-YOLOv3/models.py:57-71) by two launches with no hand-off inside a launch. */
int mdcv_xstats_words(int reps, int C);
int mdcv_xstats_reps(int rows, int C);
int mdcv_conv2d_xstats(int dtype, const void* in, int in_ldc, const void* w_packed, void* out, int out_ldc, const float* bias, void* xacc,
                       int reps, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Nout, int KH, int KW, int stride, int pad, int dil,
                       void* stream);
int mdcv_pw_conv_fwd_xstats(int dtype, const void* y, int ldy, const float* scale, const float* shift, const void* resid, int ldr, int act,
                            float slope, void* z_out, int ldz, const void* w_packed, const float* bias, void* out, int out_ldc, void* xacc,
                            int reps, long long M, int K, int N, void* stream);
int mdcv_bn_act_fwd_xstats(int dtype, const void* y, int ldy, const void* xacc, int reps, double count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift, float* mean,
                           float* invstd, const void* resid, int ldr, void* out, int ldo, int M, int C, int act, float slope, void* stream);
int mdcv_conv2d_stats_rows(int M);      /* generic kernels: one row per 128 output pixels */
/* rows of stats_partial a FORWARD launch with this geometry writes (use this one to size the buffer: the 3x3 / stride-1 /
 * pad-1 shift kernel walks a padded pixel stream and writes more rows than M / 128; every row it returns is written). */
int mdcv_conv2d_stats_rows_geom(int dtype, int B, int Hout, int Wout, int Cin, int Nout, int KH, int KW, int stride, int pad, int dil,
                                int in_ldc);

/* weight gradient: dW (OIHW fp32, real channel counts) = dY^T * im2col(X).  ws = splits*Cout*KH*KW*Cin floats of scratch. */
int mdcv_conv2d_wgrad_splits(int dtype, int M, int Cout, int Ktot);
/* number of fp32 slabs for the kernel mdcv_conv2d_wgrad picks for this geometry (3x3 stride-1 layers with 128-multiple channel
 * counts run a kernel whose kw taps share one activation tile and that wants its own split); ws = splits*Cout*KH*KW*Cin floats. */
int mdcv_conv2d_wgrad_splits_geom(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int KH, int KW, int stride,
                                  int pad, int dil, int dy_ldc, int x_ldc);
int mdcv_conv2d_wgrad(int dtype, const void* dy, int dy_ldc, const void* x, int x_ldc, float* ws, int splits,
                      float* dw_oihw, int accumulate, int B, int Hin, int Win, int Cin, int Cin_real,
                      int Hout, int Wout, int Cout, int Cout_real, int KH, int KW, int stride, int pad, int dil, void* stream);

/* OIHW fp32 parameters -> GEMM operand layouts (w_dgrad may be NULL) */
int mdcv_pack_weights(int dtype, const float* w_oihw, void* w_fwd, void* w_dgrad, int Cout, int Cin, int KH, int KW,
                      int Cout_pad, int Cin_pad, void* stream);

/* all convs of a network in ONE launch; table = nlayers device-resident 72-byte records
 *   { const float* w_oihw; void* w_fwd; void* w_dgrad|NULL; int Cout, Cin, KH*KW, Cout_pad, Cin_pad; int reserved[3];
 *     const float* bias|NULL; float* bias_padded; }   (bias: the fp32 bias parameter, copied into the padded operand buffer) */
int mdcv_pack_weights_batched(int dtype, const void* table, int nlayers, int max_taps, void* stream);   /* max_taps = max KH*KW (times Cin_pad/64 scaling is internal) */

/* ---- layout conversion at the API edge (reference tensors are NCHW fp32: train.py:60, train_eval.py:60) */
int mdcv_nchw_to_nhwc(int dtype, const float* src, void* dst, int B, int C, int H, int W, int ldc, int Cpad, void* stream);
int mdcv_nhwc_to_nchw(int dtype, const void* src, int ldc, float* dst, int B, int C, int H, int W, void* stream);

/* ---- BatchNorm2d (eps 1e-5, momentum 0.1) + LeakyReLU/ReLU + shortcut add (models.py:66-71,325-327 ; resnet.py:22-27) */
int mdcv_partial_reduce(const float* partial, int rows, int nsums, int C, double* accum, void* stream);
int mdcv_bn_finalize(double* accum, double count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float momentum, float eps, float* scale, float* shift, float* mean, float* invstd, int C, void* stream);
int mdcv_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                        float* scale, float* shift, int C, void* stream);
/* the same for a conv that has its own bias in front of the BatchNorm (RektNet): shift also absorbs conv_bias * scale, so that
 * mdcv_conv2d_affine_act(scale, shift) == BatchNorm_eval(conv + bias).  conv_bias may be NULL. */
int mdcv_bn_eval_coeffs_bias(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                             const float* conv_bias, float* scale, float* shift, int C, void* stream);
/* out = act(y1*s1+b1 [+ y2*s2+b2]) [+ resid] */
int mdcv_bn_act_fwd(int dtype, const void* y1, int ld1, const float* s1, const float* b1, const void* y2, int ld2, const float* s2,
                    const float* b2, const void* resid, int ldr, void* out, int ldo, int M, int C, int act, float slope, void* stream);
int mdcv_bn_act_bwd_reduce_ws_floats(int dtype, int M, int C, int nsums);
/* partial rows -> statistics -> scale/shift (+ running stats) in ONE launch while rows <= 4096 (a workgroup owns 16 channels and
 * sums their rows itself); larger buffers are first folded to 64 rows IN PLACE by one more launch (no atomics; `partial` is the
 * caller's scratch and is consumed -- hence not `const`).  `accum` is unused (kept for the two-stage entry points mdcv_partial_reduce / mdcv_bn_finalize). */
int mdcv_bn_stats_finalize(float* partial, int rows, double* accum, double count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift, float* mean,
                           float* invstd, int C, void* stream);
/* mdcv_bn_act_bwd_reduce + mdcv_bn_bwd_finalize for one BatchNorm (y2 == NULL) or the fused residual pair, two launches in all. */
int mdcv_bn_act_bwd_reduce_finalize(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1,
                                    const float* mean1, const float* invstd1, const void* y2, int ld2, const float* s2, const float* b2,
                                    const float* mean2, const float* invstd2, float* partial_ws, int M, int C, int act, float slope,
                                    double count, const float* gamma1, float* dgamma1, float* dbeta1, float* cA1, float* cB1, float* cC1,
                                    const float* gamma2, float* dgamma2, float* dbeta2, float* cA2, float* cB2, float* cC2, void* stream);
/* finalize for the fused data-gradient sums: rows x [2][C] partials (sum g, sum g*(y-mean)) -> dgamma, dbeta, cA, cB, cC
 * (more than 4096 rows are folded in place first, as above: `partial` is consumed) */
int mdcv_bn_bwd_finalize_rows(float* partial, int rows, int C, double count, const float* gamma, const float* mean,
                              const float* invstd, float* dgamma, float* dbeta, float* cA, float* cB, float* cC, void* stream);
int mdcv_bn_act_bwd_reduce(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1,
                           const float* mean1, const float* invstd1, const void* y2, int ld2, const float* s2, const float* b2,
                           const float* mean2, const float* invstd2, double* accum, float* partial_ws, int M, int C, int act, float slope,
                           void* stream);
int mdcv_bn_bwd_finalize(double* accum, int kx, int nsums, int zero_after, double count, const float* gamma, const float* mean,
                         const float* invstd, float* dgamma, float* dbeta, float* cA, float* cB, float* cC, int C, void* stream);
int mdcv_bn_act_bwd_apply(int dtype, const void* dout, int ldd, const void* y1, int ld1, const float* s1, const float* b1,
                          const float* cA1, const float* cB1, const float* cC1, void* dy1, int ldy1,
                          const void* y2, int ld2, const float* s2, const float* b2, const float* cA2, const float* cB2,
                          const float* cC2, void* dy2, int ldy2, int M, int C, int act, float slope, void* stream);
int mdcv_colsum(int dtype, const void* x, int ldc, int M, int C, double* accum, void* stream);
/* the same sums without atomics: per-block partial rows in partial_ws (mdcv_colsum_ws_floats floats), then one reduce launch -> out[C] */
int mdcv_colsum_ws_floats(int dtype, int M, int C);
int mdcv_colsum_f32(int dtype, const void* x, int ldc, int M, int C, float* partial_ws, float* out, void* stream);
int mdcv_accum_to_f32(double* accum, float* out, int n, int zero_after, void* stream);

/* ---- nn.Upsample(scale 2, nearest) fwd/bwd (models.py:86-88); H,W are the LOW-resolution dims */
int mdcv_upsample2x_fwd(int dtype, const void* in, int ldi, void* out, int ldo, int B, int H, int W, int C, void* stream);
int mdcv_upsample2x_bwd(int dtype, const void* dout, int ldo, void* din, int ldi, int B, int H, int W, int C, void* stream);

/* ---- nn.MaxPool2d(2,2) and nn.ZeroPad2d((0,1,0,1)) + nn.MaxPool2d(2,1) of yolo_baseline_tiny.cfg (models.py:74-84).
 * H,W = input dims; output is H/2 x W/2 (stride 2) or H x W (stride 1); idx [B,Ho,Wo,C] bytes = winning window slot for backward */
int mdcv_maxpool2x2_fwd(int dtype, const void* in, int ldi, void* out, int ldo, unsigned char* idx, int B, int H, int W, int C, int stride,
                        void* stream);
int mdcv_maxpool2x2_bwd(int dtype, const void* dout, int ldo, const unsigned char* idx, void* din, int ldi, int B, int H, int W, int C, int stride,
                        void* stream);

/* generic forms of the two (models.py:74-88 builds nn.MaxPool2d(size, stride, (size - 1) // 2) and nn.Upsample(scale_factor = stride) for any
 * size / stride): window k <= 15, -inf padding (pad < k), Ho = (H + 2*pad - k) / stride + 1; idx = kh*k + kw of the first maximum;
 * backward gathers over the windows that contain an input pixel (no atomics).  H, W = input dims. */
int mdcv_maxpool_fwd(int dtype, const void* in, int ldi, void* out, int ldo, unsigned char* idx, int B, int H, int W, int C, int k, int stride,
                     int pad, void* stream);
int mdcv_maxpool_bwd(int dtype, const void* dout, int ldo, const unsigned char* idx, void* din, int ldi, int B, int H, int W, int C, int k, int stride,
                     int pad, void* stream);
int mdcv_upsample_fwd(int dtype, const void* in, int ldi, void* out, int ldo, int B, int H, int W, int C, int scale, void* stream);
int mdcv_upsample_bwd(int dtype, const void* dout, int ldo, void* din, int ldi, int B, int H, int W, int C, int scale, void* stream);

/* ---- YOLOLayer.forward (models.py:140-220) + build_targets / bbox_iou (utils/utils.py:163-275)
 * logits NHWC, channel = a*(5+C)+attr.  anchors_scaled = anchors/stride, fp32 [A][2].  targets fp32 [B][T][5].
 * train: out7[0] += loss, out7[1..6] += (x,y,w,h,obj,noobj) parts; dlogits = d loss / d logits (* *gscale if given). */
long long mdcv_yolo_head_workspace_bytes(int B, int A, int Gh, int Gw);
int mdcv_yolo_head_train(int dtype, const void* logits, int ldc, void* dlogits, int ldd, int Cpad, const float* targets,
                         const float* anchors_scaled, int B, int T, int A, int C, int Gh, int Gw, float thresh, float xy_loss,
                         float wh_loss, float obj_loss, float noobj_loss, void* workspace, float* out7, const float* gscale,
                         void* stream);
int mdcv_yolo_head_grad(int dtype, const void* logits, int ldc, void* dlogits, int ldd, int Cpad, const float* targets,
                        const float* anchors_scaled, int B, int T, int A, int C, int Gh, int Gw, float thresh, float xy_loss,
                        float wh_loss, float obj_loss, float noobj_loss, void* workspace, const float* gscale, void* stream);
int mdcv_yolo_head_decode(int dtype, const void* logits, int ldc, const float* anchors_scaled, float stride, int B, int A, int C, int Gh,
                          int Gw, float* out, int rows_total, int row_off, void* stream);
/* utils.bbox_iou (utils/utils.py:163-193, "+1 pixel" convention) for n = max(n1, n2) box pairs; a side with ONE row is broadcast.  Rows are `stride`
 * floats apart, the first four are the box (corners = 1: x1 y1 x2 y2; 0: cx cy w h).  fp32; every operation rounds where the reference's torch op
 * rounds, NaN propagates as torch.max / torch.min / clamp propagate it: bit-identical to the reference. */
int mdcv_bbox_iou(const float* box1, long long n1, int stride1, const float* box2, long long n2, int stride2, int corners, float* out, void* stream);
long long mdcv_build_targets_workspace_bytes(int B, int T, int A, int Gh, int Gw);
int mdcv_build_targets(const float* targets, const float* anchors, int B, int T, int A, int C, int Gh, int Gw, float thresh,
                       unsigned char* mask, unsigned char* conf_mask, float* tx, float* ty, float* tw, float* th, float* tconf,
                       unsigned char* tcls, void* workspace, int* err_out, void* stream);

/* ---- KeypointNet head (keypoint_net.py:46-56,68-70) and CrossRatioLoss (cross_ratio_loss.py:20-63) */
/* the head's 1x1 conv (keypoint_net.py:40,68: `self.out`, Conv2d(128, 7, 1)) with fp32 logits out of bf16 features: x [M][ldx] bf16 NHWC (C % 32 == 0,
 * C <= 1024), w = the fp32 weights [K][C] as the module holds them, bias [K] or NULL, out fp32 [M][8] (columns >= K are zeros), K <= 8 */
int mdcv_head1x1_f32(const void* x_bf16, int ldx, const float* w, const float* bias, float* out, long long M, int C, int K, void* stream);
int mdcv_softargmax_fwd(int dtype, const void* logits, int ldc, int B, int K, int H, int W, float* hm, float* pts, void* stream);
int mdcv_softargmax_bwd(int dtype, const float* hm, const float* pts, const float* dpts, const float* dhm, float* sdot_ws, int B, int K,
                        int H, int W, void* dlogits, int ldd, void* stream);
int mdcv_cross_ratio_loss(const float* hm, const float* pts, const float* thm, const float* tpts, int B, int H, int W, int loss_type,
                          int include_geo, float gamma_horz, float gamma_vert, double* acc_ws, const float* gscale, float* out3,
                          float* dpts, float* dhm, void* stream);

/* ---- RektNet validation of a whole batch in ONE launch (csrc/kpt_eval.hip): replaces the per-image loop of eval_model
 *      (RektNet/train_eval.py:115-138, a DataLoader of batch_size 1 and three .item() per image) and of print_kpt_L2_distance (:140-186).
 * rows [B][MDCV_KPT_EVAL_ROW] fp32, 16-byte aligned; row i = loc, geo, total, d0 .. d6, 0, 0:
 *   loc, geo, total   what CrossRatioLoss(loss_type, include_geo, gamma_horz, gamma_vert) returns for sample i ALONE (hm[i:i+1], pts[i:i+1], ...):
 *                     loc = sum of the 14 squared (0) / absolute (2) point differences, or of the 7 H W squared heat-map differences (1);
 *                     geo = gamma_horz (hA + hB) / 2 + gamma_vert (vA + vB + vC + vD) / 4, each term 1 - u.v of THIS sample's unit vectors
 *                     (F.normalize's eps 1e-12: coincident points give a zero vector); geo = 0 and total = loc without include_geo.
 *                     NOT what mdcv_cross_ratio_loss gives for the batch: its geo is the mean of a [B,B] all-pairs matrix.
 *   d_k               sqrt((dist_sx (p_kx - t_kx))^2 + (dist_sy (p_ky - t_ky))^2): utils.calculate_distance's pixel distance when the caller
 *                     passes dist_sx = C input_size[0], dist_sy = C input_size[1] with C = x_batch.shape[1] = 3 -- the reference multiplies
 *                     the normalised points by the image's CHANNEL count before input_size (train_eval.py:152-157); reproduced, not corrected.
 * fp32 differences and products, fp64 accumulation, one rounding per output; NaN / Inf stay inside their own sample.  Row i is the same bits
 * whatever B is and wherever sample i stands in the batch.  loss_type 0 / 2 never read hm / thm (both may be NULL).  Nothing is written
 * beyond row B - 1.  MDCV_EARG before any launch: NULL pts / tpts / rows, rows not 16-byte aligned, B < 1 or B > 65535, loss_type outside
 * 0..2, and for loss_type 1 NULL hm / thm, H < 1, W < 1 or 7 H W > INT_MAX. */
#define MDCV_KPT_EVAL_ROW 12
int mdcv_kpt_eval_rows(const float* hm, const float* pts, const float* thm, const float* tpts, int B, int H, int W, int loss_type, int include_geo,
                       float gamma_horz, float gamma_vert, float dist_sx, float dist_sy, float* rows, void* stream);

/* ---- detection post-processing: replaces the per-image Python loop validate.py:80-141, the sequential
 *      greedy NMS utils/nms.py:4-61 and average_precision/compute_ap utils/utils.py:58-119.
 *      Visiting order: descending score, equal scores by descending index (the reference's ascending sort walked from the
 *      back, nms.py:25-32; its CPU sort is unstable past 16 elements, so for ties this is the stable-sort behaviour).
 *      top_k <= MDCV_NMS_MAX_TOPK (the reference always uses 200, nms.py:4 / validate.py:93); larger is MDCV_EARG. */
#define MDCV_NMS_MAX_TOPK 512
long long mdcv_nms_workspace_bytes(int n);
/* boxes [n,4] corner format, scores [n]; keep[0..*count) <- kept indices in visiting order (keep has room for min(n,top_k));
 * count is a device int.  n == 0 gives *count = 0 (nms.py:17-18). */
int mdcv_nms(const float* boxes, const float* scores, int n, float overlap, int top_k, long long* keep, int* count, void* workspace,
             void* stream);
long long mdcv_detect_post_workspace_bytes(int B, int N);
/* pred [B,N,5+C] eval-mode rows (cx,cy,w,h,conf,cls...), targets [B,T,5] zero-padded (cls,cx,cy,w,h) or NULL with T = 0.
 * Per image b: out_count[b] kept detections in descending confidence; out_boxes [B,top_k,4] corner, out_prob, out_cls (first
 * argmax), out_index (row in N), out_correct [B,top_k]; out_stats [B,4] = (AP, recall, precision, valid) with valid = 0 where the
 * reference loop `continue`s (no detection kept, validate.py:97, or no real label, validate.py:120). */
int mdcv_detect_post(const float* pred, int B, int N, int C, const float* targets, int T, float conf_thres, float nms_thres,
                     float iou_thres, float width, float height, int top_k, float* out_boxes, float* out_prob, int* out_cls,
                     long long* out_index, unsigned char* out_correct, int* out_count, float* out_stats, void* workspace,
                     void* stream);
/* utils.py:58-88 on its own: tp u8[m], conf f32[m], 1 <= m <= MDCV_NMS_MAX_TOPK; out3 = (AP, recall, precision). */
int mdcv_average_precision(const unsigned char* tp, const float* conf, int m, int n_gt, float* out3, void* stream);

/* ---- detect -> crop -> keypoints glue.  Cuts box k < count[b] of frame b out of frames [B,C,H,W] (fp32) and
 *      resamples it to out_h x out_w with cv2.resize's default bilinear rule (RektNet/utils.py:73-76 prep_image; layout of
 *      RektNet/detect.py:33-35: [M,C,out_h,out_w]).  Boxes [B,K,4] are corner boxes in detector coordinates and are mapped to
 *      frame pixels as x * scale_x + off_x (CVC-YOLOv3/detect.py:98-101), rounded outwards and clamped to the frame.
 *      Crops are packed image-major: out row m, owner[m] = b, *total = M (device ints; out / owner hold B*K rows).
 *      out_h, out_w <= 256. */
int mdcv_crop_resize(const float* frames, int B, int C, int H, int W, const float* boxes, const int* count, int K, float scale_x,
                     float scale_y, float off_x, float off_y, int out_h, int out_w, float* out, int* owner, int* total, void* stream);

/* The same cut with the rule the reference's loaders actually apply (RektNet/dataset.py:35-38,52, RektNet/detect.py:29-35): the frame
 * is a uint8 image [B,C,H,W], cv2.resize runs its 8-bit fixed-point INTER_LINEAR (11-bit coefficients, result rounded to 8 bits), and
 * only then is the crop divided by 255: out = (float)(u8 / 255.0). */
int mdcv_crop_resize_u8(const unsigned char* frames, int B, int C, int H, int W, const float* boxes, const int* count, int K, float scale_x,
                        float scale_y, float off_x, float off_y, int out_h, int out_w, float* out, int* owner, int* total, void* stream);

/* ---- on-device synthetic cone data with the output contracts of the reference's datasets; every value is a pure
 *      function of (seed, step, index), reproduced bit for bit by oracle/synth_oracle.py.
 *      detector batch (CVC-YOLOv3/utils/datasets.py:124-315): images [B,3,H,W] in [0,1], targets [B,T,5] (cls,cx,cy,w,h), zero rows last.
 *      crop batch (RektNet/dataset.py:34-56, RektNet/utils.py:83-111): images [B,3,80,80], heat-maps [B,7,80,80], points [B,7,2]. */
int mdcv_synth_cone_batch(unsigned int seed, int step, int B, int T, int H, int W, int num_classes, float* images, float* targets, void* stream);
int mdcv_synth_crop_batch(unsigned int seed, int step, int B, int size, float* images, float* heatmaps, float* points, void* stream);

/* ---- real-image detector batches (csrc/imgload.hip; CVC-YOLOv3/utils/datasets.py:124-315 ImageLabelDataset.__getitem__, image half):
 *      decoded uint8 RGB source windows -> Pillow's 8-bit convolution resize (horizontal pass into a uint8 scratch, then vertical), the
 *      127 padding and patch crop around it, convert('L') when C == 1, hflip, and to_tensor's /255 into out [B,C,H,W] fp32; byte-exact.
 *      The resize input is a VIRTUAL image: a 127 canvas holding the window's bytes, so padding in front of the filter (the pad-and-resize
 *      path) reads 127 at the border taps.  One descriptor of MDCV_IMGLOAD_DESC ints per image (mdcv/data/images.py writes them):
 *       [0] src_off   byte offset of the window in `src` (HWC, rows of win_w * 3 bytes)   [1] win_w  [2] win_h
 *       [3] ksize_x   [4] ksize_y   [5] cx_off  [6] cy_off   offsets in `coefs` (ints) of the column / row tables; entry j of a table is
 *                     ksize + 2 ints: first tap (window column / scratch row), tap count, ksize 22-bit fixed-point coefficients
 *       [7] scr_w     resized columns computed (column table entries)   [8] scr_h  scratch rows: virtual rows [row0, row0 + scr_h)
 *       [9] row0      virtual row of scratch row 0, relative to the window's first row   [10] ny  resized rows (row table entries)
 *       [11] ox_off   [12] oy_off   output (x, y) + off = resized (column, row) index into the tables; x is read mirrored when flip
 *       [13..16]      pad_x0, pad_x1, pad_y0, pad_y1: outside the resized image but inside this box (same coordinates) -> 127, else 0
 *       [17] flip     [18], [19] must be 0
 *      desc_host is validated (MDCV_EARG) and sizes nothing else; desc is its device copy, which the kernels read and check again (an
 *      image whose device descriptor fails the checks is written as zeros).  Scratch: mdcv_imgload_workspace_bytes(B, max_scr_w, max_scr_h);
 *      every descriptor needs scr_w <= max_scr_w, scr_h <= max_scr_h.  C in {1, 3}. */
#define MDCV_IMGLOAD_DESC 20
long long mdcv_imgload_workspace_bytes(int B, int max_scr_w, int max_scr_h);
int mdcv_imgload_batch(const int* desc_host, const int* desc, int B, const int* coefs, long long n_coefs, const unsigned char* src,
                       long long src_bytes, int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace, float* out, void* stream);

/* ---- the same batches with the reference's training augmentation (csrc/imgaug.hip; datasets.py:226-242 over torchvision 0.3's ColorJitter
 *      and F.affine, which are Pillow's ImageEnhance blends, convert('HSV') / convert('RGB') and Image.transform(AFFINE, BILINEAR, fill 127)):
 *      patch -> jitter -> affine -> convert('L') when C == 1 -> hflip -> /255 into out [B,C,H,W] fp32; byte-exact against Pillow 12.2.
 *      desc_host / desc / coefs / src / workspace are mdcv_imgload_batch's.  One more descriptor of MDCV_IMGAUG_DESC ints per image:
 *       [0..11]   six doubles (low word first): Image.transform's AFFINE data, output pixel centre -> input position; read when [21] is 1
 *       [12] jitter   0 / 1
 *       [13..16]  the order of the four ops, a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue
 *       [17..19]  float32 bits of the brightness, contrast and saturation factors (Image.blend's alpha), each in [0, 16]
 *       [20] hue      the uint8 added to the H channel, 0..255
 *       [21] affine   0 / 1        [22], [23] must be 0
 *      An image with [12] == [21] == 0 comes out as mdcv_imgload_batch writes it.  aug_host is validated (MDCV_EARG); aug is its device
 *      copy, checked again by the kernels (an image whose device descriptors fail is written as zeros).  No entry of this descriptor
 *      indexes memory: every tap is clamped to the H x W patch.  aug_workspace: mdcv_imgaug_workspace_bytes(B, H, W) bytes (the uint8
 *      RGBX patches and one luma sum per image, which bounds H * W by 4096 * 4096).  Launches: horizontal pass, uint8 patch, the luma
 *      sums (only when some image's jitter is on), apply. */
#define MDCV_IMGAUG_DESC 24
long long mdcv_imgaug_workspace_bytes(int B, int H, int W);
int mdcv_imgload_aug_batch(const int* desc_host, const int* desc, const int* aug_host, const int* aug, int B, const int* coefs, long long n_coefs,
                           const unsigned char* src, long long src_bytes, int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace,
                           void* aug_workspace, float* out, void* stream);

/* ---- the same two batches with source windows referenced in place in a device-resident frame cache (mdcv/data/framecache.py).  Per image
 *      the horizontal pass reads EITHER its staged window in `src` (as above) OR a rectangle of a decoded frame kept in `pool`.  The choice
 *      is one row of MDCV_IMGLOAD_FREF long longs per image, beside the descriptors (fref_host / fref: host and device copy):
 *       [0] off     byte offset of the frame in `pool`, or -1: this image is staged and descriptor word [0] locates it (the other three
 *                   words are then not read)
 *       [1] pitch   bytes from one frame row to the next (3 * frame width; any value, no alignment is assumed)
 *       [2] x0  [3] y0   the window's origin in the frame:  pixel(wy, x) = pool[off + (y0 + wy) * pitch + 3 * (x0 + x)]
 *      A reference is good when off, x0, y0 >= 0, pitch >= 3 * (x0 + win_w) and off + (y0 + win_h - 1) * pitch + 3 * (x0 + win_w)
 *      <= pool_bytes (64-bit arithmetic; empty windows allowed).  A pooled image's descriptor word [0] is not read; everything else of
 *      the descriptor, the tables, the scratch and the launches are those of the staged entry points, and the bytes written are the same.
 *      fref_host is validated with desc_host (MDCV_EARG, nothing is enqueued); the kernels check the device copies again (an image that
 *      fails is written as zeros).  pool_bytes <= 2^60; pool may be NULL when pool_bytes is 0. */
#define MDCV_IMGLOAD_FREF 4
int mdcv_imgload_frames_batch(const int* desc_host, const int* desc, const long long* fref_host, const long long* fref, int B, const int* coefs,
                              long long n_coefs, const unsigned char* src, long long src_bytes, const unsigned char* pool, long long pool_bytes,
                              int max_scr_w, int max_scr_h, int C, int H, int W, void* workspace, float* out, void* stream);
int mdcv_imgload_aug_frames_batch(const int* desc_host, const int* desc, const long long* fref_host, const long long* fref, const int* aug_host,
                                  const int* aug, int B, const int* coefs, long long n_coefs, const unsigned char* src, long long src_bytes,
                                  const unsigned char* pool, long long pool_bytes, int max_scr_w, int max_scr_h, int C, int H, int W,
                                  void* workspace, void* aug_workspace, float* out, void* stream);

/* ---- the reference's four imgaug options on a finished detector batch (csrc/imgfx.hip; datasets.py:253-295: iaa.GaussianBlur,
 *      iaa.AdditiveGaussianNoise(per_channel=0.5), iaa.SigmoidContrast, iaa.Sharpen of imgaug 0.3.0; DESIGN §16.3 defines the arithmetic).
 *      src [B,3,H,W] fp32 holding u / 255 (what the entry points above write) -> dst, the same layout, out of place; one launch.  Per image
 *      the ops run on the bytes in the order blur, noise, contrast, sharpen, each behind its flag; an image with no flag set is copied
 *      bit for bit.  One descriptor of MDCV_IMGFX_DESC ints per image (mdcv/data/images.py writes them):
 *       [0] blur      0 / 1     [1] r  radius, 1..7     [2..9]  the half table q[0..7], centre first: q >= 0, q[k] == 0 for k > r,
 *                     q[0] + 2 * sum q[1..] == 256.  Separable, BORDER_REFLECT_101: t = sum q * src (unrounded), (sum q * t + 32768) >> 16
 *       [10] noise    0 / 1     [11] per_channel  0: one draw per pixel shared by the channels, 1: one per (y, x, c)
 *       [12] seed     32 bits   [13..14] scale, a double (low word first) in [0, 255].  Sample counter n = y * W + x, or 3 * n + c per
 *                     channel; S = the twelve 16-bit halves of the six hash words of (seed, n, j) summed; the byte gets
 *                     clip(rint(scale * (S - 393210) / 65536), -255, 255) added and is clipped to 0..255
 *       [15] contrast 0 / 1     [16] table  index into `luts` (n_luts tables of 256 bytes, computed on the host), < n_luts
 *       [17] sharpen  0 / 1     [18] kc  [19] kn  float32 bits of the centre and neighbour coefficients, kc in [0, 16], |kn| <= 2:
 *                     rint((double)kc * centre + (double)kn * (sum of the 8 neighbours)) clipped to 0..255, BORDER_REFLECT_101
 *       [20..23] must be 0
 *      Every field is checked whether or not its flag is set, the table index only when [15] is.  fx_host is validated (MDCV_EARG, nothing
 *      is enqueued); fx is its device copy, checked again by the kernel (an image whose device descriptor fails is written as zeros).
 *      MDCV_EARG also for: C != 3, H or W < 16, H * W > 4096 * 4096, B outside 1..65535, dst overlapping src.  No scratch. */
#define MDCV_IMGFX_DESC 24
int mdcv_imgfx_batch(const int* fx_host, const int* fx, int B, const unsigned char* luts, int n_luts, int C, int H, int W, const float* src,
                     float* dst, void* stream);

/* ---- real key-point crop batches (csrc/kptload.hip; RektNet/dataset.py:34-56 ConeDataset.__getitem__ over RektNet/utils.py:73-96):
 *      B decoded crops (uint8, HWC, RGB, any height and width, packed back to back in `src` at unaligned byte offsets) ->
 *       images   [B,3,S,S] fp32: cv2.resize of the 8-bit crop to S x S with mdcv_crop_resize_u8's rule, then (float)(u8 / 255.0); the
 *                planes are B, G, R (cv2.imread's order, which the reference keeps)
 *       heatmaps [B,7,S,S] fp32: prep_label in float64 as mdcv_synth_crop_batch computes it (one-hot at the hot pixel of the original
 *                crop -> INTER_LINEAR resize -> [1,4,6,4,1]/16 blur with BORDER_REFLECT_101 -> divided by sum_y * sum_x); a map whose
 *                down-scaled one-hot misses every tap is all NaN (0 / 0), as in the reference
 *      One descriptor of MDCV_KPTLOAD_DESC ints per crop (mdcv/data/crops.py writes them):
 *       [0] src_off  byte offset of the crop in `src` (rows of w * 3 bytes)   [1] h   [2] w   [3] must be 0
 *       [4 + 2k], [5 + 2k]  the hot pixel (int(x), int(y)) of key point k = 0..6, inside the crop   [18], [19] must be 0
 *      Bounds, checked before the launch (MDCV_EARG, nothing is enqueued): MDCV_KPTLOAD_MIN_SIZE <= S <= MDCV_KPTLOAD_MAX_SIZE,
 *      1 <= h, w <= MDCV_KPTLOAD_MAX_SIDE, every crop inside src_bytes <= 2^31 - 1, 1 <= B <= 65535.  desc_host is what is validated;
 *      desc is its device copy, whose crop extents the kernel checks again (a crop that fails is written as zeros).  One launch. */
#define MDCV_KPTLOAD_DESC 20
#define MDCV_KPTLOAD_MIN_SIZE 16
#define MDCV_KPTLOAD_MAX_SIZE 256
#define MDCV_KPTLOAD_MAX_SIDE 4096
int mdcv_kptload_batch(const int* desc_host, const int* desc, int B, const unsigned char* src, long long src_bytes, int S, float* images,
                       float* heatmaps, void* stream);

/* ---- detections drawn into the frames on the device (csrc/detect_draw.hip; the tail of single_img_detect, CVC-YOLOv3/detect.py:99-104:
 *      four .item() reads and one ImageDraw.rectangle(outline="red") per box on the host).  ONE launch per batch, grid (K, B); slot k of frame b
 *      does nothing unless k < count[b] (a device int, as mdcv_detect_post writes it), so the host never reads the counts.  Per kept box:
 *       frame_boxes [B,K,4] double   (double)boxes[b,k,j] / ratio - pad (pad_w for x, pad_h for y) in IEEE double: Python's `x.item() / ratio - pad_w`
 *       rects       [B,K,4] int32    (int) of those doubles (toward zero: -0.9 -> 0, -1.5 -> -1), or (0, 0, -1, -1) for a box that is NOT
 *                                    drawn: x1 < x0 or y1 < y0 compared as doubles (where Pillow raises), or any coordinate NaN, +-inf or of
 *                                    magnitude >= 2^30 (where C's conversion is undefined); skipped[b] counts them (a departure: the
 *                                    reference's behaviour there is an exception or undefined)
 *       pool                         the outline, as Pillow 12.2's ImagingDrawRectangle draws it for width 1 without fill: rows y0 and y1 from x0
 *                                    to x1 inclusive, columns x0 and x1 over every row between y0 + 1 and y1 inclusive in either order (so with
 *                                    y1 == y0 row y0 + 1 gets the two end pixels), clipped to the frame; bytes (red, green, blue), the same for
 *                                    every box of the call -- overlapping boxes store identical bytes and no order between them matters
 *      boxes [B,K,4] fp32 corner boxes in detector coordinates (mdcv_detect_post's out_boxes with K = top_k).  Frames are uint8 HWC RGB with rows
 *      of 3 * W bytes in `pool`, the layout mdcv_imgload_frames_batch reads.  One descriptor of MDCV_DETECT_DESC long longs per frame:
 *       [0] off   byte offset of the frame in `pool`   [1] W   [2] H   [3] the bits of the double `ratio`   [4] pad_w   [5] pad_h
 *      (ratio and the pads: calculate_padding's, mdcv/data/images.py letterbox()).  A descriptor is good when off >= 0, 1 <= W, H <= 2^24,
 *      off + 3 W H <= pool_bytes, |pad| <= 2^24 and 0 < ratio < 2^30.  desc_host is validated (MDCV_EARG, nothing is enqueued); desc is its
 *      device copy, whose frame extents the kernel checks again (a frame that fails is not drawn on).  skipped [B] is zeroed by the call (a
 *      memset on `stream` in front of the launch).  Slots k >= count[b] of frame_boxes / rects are not written.  B == 0 or K == 0: MDCV_OK,
 *      nothing is enqueued or written.  B, K <= 65535.  No state is kept between calls. */
#define MDCV_DETECT_DESC 6
int mdcv_detect_draw_boxes(const long long* desc_host, const long long* desc, int B, const float* boxes, const int* count, int K,
                           unsigned char* pool, long long pool_bytes, int red, int green, int blue, double* frame_boxes, int* rects,
                           int* skipped, void* stream);

/* The same call without the outline: steps a to c only, through the same kernel, so frame_boxes, rects and skipped hold the same bytes as
 * mdcv_detect_draw_boxes writes for the same arguments, and no byte of any pool is read or written (only pool_bytes is taken, for the same
 * descriptor checks).  The cone pipeline maps first, cuts its crops out of the untouched frames (mdcv_crop_resize_frames_u8), and calls
 * mdcv_detect_draw_boxes afterwards. */
int mdcv_detect_map_boxes(const long long* desc_host, const long long* desc, int B, const float* boxes, const int* count, int K,
                          long long pool_bytes, double* frame_boxes, int* rects, int* skipped, void* stream);

/* ---- tile-and-scale inference, the join (csrc/detect_tiles.hip; mdcv/yolo/detect.py TiledFrameDetector).  Training cuts every scaled frame
 *      into network-sized tiles (ts=True); inference on the same tiles yields, per frame, T tiles x K boxes in TILE coordinates.  This call
 *      makes them one list per frame in scaled-frame coordinates and removes the duplicates of overlapping tiles.  The reference has no tiled
 *      inference: the scan is its utils/nms.py:31-61 with the fp32 arithmetic of mdcv_nms / mdcv_detect_post (one shared device function), the
 *      seam rule below is a departure.  ONE launch per batch of frames, one workgroup per frame, no workspace, no state between calls; the
 *      counts are read on the device only.
 *      tile_boxes [T,K,4] fp32, tile_prob [T,K] fp32, tile_count [T] int32: device arrays as mdcv_detect_post writes out_boxes, out_prob and
 *      out_count for T tiles with K = its top_k (a count is clamped to 0..K).  Tile table: MDCV_TILE_DESC int32 words per tile,
 *       [0] frame index in 0..B-1   [1] off_x   [2] off_y   [3] 0
 *      the tiles of one frame contiguous, frames ascending (a frame may have none: count 0).  tiles_host is validated (MDCV_EARG, nothing is
 *      enqueued); tiles is its device copy, which the kernel checks again per frame (a frame whose tiles fail gets count 0).
 *      Per frame b:  candidates (t, k), k < tile_count[t], corner j = (float)((double)tile_boxes[t,k,j] + (double)off) (off_x for j = 0, 2, off_y
 *      for j = 1, 3: one rounding), score tile_prob[t,k].  Visiting order: descending score, equal scores by ascending tile index, then
 *      ascending slot; only the first top_k candidates in that order are considered (nms.py:26).  Greedy scan: a remaining candidate j stays
 *      behind a kept i iff IoU <= overlap (a NaN leaves) and, when contain_thres >= 0 and j and i come from different tiles, also
 *      inter / min(area_j, area_i) <= contain_thres -- the seam rule: it removes the part of a cone that a tile edge cut off when the
 *      neighbouring tile holds the whole cone, which plain IoU cannot.  A negative contain_thres turns it off.
 *      out_boxes [B,top_k,4] fp32, out_prob [B,top_k] fp32, out_src [B,top_k,2] int32 = (tile index in the batch, slot in the tile),
 *      out_count [B] int32: kept boxes in visiting order; slots past out_count[b] hold zeros, their out_src (-1, -1).
 *      Limits (beyond them MDCV_EARG): at most MDCV_TILE_MAX_PER_FRAME tiles per frame, K and top_k <= MDCV_NMS_MAX_TOPK (so at most 32768
 *      candidates per frame), 1 <= top_k, |off| <= MDCV_TILE_MAX_OFFSET, B <= 65535.  B == 0, T == 0 or K == 0: MDCV_OK, nothing is enqueued
 *      or written. */
#define MDCV_TILE_DESC 4
#define MDCV_TILE_MAX_PER_FRAME 64
#define MDCV_TILE_MAX_OFFSET 16777216
int mdcv_detect_merge_tiles(const float* tile_boxes, const float* tile_prob, const int* tile_count, const int* tiles_host, const int* tiles,
                            int T, int K, int B, float overlap, float contain_thres, int top_k, float* out_boxes, float* out_prob,
                            int* out_src, int* out_count, void* stream);

/* ---- cone key points on whole frames, drawn on the device (csrc/kpt_detect.hip; RektNet/detect.py and RektNet/utils.py:61-66 for every
 *      cone of every frame of a batch).  Frames and descriptors are mdcv_detect_draw_boxes': uint8 HWC RGB, rows of 3 * W bytes, at any
 *      byte offset in `pool`; of a descriptor these calls read off, W, H (and test the pads' range), not the ratio.  desc_host is validated
 *      (MDCV_EARG, nothing is enqueued); desc is its device copy, which the kernels check again.  One launch each; no state is kept.
 *
 *      mdcv_crop_resize_frames_u8: rects [B,K,4] int32 (x0, y0, x1, y1 as mdcv_detect_draw_boxes writes them) and count [B] are device
 *      arrays the host never reads.  Slot k of frame b is looked at when k < min(count[b], K, max_per_frame).  Its window is the rect
 *      clipped to the frame, both ends inclusive: cx0 = max(x0, 0), cx1 = min(x1, W - 1), cy0 = max(y0, 0), cy1 = min(y1, H - 1).  A box HAS
 *      A CROP unless the window is empty (cx1 < cx0 or cy1 < cy0: the skipped rect (0, 0, -1, -1) among them), a side is above
 *      MDCV_KPTLOAD_MAX_SIDE, or the frame's device descriptor fails its check.  The boxes with a crop are numbered m = 0, 1, ... in
 *      (frame, slot) order by an exclusive prefix computed on the device, and for each:
 *       crops  [m,3,S,S] fp32   mdcv_kptload_batch's image rule applied to the window's pixels read in place: cv2's 8-bit INTER_LINEAR to
 *                               S x S, then (float)(u8 / 255.0); planes B, G, R (the pool is RGB: plane p is byte 2 - p of a pixel)
 *       owner  [m,2]   int32    (b, k)
 *       window [m,4]   int32    (cx0, cy0, w, h)
 *      and total [1] int32 = their number.  crops / owner / window hold B * min(K, max_per_frame) rows; rows at total and beyond are not
 *      written.  MDCV_KPTLOAD_MIN_SIZE <= S <= MDCV_KPTLOAD_MAX_SIZE, 1 <= B, K <= 65535, max_per_frame >= 1,
 *      B * min(K, max_per_frame) <= 2^20, 1 <= pool_bytes <= 2^60, no null pointer.
 *
 *      mdcv_kpt_draw_points: pts [M,7,2] fp32 (x, y normalised in the window), window [M,4] and owner [M,2] as above (of owner only the
 *      image index is read), all on the device; colours: 7 x 3 bytes ON THE HOST, (R, G, B) of key point 0..6, copied into the launch.
 *       centers [M,7,2] int32   (wx0 + (int)((double)pt_x * w), wy0 + (int)((double)pt_y * h)): the product in IEEE double, truncated
 *                               toward zero (what `int(pt[0] * w)` gave under NumPy 1.x, where float32 * int is a float64).  A point that
 *                               is NaN or infinite or whose product has magnitude >= 2^30 is not drawn, gets (-1, -1), and skipped[image]
 *                               counts it; so do all 7 points of a cone whose image index is outside [0, n_images) (not counted), whose
 *                               image's device descriptor fails, or whose window does not lie inside its image (x0, y0 >= 0, w, h >= 1,
 *                               x0 + w <= W, y0 + h <= H)
 *       pool                    each drawn point as cv2.circle(img, c, 2, colour, -1) (LINE_8, shift 0): the 13 pixels |dx| + |dy| <= 2
 *                               around the centre, clipped to the IMAGE (not the window).  Overlapping discs: a pixel holds the colour of
 *                               the LAST point covering it in (row m, key point) order among the cones of its image, as after the
 *                               reference's sequential loop, under any schedule; no other byte of the pool is written.
 *      Rows of one image must be contiguous in owner (image-major, as mdcv_crop_resize_frames_u8 writes them): cones of one image in two
 *      separate runs are ordered only inside each run.  skipped [n_images] is zeroed by the call (a memset on `stream`).  M == 0: only
 *      that memset.  1 <= n_images <= 65535, 0 <= M <= 2^20.
 *
 *      mdcv_kpt_heatmap_mosaic: hm [B,7,S,S] fp32 -> out [B,7*S,S] uint8, the `_hm` picture of RektNet/detect.py:40-48.  Per map:
 *      cmin, cmax of the map; v = (x - cmin) / (cmax - cmin), each a correctly rounded float32 operation; out = rint((double)v * 255.0),
 *      ties to even, saturated to 0..255 (cv2.imwrite's convertTo(CV_8U) of the float64 array), NaN -> 0.  A constant map, and a map
 *      holding a NaN, give zeros (a departure: the reference divides by zero).  0 <= B <= 65535, 1 <= S <= 4096. */
int mdcv_crop_resize_frames_u8(const long long* desc_host, const long long* desc, int B, const unsigned char* pool, long long pool_bytes,
                               const int* rects, const int* count, int K, int max_per_frame, int S, float* crops, int* owner, int* window,
                               int* total, void* stream);
int mdcv_kpt_draw_points(const long long* desc_host, const long long* desc, int n_images, unsigned char* pool, long long pool_bytes,
                         const float* pts, const int* window, const int* owner, int M, const unsigned char* colours, int* centers,
                         int* skipped, void* stream);
int mdcv_kpt_heatmap_mosaic(const float* hm, int B, int S, unsigned char* out, void* stream);

/* ---- optimizer step over the flat fp32 parameter buffer (train.py:180-187,72 ; train_eval.py:263,72) */
int mdcv_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, int step, float lr, float beta1,
                   float beta2, float eps, float weight_decay, float grad_scale, void* stream);
int mdcv_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, int step, float lr, float momentum, float weight_decay,
                  float grad_scale, void* stream);

/* ---- gradient guard (csrc/grad_guard.hip): global-norm clipping and dropping a step whose gradient is not finite, decided
 *      on the device.  Four enqueue-only entry points on the caller's stream; no process state; nothing here waits for the GPU.
 *
 *      mdcv_grad_sumsq: partials[c] = the sum of (double)g[i] * (double)g[i] over chunk c = elements [c * CHUNK, min(n, (c + 1) * CHUNK)),
 *      CHUNK = MDCV_GRAD_GUARD_CHUNK, for c < ceil(n / CHUNK).  Order inside a chunk: thread t of 256 adds
 *      elements (r * 256 + t) * 4 + e for r = 0..3, e = 0..3 (elements beyond n add +0.0); the 256 sums are joined by the xor butterfly
 *      of each wave (offsets 32, 16, .. 1) and then ((w0 + w1) + w2) + w3.  The order is a function of n alone: the grid (capped at
 *      MDCV_GRAD_GUARD_MAX_GRID workgroups, which stride over the chunks) and the order in which workgroups run do not enter, and no
 *      atomics are used.  grads 16-byte aligned, n >= 1; partials is caller-owned scratch, every word of it is written.
 *
 *      mdcv_grad_guard_finalize: one workgroup.  Thread t adds partials t, t + 256, .. in order, the 256 sums are joined as above, and
 *      the block is written (ordinary stores):
 *        sumsq                  the sum; finite exactly when every gradient is
 *        norm                   (float)(fabs((double)grad_scale) * sqrt(sumsq))
 *        coef                   max_norm > 0: fminf(1, max_norm / (norm + 1e-6f)) -- torch.nn.utils.clip_grad_norm_; otherwise 1
 *        scale                  grad_scale * coef: what the guarded updates multiply every gradient by
 *        finite, apply          apply = finite || !skip_nonfinite
 *        attempted, applied, skipped, clipped   counters; clipped counts applied steps with a finite norm and coef < 1
 *        max_norm_seen          the largest finite norm so far
 *        bc1, bc2_sqrt          (float)(1 - beta1^t), (float)sqrt(1 - beta2^t) in double with t = applied + 1 (the count BEFORE this
 *                               call): a skipped step leaves no trace in the bias correction.  beta^t is square-and-multiply from the
 *                               low bit of t up (r = r * x on a set bit, then x = x * x while bits remain).  SGD passes 0 for both.
 *      and history[attempted % ring] = norm (attempted BEFORE this call; ring == 0: no history).  The caller zeroes the block once.
 *
 *      mdcv_adam_step_guarded / mdcv_sgd_step_guarded: mdcv_adam_step / mdcv_sgd_step with grad_scale = block->scale, the bias
 *      corrections from the block and "first step" = block->applied == 1 (this step is the first one applied); block->apply == 0: every
 *      thread returns before it reads or writes params, grads or state.  Any 16-byte aligned slice may be passed, as to mdcv_adam_step.
 *      These round every operation on its own (no fma contraction), so they differ from the unguarded kernels in the last bit. */
#define MDCV_GRAD_GUARD_CHUNK 4096
#define MDCV_GRAD_GUARD_MAX_GRID 2048
typedef struct mdcv_grad_guard_block {
  double sumsq;                                   /* byte  0 */
  float norm, coef, scale, bc1, bc2_sqrt;         /* bytes 8, 12, 16, 20, 24 */
  float max_norm_seen;                            /* byte 28 */
  int finite, apply;                              /* bytes 32, 36 */
  long long attempted, applied, skipped, clipped; /* bytes 40, 48, 56, 64; 72 bytes in all */
} mdcv_grad_guard_block;
int mdcv_grad_sumsq(const float* grads, long long n, double* partials, void* stream);
int mdcv_grad_guard_finalize(const double* partials, long long n_partials, float grad_scale, float max_norm, int skip_nonfinite, double beta1,
                             double beta2, mdcv_grad_guard_block* block, float* history, int ring, void* stream);
int mdcv_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, const mdcv_grad_guard_block* block,
                           float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);
int mdcv_sgd_step_guarded(float* params, const float* grads, float* momentum_buf, long long n, const mdcv_grad_guard_block* block, float lr,
                          float momentum, float weight_decay, void* stream);

/* ---- weight EMA (csrc/weight_ema.hip): an exponential moving average of the flat fp32 parameter buffer and of the BatchNorm
 *      running statistics, kept in ONE shadow buffer.  Five enqueue-only entry points on the caller's stream; no process state; nothing
 *      here waits for the GPU.  The state is the control block below (the caller zeroes it once).
 *
 *      mdcv_ema_advance: one thread.  apply = guard ? guard->apply : 1 (a NULL guard applies).  apply != 0: with t = block->updates,
 *        d64 = min((double)decay, (1.0 + (double)t) / ((double)warmup + (double)t)) in double, d = (float)d64, omd = 1.0f - d;
 *        block->d = d, block->omd = omd, block->apply = 1, block->updates = t + 1.  apply == 0: block->apply = 0, nothing else is
 *        written.  0 <= decay < 1, warmup >= 1 (warmup == 1: d == decay from the first update).  No transcendental.
 *
 *      mdcv_ema_update: ema[i] = ema[i] + omd * (params[i] - ema[i]) for i < n: a subtraction, a product and a sum, each rounded to
 *        fp32 on its own.  omd and apply are read from the block; block->apply == 0: every thread returns before it reads or writes
 *        ema or params.  Any 16-byte aligned slice of the two buffers may be passed (as to mdcv_adam_step); any n >= 0.  params is read
 *        with non-temporal loads: inside a training step this pass is its last reader.
 *      mdcv_ema_update_segments: the same arithmetic, in ONE launch, over the rows of a device table: row r updates
 *        ema[offset .. offset + length) from src[0 .. length).  src is any 4-byte aligned address; offset and length count elements.
 *        A row that does not lie inside ema[0 .. ema_elems), or whose src is NULL, is left alone (checked on the device: the table lives there).
 *
 *      mdcv_ema_swap / mdcv_ema_swap_segments: exchange the 32-bit words of the two sides (no arithmetic: NaN payloads, signed zeros
 *        and denormals pass unchanged), so that two calls restore every bit.  They read no block.
 *
 *      One grid pass of mdcv_ema_update / mdcv_ema_swap covers MDCV_EMA_MAX_GRID * MDCV_EMA_THREADS * 4 elements; longer ranges are
 *      strided over. */
#define MDCV_EMA_THREADS 256
#define MDCV_EMA_MAX_GRID 2048
typedef struct mdcv_ema_block {
  long long updates;                              /* byte  0: updates applied so far */
  float d, omd;                                   /* bytes 8, 12: the decay of the latest applied update and 1 - d */
  int apply, reserved;                            /* bytes 16, 20; 24 bytes in all */
} mdcv_ema_block;
typedef struct mdcv_ema_segment {
  const float* src;                               /* byte  0: the live tensor */
  long long offset, length;                       /* bytes 8, 16: its place in the shadow buffer, in elements; 24 bytes in all */
} mdcv_ema_segment;
int mdcv_ema_advance(mdcv_ema_block* block, const mdcv_grad_guard_block* guard, float decay, long long warmup, void* stream);
int mdcv_ema_update(float* ema, const float* params, long long n, const mdcv_ema_block* block, void* stream);
int mdcv_ema_update_segments(float* ema, long long ema_elems, const mdcv_ema_segment* table, int n_segments, const mdcv_ema_block* block,
                             void* stream);
int mdcv_ema_swap(float* ema, float* params, long long n, void* stream);
int mdcv_ema_swap_segments(float* ema, long long ema_elems, const mdcv_ema_segment* table, int n_segments, void* stream);

/* ---- per-step bookkeeping of the training loops in one launch (csrc/train_log.hip; CVC-YOLOv3/train.py:54,63-64,74-90 ;
 *      RektNet/train_eval.py:74-78): what the loops read back with `.item()` every step stays on the device.
 *      losses: n_losses addresses ON THE HOST (copied into the launch), each a device pointer to ONE fp32 or NULL (= 0.0f: RektNet's
 *      geometric loss without include_geo); 1 <= n_losses <= MDCV_TRAIN_LOG_MAX_LOSSES.
 *      targets [B,T,5] fp32 on the device, read only if with_targets != 0.
 *       count                   the number of (b, t) with MORE THAN ONE of targets[b,t,1:5] > 0 (train.py:63; NaN > 0 is false);
 *                               0 if with_targets == 0 or B * T == 0
 *       row [MDCV_TRAIN_LOG_ROW] fp32   loss_0 .. loss_{n-1}, (float)count, zeros to the end; every word of the row is written
 *       acc [n_losses + 1] fp64         acc[j] += (double)loss_j for j < n_losses, then acc[n_losses] += (double)count + 1e-12: IEEE
 *                               double additions by ONE thread, one launch after the other on the stream -- the sums Python's
 *                               `epoch_losses[j] += loss.item()` and `epoch_num_targets += count + 1e-12` hold, bit for bit.  The caller
 *                               starts acc[j] at 0.0 and acc[n_losses] at 1e-12 (train.py:54).
 *      One workgroup: a strided pass over the B * T targets, an integer reduction (exact in any order), then the additions above.  Nothing
 *      outside row[0 .. MDCV_TRAIN_LOG_ROW) and acc[0 .. n_losses] is written.  MDCV_EARG before any launch: losses, acc or row NULL, n_losses
 *      out of range, B < 0, T < 0, B * T > INT_MAX, or with_targets != 0 and B * T > 0 and targets NULL. */
#define MDCV_TRAIN_LOG_MAX_LOSSES 8
#define MDCV_TRAIN_LOG_ROW 12
int mdcv_train_log_step(const float* const* losses, int n_losses, const float* targets, int with_targets, int B, int T, double* acc,
                        float* row, void* stream);

/* ---- runtime plumbing: device query, HIP events on a caller stream, hipGraph capture of a launch sequence */
int mdcv_device_info(int* cu_count, int* wave_size, long long* hbm_bytes, char* arch, int arch_len);
int mdcv_event_create(void** ev);
int mdcv_event_record(void* ev, void* stream);
int mdcv_event_sync(void* ev);
int mdcv_event_elapsed_ms(void* start, void* stop, float* ms);
int mdcv_event_destroy(void* ev);
/* everything enqueued on `from` so far happens before what is enqueued on `to` afterwards (one event record + one stream wait on a
 * ring event without timing; device_scope != 0: the record releases to device scope, all a consumer on the same GPU needs) */
/* On-box peak probe: `blocks` workgroups x 4 waves x iters x 8 independent v_mfma_f32_16x16x32_bf16 on register operands; *flops = the FLOP
 * count of the launch.  Time it with events on `stream`: the dense bf16 MFMA rate this box sustains (spec: ~2.5 PFLOP/s).  sink: >= 1 float. */
int mdcv_probe_mfma(int blocks, int iters, float* sink, double* flops, void* stream);
int mdcv_stream_fork(void* from, void* to, int device_scope);
/* the same ordering without a marker packet in the producer's queue: the next kernel this library launches (exactly one, on `from`) carries
 * the event as its dispatch packet's stop event; mdcv_stream_fork_wait(to, ev) then makes `to` wait for it */
int mdcv_stream_fork_arm(void* from, int device_scope, void** ev_out);
int mdcv_stream_fork_wait(void* to, void* ev);
/* In-library kernel profiler: between _begin and _stop EVERY kernel this library launches carries a start / stop HIP event pair bound
 * to its own dispatch on the stream it is launched on (hipExtLaunchKernel: no extra packets, the durations are the kernel's own).  _count = launches recorded so far (lets a host attribute them to its own calls); _stop ends recording,
 * waits for the events and returns the record count; _read(i) -> duration in ms and the kernel symbol as rocprofv3 prints it.
 * (bench.py's `roofline` / `roofline_kernels`; not meant for timed regions: each record costs two event records.) */
int mdcv_profile_begin(void);
int mdcv_profile_count(void);
int mdcv_profile_stop(void);
int mdcv_profile_read(int i, float* ms, char* name, int name_len);
int mdcv_graph_begin(void* stream);
int mdcv_graph_end(void* stream, void** graph_exec);
int mdcv_graph_launch(void* graph_exec, void* stream);
int mdcv_graph_destroy(void* graph_exec);

/* ---- 1x1 convolution blocks with the neighbouring BatchNorm pass folded into the operand load (csrc/pw_block.hip; bf16 only).
 *      Replaces, for a 1x1 conv whose input is the output of a conv -> BatchNorm -> activation (-> shortcut add) block
 *      (CVC-YOLOv3/models.py:48-72 + the shortcut of :322-327), the pair  mdcv_bn_act_fwd + mdcv_conv2d  by one launch with identical results.
 *      K = channels of the transformed operand (multiple of 32, K/8 divides 256, 64 <= K <= 1024), N = output channels (multiple of 8). */
int mdcv_pw_rows(long long M, int K);          /* rows of stats_partial the entry points below write: one per pixel tile */
/* forward: z = act(y * scale + shift) (+ resid) -> z_out ; out = z . W^T (+ bias) ; stats_partial (may be NULL): [mdcv_pw_rows][2][N] */
int mdcv_pw_conv_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift, const void* resid, int ldr, int act,
                     float slope, void* z_out, int ldz, const void* w_packed, const float* bias, void* out, int out_ldc,
                     float* stats_partial, long long M, int K, int N, void* stream);

/* ---- backward of a pointwise (1x1, stride 1) nn.Conv2d in ONE launch (CVC-YOLOv3/models.py:59-65, the 34 1x1 layers of yolo_baseline):
 * dx = dy . W (+ addsrc) [M x Cin] AND the fp32 slab partials of dW = dy^T . x (ws[slabs][Cout][Cin]; one slab per run of pixels, summed in
 * fixed order by mdcv_wgrad_reduce: bit-reproducible), a workgroup holding each dy / x pixel tile in LDS once for both products.  fy != NULL:
 * also the BatchNorm-backward partial sums of the layer that produced this conv's input, [slabs][2][Cin] (as mdcv_conv2d_dgrad_bnsums).
 * bf16 only; Cout (channels of dy, padded) in {64, 128, 256, 512}, Cin a multiple of 64.  mdcv_pw_bwd_slabs returns 0 for layers that do not
 * take this form (then: mdcv_conv2d mode 1 + mdcv_conv2d_wgrad). */
int mdcv_pw_bwd_slabs(int dtype, long long M, int Cin, int Cout, int ldy, int ldx, int lddx, int ldadd, int ldfy);
int mdcv_pw_bwd(int dtype, const void* dy, int ldy, const void* x, int ldx, const void* wd_packed, void* dx, int lddx, const void* addsrc,
                int ldadd, float* ws, int slabs, const void* fy, int ldfy, const float* fscale, const float* fshift, const float* fmean, int fact,
                float fslope, float* fpartial, long long M, int Cin, int Cout, void* stream);
/* Weight gradient of a conv -> BatchNorm -> activation layer whose INPUT needs no gradient (a network's first conv, CVC-YOLOv3/models.py:57-71 at
 * index 0), straight from dz (gradient of the activation output) and y (raw conv output): dy = cA*g + cB*y + cC, g = dz * act'(scale*y + shift) is formed
 * in the kernel's operand load, rounded to bf16 as mdcv_bn_act_bwd_apply rounds it -- bit-identical to apply + mdcv_conv2d_wgrad, without the apply
 * pass over the layer's output tensor.  _ok() = 1 where the geometry takes this form (bf16, Cout_pad <= 32); splits: any count
 * mdcv_conv2d_wgrad_splits_geom returns for the geometry -- the plans ask it with MDCV_TUNED(dtype, 20768), a target of three blocks per CU. */
int mdcv_conv2d_wgrad_bnapply_ok(int dtype, int B, int Hin, int Win, int Cin, int Hout, int Wout, int Cout, int KH, int KW, int stride,
                                 int pad, int dil, int dz_ldc, int y_ldc, int x_ldc);
int mdcv_conv2d_wgrad_bnapply(int dtype, const void* dz, int dz_ldc, const void* y, int y_ldc, const float* scale, const float* shift,
                              const float* cA, const float* cB, const float* cC, int act, float slope, const void* x, int x_ldc, float* ws,
                              int splits, float* dw_oihw, int accumulate, int B, int Hin, int Win, int Cin, int Cin_real, int Hout, int Wout,
                              int Cout, int Cout_real, int KH, int KW, int stride, int pad, int dil, void* stream);
/* sum of fp32 weight-gradient slabs ws[splits][Cout_pad][KK * Cin_pad] into the OIHW gradient [Cout][Cin][KK] (fixed split order) */
int mdcv_wgrad_reduce(const float* ws, int splits, float* dw_oihw, int accumulate, int Cout_pad, int Cout, int Cin_pad, int Cin, int KK,
                      void* stream);

/* ---- the one exchange step of the data-parallel path, for hosts that do not go through torch.distributed:
 *      nn.DataParallel's gradient reduction (CVC-YOLOv3/train.py:193-195 with `losses[0].sum().backward()`, train.py:70) as an RCCL
 *      all-reduce(SUM) of the flat fp32 gradient buffer over xGMI, one process per GPU.  librccl is bound at run time (dlopen by
 *      soname, sharing the instance a host such as torch already loaded); -2 = librccl not found.  Return values > 0 are ncclResult_t.
 *      id128: 128-byte ncclUniqueId made by rank 0 (mdcv_comm_unique_id) and handed to every rank by the host (file, socket, MPI...). */
int mdcv_comm_unique_id(void* id128);
int mdcv_comm_init(void** comm, int nranks, const void* id128, int rank);     /* on the calling thread's current HIP device */
int mdcv_comm_allreduce_sum(void* comm, float* buf, long long n, void* stream);   /* in place, enqueue-only */
int mdcv_comm_destroy(void* comm);

/* ---- anchor k-means of dataset preparation (CVC-YOLOv3/generate_kmeans_dataset_csvs.py:16-28 `assignment` / `update`, the loop of main at
 *      139-149): batched Lloyd iterations over N boxes points[N][2] = (h, w) in fp64, K clusters, R independent restarts, bit-reproducible.
 *      Limits: 1 <= K <= 16, 1 <= R <= 64, 1 <= N < 2^24; every coordinate finite, |x| < 2^14 and a multiple of 2^-64 (the CALLER checks the
 *      coordinates: they are device data).  Arithmetic: assignment, for k in index order, q = fl(fl(dh*dh) + fl(dw*dw)), d = sqrt(q) correctly
 *      rounded, the first minimum wins and a NaN centroid never wins; update c[k] = fl(S_k / n_k) per coordinate with S_k the EXACT sum of the
 *      members rounded once to nearest-even (math.fsum), NaN for an empty cluster.  The sums are integers (fixed point, quantum 2^-64, integer
 *      atomics): independent of the order blocks land in, so an unchanged assignment reproduces the same centroids and steps after a restart's
 *      fixed point are no-ops.
 *      Step 0 assigns to the initial centroids (the boxes init[R][K], indices into points); step t >= 1 updates from step t-1's assignment and
 *      assigns again.  mdcv_kmeans_begin clears the workspace (ws: mdcv_kmeans_workspace_bytes, 8-byte aligned) and gathers the initial
 *      centroids.  mdcv_kmeans_steps enqueues steps t0 .. t0+n_steps-1 (one launch each; the caller continues a run with t0 = the steps done so
 *      far) and one small launch that writes record[R][MDCV_KMEANS_REC_HEAD + 2K], 8-byte words per restart: converged_at (the first step whose
 *      assignment equals the previous step's, -1 = not yet), the low and high word of the distortion D = high * 2^32 + low =
 *      sum_i floor(q_i * 2^32) of the last step, 1 if a centroid is NaN, then the centroids after the last step's update, [K][2] fp64 bits.
 *      assign[R][N] holds the last step's assignment (state between calls). */
#define MDCV_KMEANS_MAX_K 16
#define MDCV_KMEANS_MAX_R 64
#define MDCV_KMEANS_REC_HEAD 4
long long mdcv_kmeans_workspace_bytes(long long N, int K, int R);     /* MDCV_EARG outside the limits */
int mdcv_kmeans_begin(void* ws, const double* points, const int* init, long long N, int K, int R, void* stream);
int mdcv_kmeans_steps(void* ws, const double* points, unsigned char* assign, long long* record, long long N, int K, int R, int t0,
                      int n_steps, void* stream);

/* ---- dataset-level detection evaluation: COCO-style average precision over a whole validation set, csrc/detmap.hip.
 *      The caller owns the dataset buffers, sized for `cap` images of K rows: score f32 [cap,K], cls i32 [cap,K], count i32 [cap],
 *      status u32 [S,cap,K] (two bits per IoU threshold j at bit 2j: MDCV_DETMAP_FP / _TP / _IGNORED) and n_gt i64 [S,C], which the caller
 *      zeroes before the first image.  Both calls are enqueue-only; every argument is checked before a device is touched (MDCV_EARG).
 *      Limits: 1 <= K <= MDCV_NMS_MAX_TOPK, 0 <= T <= MDCV_DETMAP_MAX_GT, 1 <= J <= MDCV_DETMAP_MAX_THR thresholds in (0, 1],
 *      1 <= S <= MDCV_DETMAP_MAX_RANGES ranges [lo, hi) of box area in px^2 with lo <= hi, 1 <= C <= MDCV_DETMAP_MAX_CLASSES,
 *      cap * K <= MDCV_DETMAP_MAX_SLOTS, 0 <= first and first + B <= cap, B <= 65535.
 *      mdcv_detmap_match: images first .. first+B-1 of the dataset.  Detections boxes [B,K,4] corner fp32, prob [B,K], cls [B,K] (NULL: class
 *      0), count [B] (clamped to 0..K), rows most confident first (they are not sorted again).  Ground truth, gt_mode MDCV_DETMAP_GT_PIXELS:
 *      gt [B,T,4] corner pixels, gt_cls [B,T] (NULL: 0), gt_ignore u8 [B,T] (NULL: none), gt_count [B]; MDCV_DETMAP_GT_LABELS: gt [B,T,5] the
 *      loader's zero-padded (class, cx, cy, w, h) rows, converted with width / height by the fp32 operations of mdcv_detect_post (a row with
 *      any of cx, cy, w, h <= 0 is padding), gt_cls / gt_ignore / gt_count not read.  iou_thr [J] and ranges [S][2] are HOST arrays.  A class
 *      outside 0..C-1 (detection or ground truth) takes no part.  Per image, class, threshold and range the rule is COCOeval.evaluateImg: a
 *      ground truth is ignored when flagged or when its area is outside the range; each detection, in row order, takes the unmatched
 *      non-ignored ground truth of its class with the largest IoU >= thr (equal IoU: the higher index), else an unmatched ignored one by the
 *      same rule; TP / IGNORED accordingly, unmatched: IGNORED when its own area is outside the range, else FP.  IoU and areas: the fp32
 *      arithmetic of the NMS (nms.py:24, 44-59) with the detection as the kept box.
 *      mdcv_detmap_finalize: over images 0 .. n_images-1.  A stable sort by (class, descending score) -- equal scores stay in image, then row
 *      order -- then per (c, j, s): q [C,J,S,101,2] i64 = the precision envelope at recall levels k / 100 as (numerator, denominator) in
 *      lowest terms, (0, 1) for a level never reached; tot [C,J,S,3] i64 = (n_gt, true positives, non-ignored detections); ap [C,J,S] f64 =
 *      (sum over k = 0..100 in that order of (double)num / (double)den) / 101, or -1 where n_gt == 0.  err: one i32, bit 0 set when a valid
 *      row's score is NaN or not positive (such a row is left out).  workspace: mdcv_detmap_finalize_workspace_bytes(cap, K) bytes, 8-byte
 *      aligned (MDCV_EARG outside the limits, -2 when the sort's size query fails). */
#define MDCV_DETMAP_MAX_GT 2048
#define MDCV_DETMAP_MAX_THR 10
#define MDCV_DETMAP_MAX_RANGES 4
#define MDCV_DETMAP_MAX_CLASSES 1024
#define MDCV_DETMAP_MAX_SLOTS 1073741824
#define MDCV_DETMAP_CHUNK 1024
#define MDCV_DETMAP_GT_PIXELS 0
#define MDCV_DETMAP_GT_LABELS 1
#define MDCV_DETMAP_FP 0
#define MDCV_DETMAP_TP 1
#define MDCV_DETMAP_IGNORED 2
int mdcv_detmap_match(const float* boxes, const float* prob, const int* cls, const int* count, int B, int K, int gt_mode, const float* gt,
                      const int* gt_cls, const unsigned char* gt_ignore, const int* gt_count, int T, float width, float height,
                      const float* iou_thr, int J, const float* ranges, int S, int C, long long first, long long cap, float* ds_score,
                      int* ds_cls, int* ds_count, unsigned* ds_status, long long* ds_n_gt, void* stream);
long long mdcv_detmap_finalize_workspace_bytes(long long cap, int K);
int mdcv_detmap_finalize(const float* ds_score, const int* ds_cls, const int* ds_count, const unsigned* ds_status, const long long* ds_n_gt,
                         long long n_images, long long cap, int K, int J, int S, int C, long long* q, long long* tot, double* ap, int* err,
                         void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
