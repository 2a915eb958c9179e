/* libmdcv_pnp.so — C ABI of the opt-in cone pose solver (csrc/cone_pnp.hip): the position and orientation of every cone in the
 * camera frame from its seven key points, a batched planar PnP.  It is the consumer of the key points behind
 * `FrameConeDetector(..., camera=)`, `TiledFrameConeDetector(..., camera=)` and `mdcv.rektnet.pose.solve_cone_pnp`.
 *
 * The conventions are those of include/mdcv_hip.h and of the other opt-in libraries: plain C symbols, plain pointers and sizes,
 * caller-owned device buffers, enqueue-only on the caller's HIP stream (`stream` = hipStream_t as void*), nothing allocated, 0 on success,
 * MDCV_EARG for an argument error (checked on the host before any GPU call), a positive hipError_t otherwise.  A header and a library of
 * its own for the reason include/mdcv_cls.h gives.
 *
 * Meaning (tests/helpers/pnp_numpy.py is the float64 restatement; all arithmetic is fp64).  For cone m:
 *   1. Camera: row owner[2m] of cam (fx, fy, cx, cy), row 0 when n_cam == 1.  Pinhole, no distortion.
 *   2. Image points: with window (x0, y0, w, h), u = x0 + (double)pts.x * w, v = y0 + (double)pts.y * h -- mdcv_kpt_draw_points's
 *      product without its truncation; without a window the points are pixels.
 *   3. Start A: R = I, tz = fy * (model y extent) / (image v extent), tx and ty put the model centroid on the centroid of the points.
 *   4. Levenberg-Marquardt on the 14 reprojection residuals, unknowns (dw, dt), R <- exp([dw]x) R, Marquardt damping
 *      (1 + lambda) on the diagonal of J^T J, lambda from 1e-3: a rejected step multiplies lambda by 10 (12 in a row end the start), an
 *      accepted one divides it by 10 (floor 1e-12).  A step is accepted when every point stays in front of the camera and the cost does
 *      not rise -- by more than 2^-36 sqrt(cost), the rounding of the residuals themselves.  A start ends when an accepted step moves the
 *      projections by |J d| <= 1e-10 px, or after max_iters accepted steps (MDCV_PNP_ITER_CAP).
 *   5. Start B: start A's result with its plane normal n = R e_z mirrored about the line of sight s to the model centroid,
 *      n' = 2 (n.s) s - n, by the minimal rotation; t kept; the same refinement.  B wins when its cost is below (1 - 2^-10) of A's.
 *   6. pose[16m..]: t (3), R (9, row-major), rms in pixels (sqrt(cost / 7)), the final costs of A and of B, 0.
 *      info[4m..]: status bits, accepted steps of A, of B, the start chosen (0 = A, 1 = B).
 *   7. A degenerate cone -- a point that is not finite, w or h <= 0, fx or fy <= 0 or a camera word that is not finite or an owner frame
 *      outside 0..n_cam-1, a zero v extent of the points or y extent of the model, a Cholesky pivot that is not positive and finite or a
 *      start behind the camera -- gets its status bit, 16 NaN pose words and zeros in info[1..3].  It never stalls the launch.
 * One launch, 256-thread workgroups of 32 cones, no workspace, no host read: it can be captured into a graph. */
#ifndef MDCV_PNP_H
#define MDCV_PNP_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef MDCV_OK
#define MDCV_OK 0
#define MDCV_EARG (-1)
#endif
#define MDCV_PNP_BAD_POINTS 1
#define MDCV_PNP_BAD_WINDOW 2
#define MDCV_PNP_BAD_CAMERA 4
#define MDCV_PNP_ZERO_EXTENT 8
#define MDCV_PNP_SINGULAR 16
#define MDCV_PNP_ITER_CAP 32          /* not degenerate: the pose is the last accepted one */
#define MDCV_PNP_POSE_WORDS 16
#define MDCV_PNP_MAX_CONES 1048576

/* pts f32 [M,7,2]; window i32 [M,4] or NULL; owner i32 [M,2] (frame, slot) or NULL (then n_cam must be 1); cam f64 [n_cam,4];
 * model f64 [7,3]; pose f64 [M,16]; info i32 [M,4] -- all device pointers.  MDCV_EARG: M < 0 or > MDCV_PNP_MAX_CONES, n_cam < 1,
 * max_iters < 1, a NULL pts, cam, model, pose or info, a NULL owner with n_cam > 1.  M == 0: MDCV_OK, nothing is enqueued. */
int mdcv_cone_pnp(const float* pts, const int* window, const int* owner, const double* cam, int n_cam, const double* model, int M,
                  int max_iters, double* pose, int* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
