// Cone positions from key points: batched planar PnP (include/mdcv_pnp.h; tests/helpers/pnp_numpy.py is the definition).
//
// The workload is small (at most batch_size x max_cones = 1024 cones a batch) and latency-bound, so the split is chosen for the length of
// one cone's dependency chain, not for throughput:
//   * one 8-lane group per cone, key point k on lane k, lane 7 contributing zeros: eight cones a wave, 32 a workgroup;
//   * each lane forms its point's two Jacobian rows in registers and its share of the 21 + 6 + 1 sums of J^T J, J^T r and the cost;
//   * three xor-shuffle steps inside the group add them up.  The butterfly adds the same pairs on every lane, so all eight lanes hold
//     bit-identical sums and each solves the damped 6 x 6 system redundantly by Cholesky in registers: nothing is broadcast;
//   * no LDS, no barrier.  The loop is wave-uniform over "any group still running": every pass makes exactly ONE evaluation of the
//     normal equations at a candidate pose, and a per-group state machine decides what the candidate is (start A, a Levenberg-Marquardt
//     step, start B) and what to do with the answer.  A finished group keeps evaluating its last pose and ignores the result;
//   * fp64 throughout, sincos and sqrt of the exponential map included.
#include <hip/hip_runtime.h>
#include "../../include/mdcv_pnp.h"

namespace {

constexpr int kBlock = 256, kGroup = 8, kPoints = 7;
constexpr double kLambda0 = 1e-3, kLambdaMin = 1e-12;
constexpr int kMaxTrials = 12;
constexpr double kCostNoise = 1.0 / 68719476736.0;      // 2^-36
constexpr double kStepTol2 = 1e-10 * 1e-10;
constexpr double kTie = 1.0 / 1024.0;

enum Mode { INIT = 0, RUN = 1, DONE = 2 };

struct PnpArgs {
  const float* pts; const int* window; const int* owner; const double* cam; int n_cam; const double* model; int M, max_iters;
  double* pose; int* info;
};

__device__ __forceinline__ double group_sum(double v) {
  v += __shfl_xor(v, 1, kGroup); v += __shfl_xor(v, 2, kGroup); v += __shfl_xor(v, 4, kGroup);
  return v;
}
__device__ __forceinline__ int group_or(int v) {
  v |= __shfl_xor(v, 1, kGroup); v |= __shfl_xor(v, 2, kGroup); v |= __shfl_xor(v, 4, kGroup);
  return v;
}
__device__ __forceinline__ double group_max(double v) {
  v = fmax(v, __shfl_xor(v, 1, kGroup)); v = fmax(v, __shfl_xor(v, 2, kGroup)); v = fmax(v, __shfl_xor(v, 4, kGroup));
  return v;
}

// the normal equations at (R, t): N[0..20] = J^T J (lower triangle, row-major), N[21..26] = J^T r, N[27] = cost; -> every point in front.
// Unknowns (w, t), R <- exp([dw]x) R, so d(RP + t)/dw = -[RP]x.  `live` is false on lane 7, whose share is zero.
__device__ __forceinline__ bool normal_equations(bool live, const double P[3], double u, double v, const double cam[4], const double R[9],
                                                 const double t[3], double N[28]) {
  const double qx = R[0] * P[0] + R[1] * P[1] + R[2] * P[2], qy = R[3] * P[0] + R[4] * P[1] + R[5] * P[2],
               qz = R[6] * P[0] + R[7] * P[1] + R[8] * P[2];
  const double X = qx + t[0], Y = qy + t[1], Z = qz + t[2];
  const bool behind = live && !(Z > 0.0);
  const double iz = 1.0 / Z, x = X * iz, y = Y * iz, a = cam[0] * iz, b = cam[1] * iz;
  const double ru = cam[0] * x + cam[2] - u, rv = cam[1] * y + cam[3] - v;
  const double ju[6] = {-a * x * qy, a * (qz + x * qx), -a * qy, a, 0.0, -a * x};
  const double jv[6] = {-b * (qz + y * qy), b * y * qx, b * qx, 0.0, b, -b * y};
  int n = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) N[n++] = ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) N[21 + i] = ju[i] * ru + jv[i] * rv;
  N[27] = ru * ru + rv * rv;
#pragma unroll
  for (int i = 0; i < 28; ++i) N[i] = group_sum(live ? N[i] : 0.0);
  return group_or(behind ? 1 : 0) == 0;
}

// (A + lam diag A) d = -g by Cholesky, A = N[0..20], g = N[21..26]; false when a pivot is not positive and finite
__device__ __forceinline__ bool damped_solve(const double N[28], double lam, double d[6]) {
  double L[6][6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = N[j * (j + 1) / 2 + j] * (1.0 + lam);
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    ok = ok && s > 0.0 && s <= 1.7976931348623157e308;
    const double inv = 1.0 / sqrt(s);
    L[j][j] = inv;                                                       // the reciprocal of the pivot
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double e = N[i * (i + 1) / 2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) e -= L[i][k] * L[j][k];
      L[i][j] = e * inv;
    }
  }
  double yv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double e = -N[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) e -= L[i][k] * yv[k];
    yv[i] = e * L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double e = yv[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) e -= L[k][i] * d[k];
    d[i] = e * L[i][i];
  }
  return ok;
}

// out = (I + a K + b K^2) R with K = [w]x
__device__ __forceinline__ void rotate(const double w[3], double a, double b, const double R[9], double out[9]) {
  const double E[9] = {1.0 - b * (w[1] * w[1] + w[2] * w[2]), -a * w[2] + b * w[0] * w[1], a * w[1] + b * w[0] * w[2],
                       a * w[2] + b * w[0] * w[1], 1.0 - b * (w[0] * w[0] + w[2] * w[2]), -a * w[0] + b * w[1] * w[2],
                       -a * w[1] + b * w[0] * w[2], a * w[0] + b * w[1] * w[2], 1.0 - b * (w[0] * w[0] + w[1] * w[1])};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j] + E[3 * i + 2] * R[6 + j];
}

// exp([w]x) R
__device__ __forceinline__ void exp_rotate(const double w[3], const double R[9], double out[9]) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  double a, b;
  if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
  else { double s, c; sincos(th, &s, &c); a = s / th; b = (1.0 - c) / th2; }
  rotate(w, a, b, R, out);
}

// start B: R with its plane normal n = R e_z mirrored about the line of sight to the model centroid mc, by the minimal rotation
__device__ __forceinline__ void mirror(const double R[9], const double t[3], const double mc[3], double out[9]) {
  const double n[3] = {R[2], R[5], R[8]};
  double c[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = R[3 * i] * mc[0] + R[3 * i + 1] * mc[1] + R[3 * i + 2] * mc[2] + t[i];
  const double inv = 1.0 / sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  const double s[3] = {c[0] * inv, c[1] * inv, c[2] * inv};
  const double ns = 2.0 * (n[0] * s[0] + n[1] * s[1] + n[2] * s[2]);
  const double m[3] = {ns * s[0] - n[0], ns * s[1] - n[1], ns * s[2] - n[2]};
  const double ax[3] = {n[1] * m[2] - n[2] * m[1], n[2] * m[0] - n[0] * m[2], n[0] * m[1] - n[1] * m[0]};
  const double co = n[0] * m[0] + n[1] * m[1] + n[2] * m[2];
  if (!(1.0 + co > 1e-12)) {                                             // seen edge-on: the mirror image is the pose itself
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = R[i];
    return;
  }
  rotate(ax, 1.0, 1.0 / (1.0 + co), R, out);
}

__global__ __launch_bounds__(kBlock) void cone_pnp_kernel(PnpArgs A) {
  const int gid = blockIdx.x * kBlock + threadIdx.x;
  const int m = gid / kGroup, k = gid % kGroup;
  const bool cone = m < A.M, live = cone && k < kPoints;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- the model (shared by every cone), this lane's point of it, centroid and y extent
  double P[3] = {0.0, 0.0, 0.0}, mc[3] = {0.0, 0.0, 0.0}, ylo = 0.0, yhi = 0.0;
  for (int i = 0; i < kPoints; ++i) {
    const double px = A.model[3 * i], py = A.model[3 * i + 1], pz = A.model[3 * i + 2];
    mc[0] += px; mc[1] += py; mc[2] += pz;
    ylo = i == 0 ? py : fmin(ylo, py); yhi = i == 0 ? py : fmax(yhi, py);
    if (i == k) { P[0] = px; P[1] = py; P[2] = pz; }
  }
  mc[0] /= 7.0; mc[1] /= 7.0; mc[2] /= 7.0;
  const double ext_y = yhi - ylo;

  // ---- this cone's camera, window and point; the degenerate kinds
  int status = 0;
  double cam[4] = {1.0, 1.0, 0.0, 0.0}, u = 0.0, v = 0.0;
  if (cone) {
    int row = 0;
    if (A.n_cam > 1) row = A.owner[2 * (size_t)m];
    if (row < 0 || row >= A.n_cam) status |= MDCV_PNP_BAD_CAMERA;
    else {
#pragma unroll
      for (int i = 0; i < 4; ++i) cam[i] = A.cam[4 * (size_t)row + i];
      bool fin = true;
#pragma unroll
      for (int i = 0; i < 4; ++i) fin = fin && fabs(cam[i]) <= 1.7976931348623157e308;
      if (!(cam[0] > 0.0 && cam[1] > 0.0 && fin)) status |= MDCV_PNP_BAD_CAMERA;
    }
    double x0 = 0.0, y0 = 0.0, w = 1.0, h = 1.0;
    if (A.window) {
      const int* win = A.window + 4 * (size_t)m;
      x0 = win[0]; y0 = win[1]; w = win[2]; h = win[3];
      if (win[2] <= 0 || win[3] <= 0) status |= MDCV_PNP_BAD_WINDOW;
    }
    if (live) {
      const float px = A.pts[((size_t)m * kPoints + k) * 2], py = A.pts[((size_t)m * kPoints + k) * 2 + 1];
      if (!(fabsf(px) <= 3.402823466e38f && fabsf(py) <= 3.402823466e38f)) status |= MDCV_PNP_BAD_POINTS;
      u = x0 + (double)px * w; v = y0 + (double)py * h;
    }
  }
  status = group_or(status);
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double vhi = group_max(live ? v : -inf), vlo = -group_max(live ? -v : -inf);
  const double ub = group_sum(live ? u : 0.0) / 7.0, vb = group_sum(live ? v : 0.0) / 7.0;
  const double ext_v = vhi - vlo;
  if (cone && status == 0 && !(ext_v > 0.0 && ext_y > 0.0)) status |= MDCV_PNP_ZERO_EXTENT;

  // ---- state: the current pose and its normal equations, the candidate, start A's result
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 1.0}, N[28];
  double Rc[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tc[3] = {0.0, 0.0, 1.0}, Nc[28], d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double RA[9], tA[3], costA = nan, costB = nan, lam = kLambda0;
  int itA = 0, itB = 0, flagA = 0, flagB = 0, iters = 0, trials = 0, phase = 0;
  int mode = (cone && status == 0) ? INIT : DONE;
#pragma unroll
  for (int i = 0; i < 28; ++i) N[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) RA[i] = R[i];
  tA[0] = tA[1] = 0.0; tA[2] = 1.0;
  if (mode == INIT) {
    const double tz = cam[1] * ext_y / ext_v;
    tc[0] = tz * (ub - cam[2]) / cam[0] - mc[0]; tc[1] = tz * (vb - cam[3]) / cam[1] - mc[1]; tc[2] = tz - mc[2];
  }

  while (__any(mode != DONE)) {
    // -- the candidate of this pass
    bool solved = true;
    if (mode == RUN) {
      solved = damped_solve(N, lam, d);
      exp_rotate(d, R, Rc);
      tc[0] = t[0] + d[3]; tc[1] = t[1] + d[4]; tc[2] = t[2] + d[5];
    }
    // -- one evaluation, uniform over the wave
    const bool front = normal_equations(live, P, u, v, cam, Rc, tc, Nc);
    // -- what the group makes of it
    int finish = -1;                                                      // >= 0: this start ends with these flag bits
    if (mode == INIT) {
      if (front) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = tc[i];
#pragma unroll
        for (int i = 0; i < 28; ++i) N[i] = Nc[i];
        lam = kLambda0; iters = 0; trials = 0; mode = RUN;
      } else {
        N[27] = inf; iters = 0; finish = MDCV_PNP_SINGULAR;               // a start behind the camera
      }
    } else if (mode == RUN) {
      if (!solved) finish = MDCV_PNP_SINGULAR;
      else if (front && Nc[27] <= N[27] + kCostNoise * sqrt(N[27])) {
        double moved = 0.0;                                               // |J d|^2 = d^T (J^T J) d
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) moved += (i == j ? 1.0 : 2.0) * d[i] * d[j] * N[i * (i + 1) / 2 + j];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = tc[i];
#pragma unroll
        for (int i = 0; i < 28; ++i) N[i] = Nc[i];
        lam = fmax(lam * 0.1, kLambdaMin); ++iters; trials = 0;
        if (moved <= kStepTol2) finish = 0;
        else if (iters >= A.max_iters) finish = MDCV_PNP_ITER_CAP;
      } else {
        lam *= 10.0;
        if (++trials >= kMaxTrials) finish = 0;                           // no step of any length lowers the cost: a minimum, to rounding
      }
    }
    if (finish >= 0) {
      if (phase == 0) {
        if (finish & MDCV_PNP_SINGULAR) { status |= MDCV_PNP_SINGULAR; mode = DONE; }
        else {
#pragma unroll
          for (int i = 0; i < 9; ++i) RA[i] = R[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) tA[i] = t[i];
          costA = N[27]; itA = iters; flagA = finish;
          mirror(RA, tA, mc, Rc);
#pragma unroll
          for (int i = 0; i < 3; ++i) tc[i] = tA[i];
          phase = 1; mode = INIT;
        }
      } else {
        costB = N[27]; itB = iters; flagB = finish; mode = DONE;
      }
    }
  }

  // ---- the result: lane 0 of the group writes the cone's words
  if (cone && k == 0) {
    double* pose = A.pose + (size_t)m * MDCV_PNP_POSE_WORDS;
    int* info = A.info + 4 * (size_t)m;
    if (status != 0) {
#pragma unroll
      for (int i = 0; i < MDCV_PNP_POSE_WORDS; ++i) pose[i] = nan;
      info[0] = status; info[1] = 0; info[2] = 0; info[3] = 0;
    } else {
      const bool b = !(flagB & MDCV_PNP_SINGULAR) && costB < (1.0 - kTie) * costA;
#pragma unroll
      for (int i = 0; i < 3; ++i) pose[i] = b ? t[i] : tA[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) pose[3 + i] = b ? R[i] : RA[i];
      pose[12] = sqrt((b ? costB : costA) / 7.0); pose[13] = costA; pose[14] = costB; pose[15] = 0.0;
      info[0] = (b ? flagB : flagA) & MDCV_PNP_ITER_CAP; info[1] = itA; info[2] = itB; info[3] = b ? 1 : 0;
    }
  }
}

}  // namespace

extern "C" {

int mdcv_cone_pnp(const float* pts, const int* window, const int* owner, const double* cam, int n_cam, const double* model, int M,
                  int max_iters, double* pose, int* info, void* stream) {
  if (M < 0 || M > MDCV_PNP_MAX_CONES || n_cam < 1 || max_iters < 1) return MDCV_EARG;
  if (!pts || !cam || !model || !pose || !info || (n_cam > 1 && !owner)) return MDCV_EARG;
  if (M == 0) return MDCV_OK;
  PnpArgs a{pts, window, owner, cam, n_cam, model, M, max_iters, pose, info};
  const int per = kBlock / kGroup;
  hipLaunchKernelGGL(cone_pnp_kernel, dim3((unsigned)((M + per - 1) / per)), dim3(kBlock), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCV_OK : (int)e;
}

}  // extern "C"
