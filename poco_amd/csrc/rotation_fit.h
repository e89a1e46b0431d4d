// The rotation nearest to a 3x3 matrix, and the precision weight of an uncertainty: shared by test-time augmentation (tta_fuse.hip),
// the track smoother (track_smooth.hip), the keypoint refit (kp_refit.hip) and - Horn's matrix and the sweep count - the evaluator's
// Procrustes solve (eval_metrics.hip).  fp64 with contraction off in every function, whatever the including file's setting.  A new
// kernel that needs one of these includes this header; it does not restate them.
#pragma once
#include <hip/hip_runtime.h>

constexpr int ROT_JACOBI_SWEEPS = 10;                                 // cyclic sweeps of the 4x4 solve: see DESIGN.md "Evaluation"
constexpr double UNCERT_W_MIN = 1e-6, UNCERT_W_MAX = 1e6, UNCERT_U_MIN = 1e-6;

// One Jacobi rotation of the symmetric 4x4 `a` in the (p, q) plane, accumulated into the eigenvector matrix `v` (columns).
__device__ __forceinline__ void jacobi_rotate(double (&a)[4][4], double (&v)[4][4], int p, int q) {
  #pragma clang fp contract(off)
  const double apq = a[p][q];
  if (!(apq != 0.0)) return;                                          // zero (or NaN: nothing to gain): a branch, not a loop
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  #pragma unroll
  for (int k = 0; k < 4; ++k) {                                       // A <- A G
    const double akp = a[k][p], akq = a[k][q];
    a[k][p] = c * akp - s * akq;
    a[k][q] = s * akp + c * akq;
  }
  #pragma unroll
  for (int k = 0; k < 4; ++k) {                                       // A <- G^T A
    const double apk = a[p][k], aqk = a[q][k];
    a[p][k] = c * apk - s * aqk;
    a[q][k] = s * apk + c * aqk;
  }
  #pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double vkp = v[k][p], vkq = v[k][q];
    v[k][p] = c * vkp - s * vkq;
    v[k][q] = s * vkp + c * vkq;
  }
}

// Horn's (1987) symmetric 4x4 of a 3x3 K: the unit quaternion q of the rotation R that maximises tr(R K) maximises q^T N q.
__device__ __forceinline__ void horn_matrix(const double (&K)[3][3], double (&N)[4][4]) {
  #pragma clang fp contract(off)
  N[0][0] = K[0][0] + K[1][1] + K[2][2];
  N[1][1] = K[0][0] - K[1][1] - K[2][2];
  N[2][2] = -K[0][0] + K[1][1] - K[2][2];
  N[3][3] = -K[0][0] - K[1][1] + K[2][2];
  N[0][1] = N[1][0] = K[1][2] - K[2][1];
  N[0][2] = N[2][0] = K[2][0] - K[0][2];
  N[0][3] = N[3][0] = K[0][1] - K[1][0];
  N[1][2] = N[2][1] = K[0][1] + K[1][0];
  N[1][3] = N[3][1] = K[2][0] + K[0][2];
  N[2][3] = N[3][2] = K[1][2] + K[2][1];
}

// The rotation nearest to the row-major 3x3 M, row-major: argmax over SO(3) of tr(R^T M), i.e. of tr(R K) with K = M^T.  The largest
// eigenvector of horn_matrix(K) by SWEEPS cyclic Jacobi sweeps from E = I - a fixed count, nothing iterates on the data - taken from
// under the largest diagonal entry, normalised and expanded.  A singular M still yields a rotation: whichever eigenvector the sweeps
// leave there.
template <int SWEEPS>
__device__ __forceinline__ void nearest_rotation(const double (&M)[9], double (&R)[9]) {
  #pragma clang fp contract(off)
  const double K[3][3] = {{M[0], M[3], M[6]}, {M[1], M[4], M[7]}, {M[2], M[5], M[8]}};
  double N[4][4], E[4][4];
  horn_matrix(K, N);
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    #pragma unroll
    for (int c = 0; c < 4; ++c) E[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    jacobi_rotate(N, E, 0, 1); jacobi_rotate(N, E, 0, 2); jacobi_rotate(N, E, 0, 3);
    jacobi_rotate(N, E, 1, 2); jacobi_rotate(N, E, 1, 3); jacobi_rotate(N, E, 2, 3);
  }
  double qw = E[0][0], qx = E[1][0], qy = E[2][0], qz = E[3][0], best = N[0][0];
  #pragma unroll
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > best) { best = N[k][k]; qw = E[0][k]; qx = E[1][k]; qy = E[2][k]; qz = E[3][k]; }
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  R[0] = qw * qw + qx * qx - qy * qy - qz * qz; R[1] = 2.0 * (qx * qy - qw * qz); R[2] = 2.0 * (qx * qz + qw * qy);
  R[3] = 2.0 * (qx * qy + qw * qz); R[4] = qw * qw - qx * qx + qy * qy - qz * qz; R[5] = 2.0 * (qy * qz - qw * qx);
  R[6] = 2.0 * (qx * qz - qw * qy); R[7] = 2.0 * (qy * qz + qw * qx); R[8] = qw * qw - qx * qx - qy * qy + qz * qz;
}

// w = clamp((u_ref / max(u, 1e-6))^2, 1e-6, 1e6); a NaN or an infinity of either sign gives 1e-6
__device__ __forceinline__ double uncert_weight(float uf, double u_ref) {
  #pragma clang fp contract(off)
  if (!(fabsf(uf) <= 3.402823466e+38f)) return UNCERT_W_MIN;
  const double u = (double)uf;
  const double r = u_ref / (u > UNCERT_U_MIN ? u : UNCERT_U_MIN);
  const double w = r * r;
  return w < UNCERT_W_MIN ? UNCERT_W_MIN : (w > UNCERT_W_MAX ? UNCERT_W_MAX : w);
}
