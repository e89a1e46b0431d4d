// The ground-truth rotation of one SMPL joint: shared by poco_op_rodrigues, the evaluator's pose distance (eval_metrics.hip) and the
// flow residual (eval_likelihood.hip), so that all three see the same R_gt bits.
#pragma once
#include <hip/hip_runtime.h>

// batch_rodrigues + quat_to_rotmat (geometry.py:207-244) of one axis-angle vector: the norm is taken of theta + 1e-8, the vector
// is divided by that norm, the quaternion (cos(a/2), sin(a/2) n) is renormalised and expanded.  fp64 inside, R row-major.
__device__ __forceinline__ void rodrigues_f64(const float* __restrict__ aa, double* R) {
  const double tx = aa[0], ty = aa[1], tz = aa[2];
  const double ex = tx + 1e-8, ey = ty + 1e-8, ez = tz + 1e-8;
  const double angle = sqrt(ex * ex + ey * ey + ez * ez);
  const double nx = tx / angle, ny = ty / angle, nz = tz / angle;
  const double half = angle * 0.5;
  const double c = cos(half), s = sin(half);
  double w = c, x = s * nx, y = s * ny, z = s * nz;
  const double qn = sqrt(w * w + x * x + y * y + z * z);
  w /= qn; x /= qn; y /= qn; z /= qn;
  const double w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const double wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
  R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;   R[2] = 2 * wy + 2 * xz;
  R[3] = 2 * wz + 2 * xy;   R[4] = w2 - x2 + y2 - z2; R[5] = 2 * yz - 2 * wx;
  R[6] = 2 * xz - 2 * wy;   R[7] = 2 * wx + 2 * yz;   R[8] = w2 - x2 - y2 + z2;
}
