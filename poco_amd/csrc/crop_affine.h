// The affine part of the crops, shared by the demo crop (kernels_misc.hip) and the dataset crop (dataset_crop.hip): OpenCV 4.5.5's
// getAffineTransform (LU in double) and the inversion cv::warpAffine applies, restated step by step (oracle/crop_np.py).
#pragma once
#include <hip/hip_runtime.h>

namespace crop_affine {
// cv::hal::LU64f (LUImpl<double>, opencv/modules/core/src/matrix_decomp.cpp) for the 6x6 system of getAffineTransform.
__device__ __forceinline__ void lu_solve6(double (&A)[6][6], double (&b)[6]) {
#pragma clang fp contract(off)
  // fully unrolled with static indices (the pivot row is swapped in through selects) so that A lives in registers
  bool singular = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    int k = i;
    double best = fabs(A[i][i]);
#pragma unroll
    for (int j = i + 1; j < 6; ++j)
      if (fabs(A[j][i]) > best) { best = fabs(A[j][i]); k = j; }
    singular = singular || best < 2.220446049250313e-16 * 100;      // cv::solve returns false and leaves zeros
#pragma unroll
    for (int j = i + 1; j < 6; ++j) {
      const bool sw = k == j;
#pragma unroll
      for (int c = i; c < 6; ++c) {
        const double t = A[i][c];
        A[i][c] = sw ? A[j][c] : t;
        A[j][c] = sw ? t : A[j][c];
      }
      const double t = b[i];
      b[i] = sw ? b[j] : t;
      b[j] = sw ? t : b[j];
    }
    const double d = -1.0 / A[i][i];
#pragma unroll
    for (int j = i + 1; j < 6; ++j) {
      const double alpha = A[j][i] * d;
#pragma unroll
      for (int c = i + 1; c < 6; ++c) A[j][c] = A[j][c] + alpha * A[i][c];
      b[j] = b[j] + alpha * b[i];
    }
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = b[i];
#pragma unroll
    for (int c = i + 1; c < 6; ++c) s = s - A[i][c] * b[c];
    b[i] = s / A[i][i];
  }
  if (singular) {
#pragma unroll
    for (int j = 0; j < 6; ++j) b[j] = 0.0;
  }
}

// getAffineTransform(src, dst) of three float32 point pairs -> the inversion cv::warpAffine applies: Mi[6].
__device__ __forceinline__ void inverse_affine_from_points(const float (&sx)[3], const float (&sy)[3], const float (&dx)[3],
                                                           const float (&dy)[3], double (&Mi)[6]) {
#pragma clang fp contract(off)
  double A[6][6], b[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) A[i][j] = 0.0;
  for (int i = 0; i < 3; ++i) {
    A[2 * i][0] = A[2 * i + 1][3] = sx[i];
    A[2 * i][1] = A[2 * i + 1][4] = sy[i];
    A[2 * i][2] = A[2 * i + 1][5] = 1.0;
    b[2 * i] = dx[i];
    b[2 * i + 1] = dy[i];
  }
  lu_solve6(A, b);
  double D = b[0] * b[4] - b[1] * b[3];
  D = D != 0.0 ? 1.0 / D : 0.0;
  const double A11 = b[4] * D, A22 = b[0] * D;
  Mi[0] = A11;
  Mi[1] = b[1] * -D;
  Mi[3] = b[3] * -D;
  Mi[4] = A22;
  Mi[2] = -Mi[0] * b[2] - Mi[1] * b[5];
  Mi[5] = -Mi[3] * b[2] - Mi[4] * b[5];
}

__device__ __forceinline__ int cv_round(double v) { return __double2int_rn(v); }      // cvRound: round half to even
}  // namespace crop_affine
