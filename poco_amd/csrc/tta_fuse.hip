// Test-time augmentation (eval.py / demo.py --tta VIEWS): K views of every crop - the crop itself, mirrored, rotated, rescaled - go
// through ONE forward, and this operator takes each view's prediction back into the frame of the untransformed crop and fuses
// them per joint, weighted by the model's own uncertainty or uniformly.  The reference has no code for this; what it supplies are
// the transforms to undo: flip_pose and rot_aa (pocolib/utils/image_utils.py:236-247,269-278) in the order of pose_processing
// (base_dataset.py:253-262: rotate first, flip second, so the un-flip comes first here).  The contract is stated in
// include/poco_hip.h (poco_op_tta_fuse) and DESIGN.md section 26; tests/tta_np.py restates it in float64 numpy with plain loops.
//
// One launch on the caller's stream, nothing read back, no atomics, no LDS, no barrier:
//   tta_fuse_rows   one lane per (crop, joint), lanes dealt by a grid-stride loop over the B * 24 entries.  A lane walks the K
//                   views twice: the first pass forms M = sum w_k R_k, W and sum w_k v_k (the lane of joint 0 also the ten shape
//                   sums), then the rotation nearest to M - Horn's quaternion form, the largest eigenvector of a symmetric 4x4 by
//                   cyclic Jacobi with the fixed sweep count of eval_metrics.hip, restated here so that file stays as it is - and
//                   the second pass re-reads the K rotations (36 bytes each, in cache) for the spread instead of keeping 8 x 9
//                   doubles live across the solve.  All arithmetic in fp64 with contraction off; every output is rounded once.
// Every output word has exactly one writer and every value is a function of its own (crop, joint): the result does not depend on
// the grid.  The loops run over K and fixed counts only; nothing iterates on the data.
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int NJ = 24;
constexpr int TTA_JACOBI_SWEEPS = 10;                                 // EV_JACOBI_SWEEPS of eval_metrics.hip
// pocolib/core/constants.py:104-111 (poco_amd/datacrop.py SMPL_JOINTS_FLIP_PERM)
__constant__ int kFlipPerm[NJ] = {0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22};

struct TtaDev {
  const float *pose, *var, *betas;
  float *pose_out, *var_out, *spread, *betas_out;
  TtaViews views;
  int B, weight;
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for NaN and +-Inf

// View k of (b, j) in the base frame: the source joint's nine floats un-flipped and, for the root of a rotated view, rotated
// back.  Returns the view's weight (0 = dropped: R and v are then not to be used) and leaves the row's index in `row`.
__device__ __forceinline__ double load_view(const TtaDev& a, int k, int b, int j, double (&R)[9], double& v, size_t& row) {
  #pragma clang fp contract(off)
  const int flip = a.views.flip[k];
  const int js = flip ? kFlipPerm[j] : j;
  row = (size_t)k * (size_t)a.B + (size_t)b;
  const float* p = a.pose + (row * NJ + js) * 9;
  const float vf = a.var[row * NJ + js];
  bool ok = finite_f(vf) && vf >= 0.f;
  #pragma unroll
  for (int i = 0; i < 9; ++i) {
    const float x = p[i];
    ok = ok && finite_f(x);
    R[i] = (double)x;
  }
  v = (double)vf;
  if (!ok) return 0.0;
  if (flip) {                                                         // R[i][c] *= m_i m_c, m = (1, -1, -1): exact
    R[1] = -R[1]; R[2] = -R[2]; R[3] = -R[3]; R[6] = -R[6];
  }
  const double c = a.views.c[k], s = a.views.s[k];
  if (j == 0 && !(c == 1.0 && s == 0.0)) {                            // Rz R: rows 0 and 1 mix, row 2 stays
    #pragma unroll
    for (int col = 0; col < 3; ++col) {
      const double r0 = R[col], r1 = R[3 + col];
      R[col] = c * r0 - s * r1;
      R[3 + col] = s * r0 + c * r1;
    }
  }
  return a.weight ? 1.0 / (v + 1e-9) : 1.0;
}

// One Jacobi rotation of the symmetric 4x4 `a` in the (p, q) plane, accumulated into the eigenvector matrix `v` (columns):
// jacobi_rotate of eval_metrics.hip, restated.
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

// argmax over SO(3) of tr(R^T M) = the unit quaternion that maximises q^T N q (Horn 1987) with N built from K = M^T, as
// eval_crop builds it from its K.  A singular M (views half a turn apart) still yields a rotation: whichever eigenvector the
// sweeps leave under the largest diagonal entry.
__device__ __forceinline__ void nearest_rotation(const double (&M)[9], double (&R)[9]) {
  #pragma clang fp contract(off)
  double N[4][4], E[4][4];
  const double k00 = M[0], k01 = M[3], k02 = M[6], k10 = M[1], k11 = M[4], k12 = M[7], k20 = M[2], k21 = M[5], k22 = M[8];
  N[0][0] = k00 + k11 + k22;
  N[1][1] = k00 - k11 - k22;
  N[2][2] = -k00 + k11 - k22;
  N[3][3] = -k00 - k11 + k22;
  N[0][1] = N[1][0] = k12 - k21;
  N[0][2] = N[2][0] = k20 - k02;
  N[0][3] = N[3][0] = k01 - k10;
  N[1][2] = N[2][1] = k01 + k10;
  N[1][3] = N[3][1] = k20 + k02;
  N[2][3] = N[3][2] = k12 + k21;
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    #pragma unroll
    for (int c = 0; c < 4; ++c) E[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < TTA_JACOBI_SWEEPS; ++sweep) {
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

__global__ __launch_bounds__(TTA_THREADS) void tta_fuse_rows(TtaDev a) {
  #pragma clang fp contract(off)
  const int K = a.views.count;
  const long long total = (long long)a.B * NJ;
  for (long long idx = (long long)blockIdx.x * TTA_THREADS + threadIdx.x; idx < total; idx += (long long)gridDim.x * TTA_THREADS) {
    const int b = (int)(idx / NJ), j = (int)(idx % NJ);
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bsum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double W = 0.0, SV = 0.0;
    for (int k = 0; k < K; ++k) {
      double R[9], v;
      size_t row;
      const double w = load_view(a, k, b, j, R, v, row);
      if (w > 0.0) {
        #pragma unroll
        for (int i = 0; i < 9; ++i) M[i] = M[i] + w * R[i];
        W = W + w;
        SV = SV + w * v;
        if (j == 0) {                                                 // g_k = the joint-0 weight: this lane's w
          #pragma unroll
          for (int i = 0; i < 10; ++i) bsum[i] = bsum[i] + w * (double)a.betas[row * 10 + i];
        }
      }
    }
    const size_t o = (size_t)idx;                                     // = b * 24 + j
    if (!(W > 0.0)) {                                                 // every view dropped: the base view's words, spread NaN
      const uint32_t* p = reinterpret_cast<const uint32_t*>(a.pose) + o * 9;      // view 0 is the identity: row b, joint j
      #pragma unroll
      for (int i = 0; i < 9; ++i) reinterpret_cast<uint32_t*>(a.pose_out)[o * 9 + i] = p[i];
      reinterpret_cast<uint32_t*>(a.var_out)[o] = reinterpret_cast<const uint32_t*>(a.var)[o];
      reinterpret_cast<uint32_t*>(a.spread)[o] = 0x7fc00000u;
      if (j == 0) {
        #pragma unroll
        for (int i = 0; i < 10; ++i)
          reinterpret_cast<uint32_t*>(a.betas_out)[(size_t)b * 10 + i] = reinterpret_cast<const uint32_t*>(a.betas)[(size_t)b * 10 + i];
      }
      continue;
    }
    double Rp[9];
    nearest_rotation(M, Rp);
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      double R[9], v;
      size_t row;
      const double w = load_view(a, k, b, j, R, v, row);
      if (w > 0.0) {
        double d = 0.0;
        #pragma unroll
        for (int i = 0; i < 9; ++i) { const double df = R[i] - Rp[i]; d = d + df * df; }
        acc = acc + w * (d / 9.0);
      }
    }
    #pragma unroll
    for (int i = 0; i < 9; ++i) a.pose_out[o * 9 + i] = (float)Rp[i];
    a.var_out[o] = (float)(SV / W);
    a.spread[o] = (float)(acc / W);
    if (j == 0) {
      #pragma unroll
      for (int i = 0; i < 10; ++i) a.betas_out[(size_t)b * 10 + i] = (float)(bsum[i] / W);
    }
  }
}

}  // namespace

void launch_tta_fuse(const float* pose, const float* var, const float* betas, int B, const TtaViews& views, int weight, float* pose_out,
                     float* var_out, float* spread, float* betas_out, int max_blocks, hipStream_t s) {
  const TtaDev d{pose, var, betas, pose_out, var_out, spread, betas_out, views, B, weight};
  const int cap = max_blocks > 0 && max_blocks < TTA_MAX_BLOCKS ? max_blocks : TTA_MAX_BLOCKS;
  const long long need = ((long long)B * NJ + TTA_THREADS - 1) / TTA_THREADS;
  tta_fuse_rows<<<(int)(need < cap ? need : cap), TTA_THREADS, 0, s>>>(d);
}
