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
//                   cyclic Jacobi with a fixed sweep count: nearest_rotation of rotation_fit.h, which the evaluator shares - and
//                   the second pass re-reads the K rotations (36 bytes each, in cache) for the spread instead of keeping 8 x 9
//                   doubles live across the solve.  All arithmetic in fp64 with contraction off; every output is rounded once.
// Every output word has exactly one writer and every value is a function of its own (crop, joint): the result does not depend on
// the grid.  The loops run over K and fixed counts only; nothing iterates on the data.
#include "common.h"
#include "kernels.h"
#include "rotation_fit.h"

#include <cstdint>

namespace {

constexpr int NJ = 24;
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
    nearest_rotation<ROT_JACOBI_SWEEPS>(M, Rp);
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
