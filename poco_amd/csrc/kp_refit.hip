// Video mode's keypoint refit (demo.py --mode video --kp_refit LAMBDA, eval.py --kp_refit LAMBDA): every row's 24 joint rotations and
// its weak-perspective camera are refitted to the row's 2-D keypoints by Levenberg-Marquardt, the network's own pose being the prior
// and each joint held by its own precision lam (u_ref / u)^2.  No counterpart in the reference (its smplify_runner is not in its
// tree).  The contract is stated in include/poco_hip.h (poco_op_kp_refit) and DESIGN.md section 31; tests/refit_np.py restates it in
// float64 numpy with dense matrices and numpy.linalg.cholesky.
//
// One launch on the caller's stream, nothing read back, no atomics, no scratch in global memory.  A block of KP_REFIT_THREADS = 128
// takes one row at a time (rows are dealt to the blocks by a grid-stride loop) and keeps everything in LDS, 41 KB:
//   evaluate  q_j = Log(Rnet_j^T R_j), one lane per joint; forward kinematics level by level of the tree (8 levels for SMPL), one
//             lane per joint of the level; the residuals, one lane per keypoint; F is then summed by every lane for itself in the
//             fixed order keypoints, joints, camera: no reduction tree, the same bits in every lane, so the accept test is uniform.
//   normal    A is the packed lower triangle of a 76 x 76 matrix: rows 0 .. 74 the normal matrix, row 75 the right-hand side -g.
//             A keypoint's Jacobian rows are non-zero only in the 3 x (proper ancestors of its joint) + 3 camera columns; they are
//             formed compactly (at most 72 columns, double-buffered: one barrier per keypoint) and their outer product is added to
//             A, one lane per pair of columns, keypoint after keypoint in ascending order.
//   factor    root-free Cholesky (L D L^T) in place without pivoting, right-looking, one lane per column; the lanes walk the rows
//             in lockstep, so A[i][c] is a broadcast and A[i][j] is conflict-free.  Row 75 rides along: the forward substitution
//             is part of the factorisation.  One barrier per column.
//   solve     backward substitution, right-looking, the running sum in the lane's register; one barrier per column.
//   trial     R_j exp(d_j), one lane per joint, into the other of two point buffers; evaluate; accept = flip the buffers.
// Every value is a function of its own row alone and of no lane count: the bits do not depend on the other rows or on the grid.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "rotation_fit.h"

#include <cstdint>

namespace {

constexpr int NJ = 24;
constexpr int NU = 75;                                                // unknowns
constexpr int NR = NU + 1;                                            // rows of the packed triangle: the right-hand side is row 75
constexpr int TRI = NR * (NR + 1) / 2;                                // 2926 doubles
constexpr int MAXK = KP_REFIT_MAX_KP;
constexpr int MAXC = 72;                                              // columns of a keypoint's Jacobian: 3 x ancestors + 3; any tree of 24
                                                                      // joints has at most 23 (a chain), SMPL at most 7 (24 columns)
constexpr double RF_MU0 = 1e-3, RF_MU_MIN = 1e-12, RF_MU_MAX = 1e12;
constexpr double RF_SMALL = 1e-8;

// one evaluated point: what the Jacobian and the accept test need
struct Point {
  double R[NJ][9], G[NJ][9], p[NJ][3], q[NJ][3], r[MAXK][2], s[MAXK], x[3], F;
};

struct Shared {
  double A[TRI];
  Point pt[2];
  double Rn[NJ][9], jr[NJ][3], w[NJ], c[MAXK], kp[MAXK][2], dg[NU], xs[NU];
  double Jc[2][2][MAXC];
  int col[2][MAXC];
};
static_assert(sizeof(Shared) <= 48 * 1024, "kp_refit: the block's LDS");

struct RefitDev {
  const float *pose, *u, *jrest, *kp, *cam, *norm;
  float *pose_out, *cam_out, *shift, *cost;
  int* info;
  int N, K, min_kp, iters, levels;
  double lam, u_ref, rho, cam_prior, conf_thresh;
  signed char kp_joint[MAXK], parent[NJ], depth[NJ], nanc[NJ], anc[NJ][NJ - 1];    // anc: proper ancestors, ascending
};

__device__ __forceinline__ void mat3(const double* a, const double* b, double* c) {          // c = a b
  #pragma clang fp contract(off)
  #pragma unroll
  for (int r = 0; r < 3; ++r)
    #pragma unroll
    for (int k = 0; k < 3; ++k) c[r * 3 + k] = (a[r * 3] * b[k] + a[r * 3 + 1] * b[3 + k]) + a[r * 3 + 2] * b[6 + k];
}

__device__ __forceinline__ void mat3_tn(const double* a, const double* b, double* c) {       // c = a^T b
  #pragma clang fp contract(off)
  #pragma unroll
  for (int r = 0; r < 3; ++r)
    #pragma unroll
    for (int k = 0; k < 3; ++k) c[r * 3 + k] = (a[r] * b[k] + a[3 + r] * b[3 + k]) + a[6 + r] * b[6 + k];
}

// the rotation vector of Q: half the skew part scaled by angle / |half skew|; below 1e-8 the half skew part itself
__device__ __forceinline__ void log_so3(const double* Q, double* v) {
  #pragma clang fp contract(off)
  const double sx = 0.5 * (Q[7] - Q[5]), sy = 0.5 * (Q[2] - Q[6]), sz = 0.5 * (Q[3] - Q[1]);
  const double sn = sqrt((sx * sx + sy * sy) + sz * sz), cs = 0.5 * (((Q[0] + Q[4]) + Q[8]) - 1.0);
  const double f = sn < RF_SMALL ? 1.0 : atan2(sn, cs) / sn;
  v[0] = sx * f; v[1] = sy * f; v[2] = sz * f;
}

// Rodrigues: I + a K + b K^2
__device__ __forceinline__ void exp_so3(const double* d, double* E) {
  #pragma clang fp contract(off)
  const double t2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], t = sqrt(t2);
  double a, b;
  if (t < RF_SMALL) {
    a = 1.0 - t2 / 6.0;
    b = 0.5 - t2 / 24.0;
  } else {
    a = sin(t) / t;
    b = (1.0 - cos(t)) / t2;
  }
  const double x = d[0], y = d[1], z = d[2];
  // K^2 = d d^T - t2 I
  E[0] = 1.0 + b * (x * x - t2); E[1] = -a * z + b * (x * y);    E[2] = a * y + b * (x * z);
  E[3] = a * z + b * (x * y);    E[4] = 1.0 + b * (y * y - t2);  E[5] = -a * x + b * (y * z);
  E[6] = -a * y + b * (x * z);   E[7] = a * x + b * (y * z);     E[8] = 1.0 + b * (z * z - t2);
}

__device__ __forceinline__ double gm(double s, double rho) {
  #pragma clang fp contract(off)
  if (!(rho > 0.0)) return s;
  const double r2 = rho * rho;
  return r2 * s / (r2 + s);
}

// Fills P.q, P.G, P.p, P.r, P.s and P.F from P.R and P.x.  Called by the whole block; ends with a barrier.
__device__ void evaluate(const RefitDev& d, Shared& S, Point& P, double a0, double tx0, double ty0, double px, double py, double norm) {
  #pragma clang fp contract(off)
  const int tid = threadIdx.x;
  if (tid < NJ) {
    double Q[9];
    mat3_tn(S.Rn[tid], P.R[tid], Q);
    log_so3(Q, P.q[tid]);
  }
  if (tid == 0) {
    #pragma unroll
    for (int i = 0; i < 9; ++i) P.G[0][i] = P.R[0][i];
    #pragma unroll
    for (int i = 0; i < 3; ++i) P.p[0][i] = S.jr[0][i];
  }
  for (int lvl = 1; lvl <= d.levels; ++lvl) {
    __syncthreads();
    if (tid < NJ && d.depth[tid] == lvl) {
      const int pa = d.parent[tid];
      mat3(P.G[pa], P.R[tid], P.G[tid]);
      const double v0 = S.jr[tid][0] - S.jr[pa][0], v1 = S.jr[tid][1] - S.jr[pa][1], v2 = S.jr[tid][2] - S.jr[pa][2];
      const double* g = P.G[pa];
      #pragma unroll
      for (int r = 0; r < 3; ++r) P.p[tid][r] = P.p[pa][r] + ((g[r * 3] * v0 + g[r * 3 + 1] * v1) + g[r * 3 + 2] * v2);
    }
  }
  __syncthreads();
  const double a = a0 * exp(P.x[0]), tx = tx0 + P.x[1], ty = ty0 + P.x[2];
  if (tid < d.K) {
    double r0 = 0.0, r1 = 0.0, s = 0.0;
    const double c = S.c[tid];
    if (c != 0.0) {
      const double* pk = P.p[d.kp_joint[tid]];
      r0 = ((a * (pk[0] + tx) + px) - S.kp[tid][0]) / norm;
      r1 = ((a * (pk[1] + ty) + py) - S.kp[tid][1]) / norm;
      s = c * (r0 * r0 + r1 * r1);
    }
    P.r[tid][0] = r0; P.r[tid][1] = r1; P.s[tid] = s;
  }
  __syncthreads();
  double F = 0.0;
  for (int k = 0; k < d.K; ++k)
    if (S.c[k] != 0.0) F = F + gm(P.s[k], d.rho);
  for (int j = 0; j < NJ; ++j) F = F + S.w[j] * ((P.q[j][0] * P.q[j][0] + P.q[j][1] * P.q[j][1]) + P.q[j][2] * P.q[j][2]);
  F = F + d.cam_prior * ((P.x[0] * P.x[0] + P.x[1] * P.x[1]) + P.x[2] * P.x[2]);
  __syncthreads();                                                    // every lane has read P before lane 0 writes F into it
  if (tid == 0) P.F = F;
  __syncthreads();
}

__global__ __launch_bounds__(KP_REFIT_THREADS) void kp_refit_rows(RefitDev d) {
  #pragma clang fp contract(off)
  __shared__ Shared S;
  const int tid = threadIdx.x;
  for (int row = blockIdx.x; row < d.N; row += gridDim.x) {           // block-uniform: every thread reaches every barrier
    const float* pose = d.pose + (size_t)row * NJ * 9;
    const float* kpr = d.kp + (size_t)row * d.K * 3;
    const float* camr = d.cam + (size_t)row * 5;
    __syncthreads();                                                  // the previous row's reads of S are over
    // ---- load, and look for what cannot be fitted ------------------------------------------------------------------------------
    int bad = 0;
    auto finite = [](float v) { return fabsf(v) <= 3.402823466e+38f; };
    for (int i = tid; i < NJ * 9; i += KP_REFIT_THREADS) {
      const float v = pose[i];
      bad |= !finite(v);
      (&S.Rn[0][0])[i] = (double)v;
      (&S.pt[0].R[0][0])[i] = (double)v;
    }
    for (int i = tid; i < NJ * 3; i += KP_REFIT_THREADS) {
      const float v = d.jrest[(size_t)row * NJ * 3 + i];
      bad |= !finite(v);
      (&S.jr[0][0])[i] = (double)v;
    }
    int counts = 0;
    if (tid < d.K) {
      const float x = kpr[tid * 3], y = kpr[tid * 3 + 1], cf = kpr[tid * 3 + 2];
      bad |= !finite(x) || !finite(y) || !finite(cf);
      S.kp[tid][0] = (double)x;
      S.kp[tid][1] = (double)y;
      const double c = d.kp_joint[tid] >= 0 && (double)cf > d.conf_thresh ? (double)cf : 0.0;
      S.c[tid] = c;
      counts = c != 0.0;
    }
    if (tid < NJ) S.w[tid] = d.lam * uncert_weight(d.u[(size_t)row * NJ + tid], d.u_ref);
    const float a0f = camr[0], tx0f = camr[1], ty0f = camr[2], pxf = camr[3], pyf = camr[4], normf = d.norm[row];
    bad |= !finite(a0f) || !finite(tx0f) || !finite(ty0f) || !finite(pxf) || !finite(pyf) || !finite(normf) || !(normf > 0.f);
    if (tid < 3) S.pt[0].x[tid] = 0.0;
    const int any_bad = __syncthreads_or(bad);
    const int nkp = __syncthreads_count(counts);
    float* pose_out = d.pose_out + (size_t)row * NJ * 9;
    if (any_bad || nkp < d.min_kp) {                                  // copied through bit for bit
      for (int i = tid; i < NJ * 9; i += KP_REFIT_THREADS)
        reinterpret_cast<uint32_t*>(pose_out)[i] = reinterpret_cast<const uint32_t*>(pose)[i];
      if (tid < 3) reinterpret_cast<uint32_t*>(d.cam_out)[(size_t)row * 3 + tid] = reinterpret_cast<const uint32_t*>(camr)[tid];
      if (tid < NJ) d.shift[(size_t)row * NJ + tid] = 0.f;
      if (tid < 2) {
        d.cost[(size_t)row * 2 + tid] = 0.f;
        d.info[(size_t)row * 2 + tid] = tid == 0 ? 0 : (any_bad ? 2 : 1);
      }
      continue;
    }
    const double a0 = (double)a0f, tx0 = (double)tx0f, ty0 = (double)ty0f, px = (double)pxf, py = (double)pyf, norm = (double)normf;
    int cur = 0, accepted = 0;
    double mu = RF_MU0;
    evaluate(d, S, S.pt[0], a0, tx0, ty0, px, py, norm);
    const double F0 = S.pt[0].F;
    for (int it = 0; it < d.iters; ++it) {
      Point& P = S.pt[cur];
      Point& T = S.pt[cur ^ 1];
      // ---- the normal matrix and the right-hand side ------------------------------------------------------------------------------
      for (int e = tid; e < TRI; e += KP_REFIT_THREADS) S.A[e] = 0.0;
      __syncthreads();                                                // row 75 is zeroed by one lane and used by another
      const double a = a0 * exp(P.x[0]), tx = tx0 + P.x[1], ty = ty0 + P.x[2], f = a / norm;
      int buf = 0;
      for (int k = 0; k < d.K; ++k) {
        const double ck = S.c[k];
        if (ck == 0.0) continue;                                      // block-uniform
        const int jk = d.kp_joint[k], na = d.nanc[jk], nc = 3 * na + 3;
        double irls = ck;
        if (d.rho > 0.0) {
          const double r2 = d.rho * d.rho, h = r2 / (r2 + P.s[k]);
          irls = ck * (h * h);
        }
        const double sw = sqrt(irls);
        if (tid < nc) {
          double j0, j1;
          int column;
          if (tid < 3 * na) {
            const int j = d.anc[jk][tid / 3], x = tid % 3;
            const double g0 = P.G[j][x], g1 = P.G[j][3 + x], g2 = P.G[j][6 + x];
            const double v0 = P.p[jk][0] - P.p[j][0], v1 = P.p[jk][1] - P.p[j][1], v2 = P.p[jk][2] - P.p[j][2];
            j0 = f * (g1 * v2 - g2 * v1);                             // rows 0 and 1 of -[v]x G_j, column x: G_j[:,x] x v
            j1 = f * (g2 * v0 - g0 * v2);
            column = 3 * j + x;
          } else {
            const int x = tid - 3 * na;
            j0 = x == 0 ? a * (P.p[jk][0] + tx) / norm : (x == 1 ? f : 0.0);
            j1 = x == 0 ? a * (P.p[jk][1] + ty) / norm : (x == 2 ? f : 0.0);
            column = 72 + x;
          }
          j0 = j0 * sw;
          j1 = j1 * sw;
          S.Jc[buf][0][tid] = j0;
          S.Jc[buf][1][tid] = j1;
          S.col[buf][tid] = column;
          // the right-hand side -g rides in row 75; a column has one lane per keypoint, and keypoints are a barrier apart
          S.A[tri(NU, column)] = S.A[tri(NU, column)] - (j0 * (P.r[k][0] * sw) + j1 * (P.r[k][1] * sw));
        }
        __syncthreads();
        for (int e = tid; e < nc * nc; e += KP_REFIT_THREADS) {
          const int ci = e / nc, cj = e % nc;
          if (cj > ci) continue;                                      // the columns ascend: (ci, cj) is in the lower triangle
          const int idx = tri(S.col[buf][ci], S.col[buf][cj]);
          S.A[idx] = S.A[idx] + (S.Jc[buf][0][ci] * S.Jc[buf][0][cj] + S.Jc[buf][1][ci] * S.Jc[buf][1][cj]);
        }
        buf ^= 1;
      }
      __syncthreads();
      if (tid < NU) {                                                 // priors, then mu diag(A)
        const double pw = tid < 72 ? S.w[tid / 3] : d.cam_prior;
        const double pv = tid < 72 ? P.q[tid / 3][tid % 3] : P.x[tid - 72];
        const double dgn = S.A[tri(tid, tid)] + pw;
        S.A[tri(NU, tid)] = S.A[tri(NU, tid)] - pw * pv;
        S.A[tri(tid, tid)] = dgn + mu * dgn;
      }
      // ---- L D L^T in place; row 75 is substituted forward on the way -----------------------------------------------------------------
      for (int c = 0; c < NU; ++c) {
        __syncthreads();
        if (tid > c && tid < NU) {
          const int j = tid;
          const double fj = S.A[tri(j, c)] * (1.0 / S.A[tri(c, c)]);
          for (int i = c + 1; i < NR; ++i)
            if (i >= j) S.A[tri(i, j)] = S.A[tri(i, j)] - S.A[tri(i, c)] * fj;
        }
      }
      __syncthreads();
      // ---- backward substitution: x_c = (y_c - sum_{i > c} A[i][c] x_i) / D_c --------------------------------------------------------
      double acc = tid < NU ? S.A[tri(NU, tid)] : 0.0;
      for (int c = NU - 1; c >= 0; --c) {
        if (tid == c) S.xs[c] = acc / S.A[tri(c, c)];
        __syncthreads();
        if (tid < c) acc = acc - S.A[tri(c, tid)] * S.xs[c];
      }
      // ---- the trial point ------------------------------------------------------------------------------------------------------
      if (tid < NJ) {
        double E[9];
        exp_so3(&S.xs[3 * tid], E);
        mat3(P.R[tid], E, T.R[tid]);
      }
      if (tid < 3) T.x[tid] = P.x[tid] + S.xs[72 + tid];
      __syncthreads();
      evaluate(d, S, T, a0, tx0, ty0, px, py, norm);
      if (T.F < P.F) {                                                // the same bits in every lane
        cur ^= 1;
        ++accepted;
        mu = mu / 3.0 > RF_MU_MIN ? mu / 3.0 : RF_MU_MIN;
      } else {
        mu = mu * 3.0 < RF_MU_MAX ? mu * 3.0 : RF_MU_MAX;
      }
    }
    // ---- outputs ----------------------------------------------------------------------------------------------------------------
    const Point& P = S.pt[cur];
    for (int i = tid; i < NJ * 9; i += KP_REFIT_THREADS) pose_out[i] = (float)(&P.R[0][0])[i];
    if (tid < NJ) {
      double Q[9];
      mat3_tn(S.Rn[tid], P.R[tid], Q);
      const double sx = Q[7] - Q[5], sy = Q[2] - Q[6], sz = Q[3] - Q[1];
      const double sn = 0.5 * sqrt((sx * sx + sy * sy) + sz * sz), cs = 0.5 * (((Q[0] + Q[4]) + Q[8]) - 1.0);
      d.shift[(size_t)row * NJ + tid] = (float)(atan2(sn, cs) * (180.0 / 3.14159265358979323846));
    }
    if (tid == 0) {
      d.cam_out[(size_t)row * 3] = accepted ? (float)(a0 * exp(P.x[0])) : a0f;
      d.cam_out[(size_t)row * 3 + 1] = (float)(tx0 + P.x[1]);
      d.cam_out[(size_t)row * 3 + 2] = (float)(ty0 + P.x[2]);
      d.cost[(size_t)row * 2] = (float)F0;
      d.cost[(size_t)row * 2 + 1] = (float)P.F;
      d.info[(size_t)row * 2] = accepted;
      d.info[(size_t)row * 2 + 1] = 0;
    }
  }
}

}  // namespace

void launch_kp_refit(const float* pose, const float* u, const float* jrest, const float* kp, const float* cam, const float* norm, int N,
                     int K, const int* kp_joint, const int* parents, double lam, double u_ref, double rho, double cam_prior,
                     double conf_thresh, int min_kp, int iters, float* pose_out, float* cam_out, float* shift, float* cost, int* info,
                     int max_blocks, hipStream_t s) {
  RefitDev d{};
  d.pose = pose; d.u = u; d.jrest = jrest; d.kp = kp; d.cam = cam; d.norm = norm;
  d.pose_out = pose_out; d.cam_out = cam_out; d.shift = shift; d.cost = cost; d.info = info;
  d.N = N; d.K = K; d.min_kp = min_kp; d.iters = iters;
  d.lam = lam; d.u_ref = u_ref; d.rho = rho; d.cam_prior = cam_prior; d.conf_thresh = conf_thresh;
  for (int k = 0; k < MAXK; ++k) d.kp_joint[k] = (signed char)(k < K ? kp_joint[k] : -1);
  d.levels = 0;
  for (int j = 0; j < NJ; ++j) {                                      // the caller checked: parents[j] in [0, j) for j >= 1
    d.parent[j] = (signed char)(j ? parents[j] : -1);
    d.depth[j] = (signed char)(j ? d.depth[parents[j]] + 1 : 0);
    if (d.depth[j] > d.levels) d.levels = d.depth[j];
    int chain[NJ], n = 0;
    for (int a = j ? parents[j] : -1; a >= 0; a = a ? parents[a] : -1) chain[n++] = a;
    d.nanc[j] = (signed char)n;
    for (int i = 0; i < n; ++i) d.anc[j][i] = (signed char)chain[n - 1 - i];    // parent < child: reversed = ascending
  }
  const int cap = max_blocks > 0 && max_blocks < KP_REFIT_MAX_BLOCKS ? max_blocks : KP_REFIT_MAX_BLOCKS;
  kp_refit_rows<<<N < cap ? N : cap, KP_REFIT_THREADS, 0, s>>>(d);
}
