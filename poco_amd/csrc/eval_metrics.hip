// Evaluation metrics on the device: MPJPE, PA-MPJPE, V2V, pose distance and processed uncertainty per crop, and their reduction
// to the four numbers the reference's eval.py prints.  Replaces the host loop of pocolib/core/trainer.py:298-336 (validation_step)
// and :365-391 (validation_epoch_end) with pocolib/utils/eval_utils.py:11-118,154-165, pocolib/utils/geometry.py:207-244,
// pocolib/utils/poco_utils.py:21-25,62-94 and pocolib/utils/save_results.py:71-82.  The contract (record layout, summary, argument
// rules) is stated in include/poco_hip.h and DESIGN.md "Evaluation"; tests/eval_np.py restates it in numpy.
//
// Two launches per step (per sub-batch of at most `sub` crops), both on the caller's stream:
//   eval_partial   grid (S, B), 256 threads: block (s, b) stages vertices [s * 1024, (s + 1) * 1024) of crop b - predicted and, if
//                  given, ground truth - in LDS with ONE coalesced read, sums the vertex distances of the slice (V2V) and applies
//                  the slice of the joint regressor (CSR by row, each row's entries sorted by vertex and cut at the slice borders)
//                  to both meshes from LDS.  One partial (2 x J x 3 joint sums + 1 distance sum) per block, written, not added.
//   eval_crop      grid B, one wave: adds the S partials in slice order, maps the joints, MPJPE, similarity Procrustes (Horn's
//                  quaternion form: largest eigenvector of a symmetric 4x4 by cyclic Jacobi, a FIXED number of sweeps), pose distance
//                  through the shared Rodrigues function, processed uncertainty; writes the crop's record.
// One launch at finish: eval_finish, one block, sums the records in a fixed (strided, then tree) order.
// Every sum over vertices or joints and the whole Procrustes solve are carried in fp64 (full rate on CDNA, and the step is
// latency-bound): the records are the fp32 roundings of fp64 results, so they do not depend on the slice count or the batching.
// The processed uncertainty alone is fp32, in the order of poco_amd/postproc.py, so that it equals the host's values.
// No atomics: every output word has one writer and every sum a fixed order - two runs give the same bits.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "rodrigues.h"
#include "rotation_fit.h"
#include "../../include/poco_hip.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int EV_MAXJ = POCO_EVAL_MAX_JOINTS;          // 32
constexpr int EV_REC = POCO_EVAL_RECORD_FLOATS;        // 416
constexpr int EV_CHUNK = 1024;                         // vertices per block of eval_partial (2 x 12 KB of LDS)
constexpr int EV_PART_V2V = 2 * EV_MAXJ * 3;           // partial: [pred joints 96 | gt joints 96 | distance sum | pad]
constexpr int EV_PSTRIDE = EV_PART_V2V + 2;
constexpr int EV_MAX_SUB = 256;                        // crops per launch pair (bounds the partial scratch)
constexpr int EV_FIN_THREADS = 1024;
// record offsets (include/poco_hip.h)
constexpr int R_MPJPE = 0, R_PA = 1, R_V2V = 2, R_MPJPE_J = 4, R_PA_J = 36, R_POSE = 68, R_UNC = 92, R_PRED = 116, R_GT = 212,
              R_NONREL = 308;
static_assert(R_NONREL + EV_MAXJ * 3 <= EV_REC, "record layout");

// get_smpl_skeleton() of pocolib/utils/kp_utils.py:881-908 as parent per joint
__constant__ int EV_SMPL_PARENT[24] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};

__global__ __launch_bounds__(256) void rodrigues_kernel(const float* __restrict__ aa, float* __restrict__ rot, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  double R[9];
  rodrigues_f64(aa + (size_t)i * 3, R);
  #pragma unroll
  for (int k = 0; k < 9; ++k) rot[(size_t)i * 9 + k] = (float)R[k];
}

__device__ __forceinline__ double wave_sum(double v) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct EvalDev {
  int J, V, S, M, pelvis, nsel, kinematic;
  const int* off;      // [J * S + 1]: entries of row j inside slice s are [off[j * S + s], off[j * S + s + 1])
  const int* col;      // vertex of each entry
  const float* w;      // its weight
  const int* map;      // [M]
  const int* sel;      // [nsel]
  double* part;        // [sub][S][EV_PSTRIDE]
  float* rec;          // [capacity][EV_REC]
};

// pred / gt: the sub-batch's first crop.  gt may be null (joint ground truth): its sums are then not computed.
__global__ __launch_bounds__(256) void eval_partial(EvalDev d, const float* __restrict__ pred, const float* __restrict__ gt) {
  __shared__ float sp[EV_CHUNK * 3];
  __shared__ float sg[EV_CHUNK * 3];
  __shared__ double wred[4];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int v0 = s * EV_CHUNK;
  const int n = min(EV_CHUNK, d.V - v0);
  const size_t base = ((size_t)b * d.V + v0) * 3;
  for (int i = tid; i < n * 3; i += 256) {
    sp[i] = pred[base + i];
    if (gt) sg[i] = gt[base + i];
  }
  __syncthreads();
  double* out = d.part + ((size_t)b * d.S + s) * EV_PSTRIDE;
  // V2V (eval_utils.py:104-118): the slice's sum of vertex distances
  double dist = 0.0;
  if (gt) {
    for (int v = tid; v < n; v += 256) {
      const double dx = (double)sg[3 * v] - (double)sp[3 * v], dy = (double)sg[3 * v + 1] - (double)sp[3 * v + 1],
                   dz = (double)sg[3 * v + 2] - (double)sp[3 * v + 2];
      dist += sqrt(dx * dx + dy * dy + dz * dz);
    }
    dist = wave_sum(dist);
  }
  if (lane == 0) wred[wv] = dist;
  // J_regressor @ vertices (eval_utils.py:66-69, base_dataset.py:359-360), this slice's share, rows dealt to the four waves
  for (int j = wv; j < d.J; j += 4) {
    const int k0 = d.off[j * d.S + s], k1 = d.off[j * d.S + s + 1];
    double px = 0, py = 0, pz = 0, gx = 0, gy = 0, gz = 0;
    for (int k = k0 + lane; k < k1; k += 64) {
      const int c = d.col[k] - v0;
      const double wt = d.w[k];
      px += wt * sp[3 * c]; py += wt * sp[3 * c + 1]; pz += wt * sp[3 * c + 2];
      if (gt) { gx += wt * sg[3 * c]; gy += wt * sg[3 * c + 1]; gz += wt * sg[3 * c + 2]; }
    }
    px = wave_sum(px); py = wave_sum(py); pz = wave_sum(pz);
    gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
    if (lane == 0) {
      out[j * 3] = px; out[j * 3 + 1] = py; out[j * 3 + 2] = pz;
      out[EV_MAXJ * 3 + j * 3] = gx; out[EV_MAXJ * 3 + j * 3 + 1] = gy; out[EV_MAXJ * 3 + j * 3 + 2] = gz;
    }
  }
  __syncthreads();
  if (tid == 0) out[EV_PART_V2V] = (wred[0] + wred[1]) + (wred[2] + wred[3]);
}

// jacobi_rotate of rotation_fit.h with the file's default contraction: eval_crop is one latency-bound wave per crop, and the
// shared, uncontracted solve measured 3 us (5 %) slower per step.  Its multiply-adds fuse, so the last bits differ from the header's.
__device__ __forceinline__ void jacobi_rotate_fused(double (&a)[4][4], double (&v)[4][4], int p, int q) {
  const double apq = a[p][q];
  if (!(apq != 0.0)) return;                       // zero (or NaN: nothing to gain): a branch, not a loop
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  #pragma unroll
  for (int k = 0; k < 4; ++k) {                    // A <- A G
    const double akp = a[k][p], akq = a[k][q];
    a[k][p] = c * akp - s * akq;
    a[k][q] = s * akp + c * akq;
  }
  #pragma unroll
  for (int k = 0; k < 4; ++k) {                    // A <- G^T A
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

// b0: first crop of this sub-batch inside the step; first: record index of the step's first crop.
__global__ __launch_bounds__(64) void eval_crop(EvalDev d, int b0, long long first, int has_gt_verts, const float* __restrict__ gt_joints,
                                                const float* __restrict__ pred_pose, const float* __restrict__ gt_pose,
                                                const float* __restrict__ var_pose, int t1, int t2) {
  __shared__ double jp[EV_MAXJ][3], jg[EV_MAXJ][3], x1[EV_MAXJ][3], x2[EV_MAXJ][3];
  __shared__ double e1[EV_MAXJ], e2[EV_MAXJ];
  __shared__ float unc[24];
  const int b = blockIdx.x, t = threadIdx.x;
  const long long gb = (long long)b0 + b;
  float* rec = d.rec + (size_t)(first + gb) * EV_REC;
  const double* part = d.part + (size_t)b * d.S * EV_PSTRIDE;
  const int J = d.J, M = d.M;
  // the S partials in slice order
  for (int idx = t; idx < 2 * EV_MAXJ * 3; idx += 64) {
    const int which = idx / (EV_MAXJ * 3), r = idx % (EV_MAXJ * 3), j = r / 3, c = r % 3;
    double acc = 0.0;
    if (j < J && (which == 0 || has_gt_verts))
      for (int s = 0; s < d.S; ++s) acc += part[(size_t)s * EV_PSTRIDE + idx];
    (which ? jg : jp)[j][c] = acc;
  }
  if (t == 0) {
    double acc = 0.0;
    if (has_gt_verts)
      for (int s = 0; s < d.S; ++s) acc += part[(size_t)s * EV_PSTRIDE + EV_PART_V2V];
    rec[R_V2V] = has_gt_verts ? (float)(acc / (double)d.V) : 0.f;
    rec[3] = 0.f;
  }
  __syncthreads();
  // joint map + pelvis (eval_utils.py:70-73, base_dataset.py:361-365), MPJPE per joint (eval_utils.py:99-102)
  if (t < EV_MAXJ) {
    double err = 0.0;
    #pragma unroll
    for (int c = 0; c < 3; ++c) {
      double a = 0.0, g = 0.0, nr = 0.0;
      if (t < M) {
        nr = jp[d.map[t]][c];
        a = nr - jp[d.pelvis][c];
        g = has_gt_verts ? jg[d.map[t]][c] - jg[d.pelvis][c] : (double)gt_joints[((size_t)gb * M + t) * 3 + c];
      }
      x1[t][c] = a; x2[t][c] = g;
      rec[R_PRED + t * 3 + c] = (float)a;
      rec[R_GT + t * 3 + c] = (float)g;
      rec[R_NONREL + t * 3 + c] = (float)nr;
      err += (a - g) * (a - g);
    }
    e1[t] = sqrt(err);
    rec[R_MPJPE_J + t] = (float)e1[t];
  }
  __syncthreads();
  // similarity Procrustes of x1 onto x2 (eval_utils.py:11-59), every lane the same arithmetic
  double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
  for (int m = 0; m < M; ++m)
    #pragma unroll
    for (int c = 0; c < 3; ++c) { mu1[c] += x1[m][c]; mu2[c] += x2[m][c]; }
  #pragma unroll
  for (int c = 0; c < 3; ++c) { mu1[c] /= (double)M; mu2[c] /= (double)M; }
  double var1 = 0.0, K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int m = 0; m < M; ++m) {
    double a[3], g[3];
    #pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = x1[m][c] - mu1[c]; g[c] = x2[m][c] - mu2[c]; var1 += a[c] * a[c]; }
    #pragma unroll
    for (int r = 0; r < 3; ++r)
      #pragma unroll
      for (int c = 0; c < 3; ++c) K[r][c] += a[r] * g[c];            // K = X1 X2^T
  }
  // argmax over SO(3) of tr(R K) = the unit quaternion that maximises q^T N q (Horn 1987); the reference's U, V and Z sign fix
  // (eval_utils.py:39-45) select the same rotation
  double N[4][4], E[4][4];
  horn_matrix(K, N);
  #pragma unroll
  for (int r = 0; r < 4; ++r)
    #pragma unroll
    for (int c = 0; c < 4; ++c) E[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < ROT_JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate_fused(N, E, 0, 1); jacobi_rotate_fused(N, E, 0, 2); jacobi_rotate_fused(N, E, 0, 3);
    jacobi_rotate_fused(N, E, 1, 2); jacobi_rotate_fused(N, E, 1, 3); jacobi_rotate_fused(N, E, 2, 3);
  }
  double qw = E[0][0], qx = E[1][0], qy = E[2][0], qz = E[3][0], best = N[0][0];
  #pragma unroll
  for (int k = 1; k < 4; ++k)
    if (N[k][k] > best) { best = N[k][k]; qw = E[0][k]; qx = E[1][k]; qy = E[2][k]; qz = E[3][k]; }
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= qn; qx /= qn; qy /= qn; qz /= qn;
  double R[3][3];
  R[0][0] = qw * qw + qx * qx - qy * qy - qz * qz; R[0][1] = 2 * (qx * qy - qw * qz); R[0][2] = 2 * (qx * qz + qw * qy);
  R[1][0] = 2 * (qx * qy + qw * qz); R[1][1] = qw * qw - qx * qx + qy * qy - qz * qz; R[1][2] = 2 * (qy * qz - qw * qx);
  R[2][0] = 2 * (qx * qz - qw * qy); R[2][1] = 2 * (qy * qz + qw * qx); R[2][2] = qw * qw - qx * qx - qy * qy + qz * qz;
  double trace = 0.0;
  #pragma unroll
  for (int r = 0; r < 3; ++r)
    #pragma unroll
    for (int c = 0; c < 3; ++c) trace += R[r][c] * K[c][r];
  const double scale = trace / var1;                                // var1 = 0 (all predicted joints coincide): Inf / NaN, as the reference
  double tv[3];
  #pragma unroll
  for (int r = 0; r < 3; ++r) tv[r] = mu2[r] - scale * (R[r][0] * mu1[0] + R[r][1] * mu1[1] + R[r][2] * mu1[2]);
  if (t < EV_MAXJ) {
    double err = 0.0;
    if (t < M) {
      #pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double h = scale * (R[r][0] * x1[t][0] + R[r][1] * x1[t][1] + R[r][2] * x1[t][2]) + tv[r] - x2[t][r];
        err += h * h;
      }
      err = sqrt(err);
    }
    e2[t] = err;
    rec[R_PA_J + t] = (float)err;
  }
  // pose distance (eval_utils.py:154-160) and the uncertainty's trailing means (poco_utils.py:67-70)
  if (t < 24) {
    double G[9];
    rodrigues_f64(gt_pose + ((size_t)gb * 24 + t) * 3, G);
    const float* P = pred_pose + ((size_t)gb * 24 + t) * 9;
    double acc = 0.0;
    #pragma unroll
    for (int r = 0; r < 3; ++r) {
      double row = 0.0;
      #pragma unroll
      for (int c = 0; c < 3; ++c) { const double df = (double)P[3 * r + c] - G[3 * r + c]; row += df * df; }
      acc += row / 3.0;
    }
    rec[R_POSE + t] = (float)(acc / 3.0);
    const float* vp = var_pose + ((size_t)gb * 24 + t) * t1 * t2;
    float s1 = 0.f;
    for (int a = 0; a < t1; ++a) {
      float s2 = 0.f;
      for (int c = 0; c < t2; ++c) s2 += vp[a * t2 + c];
      s1 += t2 > 1 ? s2 / (float)t2 : s2;
    }
    unc[t] = t1 > 1 ? s1 / (float)t1 : s1;
  }
  __syncthreads();
  if (t == 0) {
    double a = 0.0, p = 0.0;
    for (int m = 0; m < M; ++m) { a += e1[m]; p += e2[m]; }
    rec[R_MPJPE] = (float)(a / (double)M);
    rec[R_PA] = (float)(p / (double)M);
    if (d.kinematic)
      for (int j = 1; j < 24; ++j) unc[j] += unc[EV_SMPL_PARENT[j]];    // poco_utils.py:21-25, child order
    for (int j = 0; j < 24; ++j) rec[R_UNC + j] = unc[j];
    for (int i = R_NONREL + EV_MAXJ * 3; i < EV_REC; ++i) rec[i] = 0.f;
  }
}

// summary[8] = {N, 1000 mean MPJPE, 1000 mean PA-MPJPE, 1000 mean V2V, Pearson r, number of (x, y) pairs, 0, 0}
__global__ __launch_bounds__(EV_FIN_THREADS) void eval_finish(EvalDev d, long long N, double* __restrict__ summary) {
  __shared__ double red[EV_FIN_THREADS];
  const int t = threadIdx.x;
  double a = 0, p = 0, v = 0, sx = 0, sy = 0;
  for (long long i = t; i < N; i += EV_FIN_THREADS) {
    const float* r = d.rec + (size_t)i * EV_REC;
    a += r[R_MPJPE]; p += r[R_PA]; v += r[R_V2V];
    for (int k = 0; k < d.nsel; ++k) { sx += r[R_POSE + d.sel[k]]; sy += r[R_UNC + d.sel[k]]; }
  }
  a = block_tree_sum<EV_FIN_THREADS>(a, red); p = block_tree_sum<EV_FIN_THREADS>(p, red); v = block_tree_sum<EV_FIN_THREADS>(v, red);
  sx = block_tree_sum<EV_FIN_THREADS>(sx, red); sy = block_tree_sum<EV_FIN_THREADS>(sy, red);
  const double n = (double)N, terms = n * (double)d.nsel;
  const double mx = sx / terms, my = sy / terms;
  double cxx = 0, cyy = 0, cxy = 0;
  for (long long i = t; i < N; i += EV_FIN_THREADS) {
    const float* r = d.rec + (size_t)i * EV_REC;
    for (int k = 0; k < d.nsel; ++k) {
      const double x = (double)r[R_POSE + d.sel[k]] - mx, y = (double)r[R_UNC + d.sel[k]] - my;
      cxx += x * x; cyy += y * y; cxy += x * y;
    }
  }
  cxx = block_tree_sum<EV_FIN_THREADS>(cxx, red); cyy = block_tree_sum<EV_FIN_THREADS>(cyy, red);
  cxy = block_tree_sum<EV_FIN_THREADS>(cxy, red);
  if (t == 0) {
    double r = cxy / (sqrt(cxx) * sqrt(cyy));
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                       // scipy.stats.pearsonr clips; a NaN stays a NaN
    summary[0] = n; summary[1] = 1000.0 * a / n; summary[2] = 1000.0 * p / n; summary[3] = 1000.0 * v / n;
    summary[4] = r; summary[5] = terms; summary[6] = 0.0; summary[7] = 0.0;
  }
}

// poco_evaluator_rank_inputs: keys and value planes for poco_op_rank_curve from the records, one lane per output row.
// mode 0: row = crop, key = u_i as eval_uncert_summary_kernel forms it, planes MPJPE | PA-MPJPE | V2V.
// mode 1: row = crop * nsel + k, key = the processed uncertainty, plane = the pose distance of selected joint k.
__global__ __launch_bounds__(256) void eval_rank_inputs(EvalDev d, int mode, long long rows, float* __restrict__ key, float* __restrict__ vals) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  if (mode == 0) {
    const float* r = d.rec + (size_t)i * EV_REC;
    double m = 0.0;
    for (int j = 0; j < 24; ++j) m += (double)r[R_UNC + j];
    m /= 24.0;
    key[i] = (float)m;
    vals[i] = r[R_MPJPE]; vals[rows + i] = r[R_PA]; vals[2 * rows + i] = r[R_V2V];
  } else {
    const long long crop = i / d.nsel;
    const int j = d.sel[(int)(i % d.nsel)];
    const float* r = d.rec + (size_t)crop * EV_REC;
    key[i] = r[R_UNC + j];
    vals[i] = r[R_POSE + j];
  }
}

// poco_evaluator_copy_records: record order[i] (or i) -> row i of out, 16 bytes per lane; an entry outside [0, have) gives zeros
__global__ __launch_bounds__(256) void eval_copy_records(const float* __restrict__ rec, const int* __restrict__ order, long long n,
                                                         long long have, float* __restrict__ out) {
  constexpr int Q = EV_REC / 4;                                       // float4 words of a record
  static_assert(EV_REC % 4 == 0, "a record is a whole number of 16-byte words");
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * Q) return;
  const long long row = i / Q;
  const int q = (int)(i - row * Q);
  const long long src = order ? (long long)order[row] : row;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (src >= 0 && src < have) v = reinterpret_cast<const float4*>(rec + (size_t)src * EV_REC)[q];
  reinterpret_cast<float4*>(out + (size_t)row * EV_REC)[q] = v;
}

}  // namespace

extern "C" int poco_op_rodrigues(const float* d_axis_angle, float* d_rotmat, int N, void* stream) {
  if (!d_axis_angle || !d_rotmat || N < 1) { poco_set_error("rodrigues: bad argument"); return POCO_ERR_ARG; }
  rodrigues_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_axis_angle, d_rotmat, N);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

// ---- evaluator ------------------------------------------------------------------------------------------------------------
struct poco_evaluator {
  int J = 0, V = 0, S = 0, M = 0, pelvis = 0, kinematic = 1, sub = 1;
  long long capacity = 0, first = 0;
  std::vector<int> off, col, map, sel;     // host copies, uploaded by the first step
  std::vector<float> w;
  bool on_device = false;
  int *d_off = nullptr, *d_col = nullptr, *d_map = nullptr, *d_sel = nullptr;
  float *d_w = nullptr, *d_rec = nullptr;
  double *d_part = nullptr, *d_summary = nullptr;
  ~poco_evaluator() {
    for (void* p : {(void*)d_off, (void*)d_col, (void*)d_map, (void*)d_sel, (void*)d_w, (void*)d_rec, (void*)d_part, (void*)d_summary})
      if (p) (void)hipFree(p);
  }
  EvalDev dev() const {
    return EvalDev{J, V, S, M, pelvis, (int)sel.size(), kinematic, d_off, d_col, d_w, d_map, d_sel, d_part, d_rec};
  }
};

static constexpr int EVAL_MAX_VERTS = 1 << 22;
static constexpr long long EVAL_MAX_CAPACITY = 1ll << 24;

extern "C" int poco_evaluator_create(const float* h_J_regressor, int J, int V, const int32_t* h_joint_map, int M, int pelvis,
                                     const int32_t* h_sel_uncert, int num_sel, int kinematic, int64_t capacity,
                                     poco_evaluator_t* out) {
  if (!out) { poco_set_error("poco_evaluator_create: null handle pointer"); return POCO_ERR_ARG; }
  *out = nullptr;
  if (!h_J_regressor || !h_joint_map || J < 1 || J > EV_MAXJ || V < 1 || V > EVAL_MAX_VERTS || M < 1 || M > J || pelvis < 0 ||
      pelvis >= J || num_sel < 0 || num_sel > 24 || (num_sel > 0 && !h_sel_uncert) || capacity < 1 || capacity > EVAL_MAX_CAPACITY) {
    poco_set_error("poco_evaluator_create: bad arguments (need a regressor and a joint map, 1 <= M <= J <= 32, 1 <= V <= 2^22, "
                   "0 <= pelvis < J, at most 24 selected joints, 1 <= capacity <= 2^24)");
    return POCO_ERR_ARG;
  }
  for (int m = 0; m < M; ++m)
    if (h_joint_map[m] < 0 || h_joint_map[m] >= J) {
      poco_set_error("poco_evaluator_create: joint map entry " + std::to_string(m) + " = " + std::to_string(h_joint_map[m]) +
                     " outside [0, " + std::to_string(J) + ")");
      return POCO_ERR_ARG;
    }
  for (int k = 0; k < num_sel; ++k)
    if (h_sel_uncert[k] < 0 || h_sel_uncert[k] >= 24) {
      poco_set_error("poco_evaluator_create: selected joint " + std::to_string(h_sel_uncert[k]) + " outside [0, 24)");
      return POCO_ERR_ARG;
    }
  auto* e = new poco_evaluator;
  e->J = J; e->V = V; e->M = M; e->pelvis = pelvis; e->kinematic = kinematic ? 1 : 0; e->capacity = capacity;
  e->S = (V + EV_CHUNK - 1) / EV_CHUNK;
  e->sub = std::max(1, std::min(EV_MAX_SUB, 4096 / e->S));
  e->map.assign(h_joint_map, h_joint_map + M);
  if (num_sel > 0) e->sel.assign(h_sel_uncert, h_sel_uncert + num_sel);
  else for (int k = 0; k < 24; ++k) e->sel.push_back(k);              // default: all 24 (EXCLUDE_UNCERT_IDX = "")
  // CSR by row without the zeros; a row's entries ascend by vertex, so each slice owns one contiguous run of them
  e->off.assign((size_t)J * e->S + 1, 0);
  for (int j = 0; j < J; ++j)
    for (int s = 0; s < e->S; ++s) {
      e->off[(size_t)j * e->S + s] = (int)e->col.size();
      const int v1 = std::min(V, (s + 1) * EV_CHUNK);
      for (int v = s * EV_CHUNK; v < v1; ++v) {
        const float x = h_J_regressor[(size_t)j * V + v];
        if (x != 0.f) { e->col.push_back(v); e->w.push_back(x); }
      }
    }
  e->off.back() = (int)e->col.size();
  *out = e;
  return POCO_OK;
}

static int evaluator_upload(poco_evaluator* e) {
  if (e->on_device) return POCO_OK;
  auto up = [](auto** d, const auto& h) -> hipError_t {
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(h[0]);
    hipError_t err = hipMalloc(d, bytes);
    if (err != hipSuccess || h.empty()) return err;
    return hipMemcpy(*d, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice);
  };
  POCO_HIP_CHECK(up(&e->d_off, e->off));
  POCO_HIP_CHECK(up(&e->d_col, e->col));
  POCO_HIP_CHECK(up(&e->d_w, e->w));
  POCO_HIP_CHECK(up(&e->d_map, e->map));
  POCO_HIP_CHECK(up(&e->d_sel, e->sel));
  POCO_HIP_CHECK(hipMalloc(&e->d_part, (size_t)e->sub * e->S * EV_PSTRIDE * sizeof(double)));
  POCO_HIP_CHECK(hipMalloc(&e->d_summary, (8 + 2) * sizeof(double)));   // [8..10): poco_evaluator_uncert_summary
  POCO_HIP_CHECK(hipMalloc(&e->d_rec, (size_t)e->capacity * EV_REC * sizeof(float)));
  e->on_device = true;
  return POCO_OK;
}

extern "C" int poco_evaluator_step(poco_evaluator_t e, int B, const float* d_pred_vertices, const float* d_gt_vertices,
                                   const float* d_gt_joints, const float* d_pred_pose, const float* d_gt_pose,
                                   const float* d_var_pose, int var_t1, int var_t2, void* stream) {
  if (!e || B <= 0 || !d_pred_vertices || !d_pred_pose || !d_gt_pose || !d_var_pose || var_t1 < 1 || var_t2 < 1 ||
      var_t1 > 4096 || var_t2 > 4096) {
    poco_set_error("poco_evaluator_step: bad arguments (need a handle, B >= 1, predicted vertices, both poses, var_pose and "
                   "trailing extents in 1..4096)");
    return POCO_ERR_ARG;
  }
  if ((d_gt_vertices != nullptr) == (d_gt_joints != nullptr)) {
    poco_set_error("poco_evaluator_step: exactly one of gt_vertices and gt_joints must be given");
    return POCO_ERR_ARG;
  }
  if (e->first + B > e->capacity) {
    poco_set_error("poco_evaluator_step: " + std::to_string(e->first) + " + " + std::to_string(B) + " crops exceed the capacity of " +
                   std::to_string(e->capacity));
    return POCO_ERR_ARG;
  }
  if (int rc = evaluator_upload(e)) return rc;
  const hipStream_t s = (hipStream_t)stream;
  const EvalDev d = e->dev();
  for (int b0 = 0; b0 < B; b0 += e->sub) {          // the partial scratch is reused in stream order
    const int nb = std::min(e->sub, B - b0);
    const size_t vo = (size_t)b0 * e->V * 3;
    eval_partial<<<dim3(e->S, nb), 256, 0, s>>>(d, d_pred_vertices + vo, d_gt_vertices ? d_gt_vertices + vo : nullptr);
    eval_crop<<<nb, 64, 0, s>>>(d, b0, e->first, d_gt_vertices ? 1 : 0, d_gt_joints, d_pred_pose, d_gt_pose, d_var_pose, var_t1,
                                var_t2);
  }
  POCO_HIP_CHECK(hipGetLastError());
  e->first += B;
  return POCO_OK;
}

extern "C" int poco_evaluator_finish(poco_evaluator_t e, double* h_summary8, float* h_records, int64_t records_cap, void* stream) {
  if (!e || !h_summary8 || (h_records && records_cap < e->first)) {
    poco_set_error("poco_evaluator_finish: bad arguments (need a handle, a summary of 8 doubles and, if records are wanted, room "
                   "for all of them)");
    return POCO_ERR_ARG;
  }
  if (e->first < 1) { poco_set_error("poco_evaluator_finish: no crop has been stepped"); return POCO_ERR_STATE; }
  if (int rc = evaluator_upload(e)) return rc;
  const hipStream_t s = (hipStream_t)stream;
  eval_finish<<<1, EV_FIN_THREADS, 0, s>>>(e->dev(), e->first, e->d_summary);
  POCO_HIP_CHECK(hipGetLastError());
  POCO_HIP_CHECK(hipMemcpyAsync(h_summary8, e->d_summary, 8 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (h_records)
    POCO_HIP_CHECK(hipMemcpyAsync(h_records, e->d_rec, (size_t)e->first * EV_REC * sizeof(float), hipMemcpyDeviceToHost, s));
  POCO_HIP_CHECK(hipStreamSynchronize(s));
  return POCO_OK;
}

// Var-MPJPE and Variance (trainer.py:374,377-378; kernel in eval_likelihood.hip): a second reduction over the same records, which it only reads
extern "C" int poco_evaluator_uncert_summary(poco_evaluator_t e, double* h_summary2, void* stream) {
  if (!e || !h_summary2) { poco_set_error("poco_evaluator_uncert_summary: bad arguments (need a handle and a summary of 2 doubles)"); return POCO_ERR_ARG; }
  if (e->first < 1) { poco_set_error("poco_evaluator_uncert_summary: no crop has been stepped"); return POCO_ERR_STATE; }
  if (int rc = evaluator_upload(e)) return rc;
  const hipStream_t s = (hipStream_t)stream;
  launch_eval_uncert_summary(e->d_rec, EV_REC, R_MPJPE, R_UNC, e->first, e->d_summary + 8, s);
  POCO_HIP_CHECK(hipGetLastError());
  POCO_HIP_CHECK(hipMemcpyAsync(h_summary2, e->d_summary + 8, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  POCO_HIP_CHECK(hipStreamSynchronize(s));
  return POCO_OK;
}

extern "C" int poco_evaluator_rank_inputs(poco_evaluator_t e, int mode, float* d_key, float* d_vals, int64_t cap, int64_t* h_n, int* h_E,
                                          void* stream) {
  if (!e || !d_key || !d_vals || !h_n || !h_E || (mode | 1) != 1) {
    poco_set_error("poco_evaluator_rank_inputs: bad arguments (need a handle, key, vals, n and E, and mode 0 or 1)");
    return POCO_ERR_ARG;
  }
  if (e->first < 1) { poco_set_error("poco_evaluator_rank_inputs: no crop has been stepped"); return POCO_ERR_STATE; }
  const long long rows = mode == 0 ? e->first : e->first * (long long)e->sel.size();
  *h_n = rows;
  *h_E = mode == 0 ? 3 : 1;
  if (cap < rows) {
    poco_set_error("poco_evaluator_rank_inputs: " + std::to_string(rows) + " rows do not fit a capacity of " + std::to_string(cap));
    return POCO_ERR_ARG;
  }
  if (int rc = evaluator_upload(e)) return rc;
  eval_rank_inputs<<<(unsigned)((rows + 255) / 256), 256, 0, (hipStream_t)stream>>>(e->dev(), mode, rows, d_key, d_vals);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_evaluator_copy_records(poco_evaluator_t e, const int32_t* d_order, int64_t n, float* d_out, void* stream) {
  if (!e || !d_out || n < 1 || ((uintptr_t)d_out & 15) != 0 || n > (1ll << 24)) {
    poco_set_error("poco_evaluator_copy_records: bad arguments (need a handle, a 16-byte aligned output and 1 <= n <= 2^24)");
    return POCO_ERR_ARG;
  }
  if (e->first < 1) { poco_set_error("poco_evaluator_copy_records: no crop has been stepped"); return POCO_ERR_STATE; }
  if (!d_order && n > e->first) {
    poco_set_error("poco_evaluator_copy_records: " + std::to_string(n) + " rows asked for, " + std::to_string(e->first) + " written");
    return POCO_ERR_ARG;
  }
  if (int rc = evaluator_upload(e)) return rc;
  const long long words = (long long)n * (EV_REC / 4);
  eval_copy_records<<<(unsigned)((words + 255) / 256), 256, 0, (hipStream_t)stream>>>(e->d_rec, d_order, n, e->first, d_out);
  POCO_HIP_CHECK(hipGetLastError());
  return POCO_OK;
}

extern "C" int poco_evaluator_reset(poco_evaluator_t e) {
  if (!e) { poco_set_error("poco_evaluator_reset: null handle"); return POCO_ERR_ARG; }
  e->first = 0;
  return POCO_OK;
}

extern "C" void poco_evaluator_destroy(poco_evaluator_t e) { delete e; }
