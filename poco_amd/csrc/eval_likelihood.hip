// The flow likelihood of the ground truth under the model's own distribution, and the two uncertainty summaries of the evaluator:
// the kernels behind poco_flow_nll, poco_flow_nll_reduce and poco_evaluator_uncert_summary (include/poco_hip.h; entries in
// engine.hip / eval_metrics.hip, which own the handles).  Restates pocolib/models/head/nf_head.py:84-123 (the training-time branch of
// flow_head.forward), pocolib/losses/losses.py:346 and pocolib/core/trainer.py:374-378; tests/likelihood_np.py is the numpy form.
//
// poco_flow_nll is three steps on the caller's stream:
//   flow_residual_kernel   a block owns 64 (crop, joint) pairs: their 192 axis-angle floats are staged with one coalesced read, 64
//                          threads turn them into R_gt with rodrigues_f64 (the function poco_op_rodrigues and the evaluator use), then
//                          all 256 threads walk the block's 576 contiguous elements: bar = |R_pred - R_gt| / (sigma + 1e-9), carried in
//                          fp64, stored as the fp32 rows [B*24, 9] of bar_pose.reshape(-1, 9).  Reads and writes are unit-stride.
//   launch_realnvp         log_prob of the rows, rep = 24: one context row per crop (kernels_flow.hip).
//   flow_epilogue_kernel   one wave per crop: log sigma, mean_9(bar), the per-crop sum over the joints in joint order (fp64), zeros
//                          for an invalid crop (a select, so a NaN in an invalid crop's inputs does not leak).
// The reductions are one block each, fp64, strided then tree: a fixed order, no atomics - two runs give the same bits.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "rodrigues.h"

namespace {

constexpr int RES_ITEMS = 64;        // (crop, joint) pairs per block of the residual kernel
constexpr int RED_THREADS = 1024;
// record offsets (include/poco_hip.h)
constexpr int N_VALID = 0, N_SUM = 1, N_LOGPHI = 8, N_LOGSIGMA = 32, N_BAR = 56;
static_assert(N_BAR + 24 == FLOW_NLL_REC, "record layout");

__global__ __launch_bounds__(256) void flow_residual_kernel(const float* __restrict__ pred_pose, const float* __restrict__ gt_pose,
                                                            const float* __restrict__ var_pose, float* __restrict__ rows, int N) {
  __shared__ float saa[RES_ITEMS * 3];
  __shared__ double sR[RES_ITEMS * 9];
  __shared__ double sden[RES_ITEMS];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * RES_ITEMS;
  const int n = min(RES_ITEMS, N - i0);                    // pairs of this block (N = 24 B)
  if (t < n * 3) saa[t] = gt_pose[(size_t)i0 * 3 + t];
  __syncthreads();
  if (t < n) {
    rodrigues_f64(saa + 3 * t, sR + 9 * t);                // nf_head.py:89
    sden[t] = (double)var_pose[i0 + t] + 1e-9;             // nf_head.py:99,101: sigma repeated over the 3x3
  }
  __syncthreads();
  for (int e = t; e < n * 9; e += 256) {
    const size_t idx = (size_t)i0 * 9 + e;
    rows[idx] = (float)(fabs((double)pred_pose[idx] - sR[e]) / sden[e / 9]);
  }
}

__global__ __launch_bounds__(64) void flow_epilogue_kernel(const float* __restrict__ rows, const float* __restrict__ logphi,
                                                           const float* __restrict__ var_pose, const int* __restrict__ valid,
                                                           float* __restrict__ out) {
  __shared__ float sls[24], slp[24];
  const int b = blockIdx.x, t = threadIdx.x;
  const bool ok = valid ? valid[b] != 0 : true;
  float* rec = out + (size_t)b * FLOW_NLL_REC;
  if (t < 24) {
    const size_t r = (size_t)b * 24 + t;
    const float ls = (float)log((double)var_pose[r]);      // losses.py:346
    const float lp = logphi[r];
    double m = 0.0;
    #pragma unroll
    for (int k = 0; k < 9; ++k) m += (double)rows[r * 9 + k];
    sls[t] = ls; slp[t] = lp;
    rec[N_LOGPHI + t] = ok ? lp : 0.f;
    rec[N_LOGSIGMA + t] = ok ? ls : 0.f;
    rec[N_BAR + t] = ok ? (float)(m / 9.0) : 0.f;
  } else if (t >= 24 + 2 && t < 24 + N_LOGPHI) {
    rec[t - 24] = 0.f;                                     // [2..8)
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < 24; ++j) s += (double)sls[j] - (double)slp[j];
    rec[N_VALID] = ok ? 1.f : 0.f;
    rec[N_SUM] = ok ? (float)s : 0.f;
  }
}

// summary[4] = {valid crops, mean log phi, mean log sigma, loss_nf}; means over valid crops x 24 joints (0 / 0 = NaN without one)
__global__ __launch_bounds__(RED_THREADS) void flow_nll_reduce_kernel(const float* __restrict__ rec, long long N, double* __restrict__ summary) {
  __shared__ double red[RED_THREADS];
  double cnt = 0, lp = 0, ls = 0, df = 0;
  for (long long i = threadIdx.x; i < N; i += RED_THREADS) {
    const float* r = rec + (size_t)i * FLOW_NLL_REC;
    if (r[N_VALID] == 0.f) continue;
    cnt += 1.0;
    for (int j = 0; j < 24; ++j) {
      const double p = r[N_LOGPHI + j], s = r[N_LOGSIGMA + j];
      lp += p; ls += s; df += s - p;
    }
  }
  cnt = block_tree_sum<RED_THREADS>(cnt, red); lp = block_tree_sum<RED_THREADS>(lp, red);
  ls = block_tree_sum<RED_THREADS>(ls, red); df = block_tree_sum<RED_THREADS>(df, red);
  if (threadIdx.x == 0) {
    const double terms = 24.0 * cnt;
    summary[0] = cnt; summary[1] = lp / terms; summary[2] = ls / terms; summary[3] = df / terms;
  }
}

// summary[2] = {Var-MPJPE, Variance} (trainer.py:374,377-378) over the evaluator's records
__global__ __launch_bounds__(RED_THREADS) void eval_uncert_summary_kernel(const float* __restrict__ rec, int stride, int off_mpjpe, int off_unc,
                                                                          long long N, double* __restrict__ summary) {
  __shared__ double red[RED_THREADS];
  double q = 0, v = 0;
  for (long long i = threadIdx.x; i < N; i += RED_THREADS) {
    const float* r = rec + (size_t)i * stride;
    double m = 0.0;
    for (int j = 0; j < 24; ++j) m += (double)r[off_unc + j];
    m /= 24.0;                                             // poco_utils.py:169: pred_uncert.mean(1)
    q += (double)r[off_mpjpe] / (m + 1e-9);
    v += m;
  }
  q = block_tree_sum<RED_THREADS>(q, red); v = block_tree_sum<RED_THREADS>(v, red);
  if (threadIdx.x == 0) { summary[0] = q / (double)N; summary[1] = v / (double)N; }
}

}  // namespace

void launch_flow_residual(const float* pred_pose, const float* gt_pose, const float* var_pose, float* rows, int B, hipStream_t s) {
  const int N = B * 24;
  flow_residual_kernel<<<(N + RES_ITEMS - 1) / RES_ITEMS, 256, 0, s>>>(pred_pose, gt_pose, var_pose, rows, N);
}

void launch_flow_nll_epilogue(const float* rows, const float* logphi, const float* var_pose, const int* valid, float* out, int B,
                              hipStream_t s) {
  flow_epilogue_kernel<<<B, 64, 0, s>>>(rows, logphi, var_pose, valid, out);
}

void launch_flow_nll_reduce(const float* rec, long long N, double* d_summary4, hipStream_t s) {
  flow_nll_reduce_kernel<<<1, RED_THREADS, 0, s>>>(rec, N, d_summary4);
}

void launch_eval_uncert_summary(const float* rec, int stride, int off_mpjpe, int off_unc, long long N, double* d_summary2, hipStream_t s) {
  eval_uncert_summary_kernel<<<1, RED_THREADS, 0, s>>>(rec, stride, off_mpjpe, off_unc, N, d_summary2);
}
