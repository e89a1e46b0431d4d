// Video mode's --track_stitch: the fragments a tracker left of one person - broken by an occlusion longer than its memory - joined
// into chains after the forward, by the regressor's own body shape (betas, weighted by the model's uncertainty) and the extrapolated
// motion of the boxes, as ONE optimal assignment of tails to heads per clip.  The contract is stated in include/poco_hip.h
// (poco_op_track_stitch) and DESIGN.md section 36; tests/stitch_np.py restates it in float64 numpy with plain loops and scipy's
// assignment.
//
// Three launches, no grid barrier, no atomics, no spin-wait; every loop is a `for` bounded by the sizes, every index taken from a
// table is clamped to its buffer:
//   1  stitch_describe  a block of one wave per fragment: the rows go along the lanes (lane l takes rows l, l + 64, ...), the sums
//                       through block_tree_sum; lanes 0..5 then fit the six lines (tail / head x cx, cy, log h) over at most 32 rows.
//   2  stitch_gains     a block of 256 per tail fragment, a lane per head of the same clip: a row of the clip's gain matrix, kept
//                       in the caller's scratch (row stride 256 doubles: 256 x 256 fp64 = 512 KB do not fit a block's LDS).
//   3  stitch_assign    a block of 256 per clip, a lane per column: shortest augmenting paths with potentials (the method of
//                       sort_tracks.hip on up to 256 columns: the row potentials, the matching and the path in LDS, every minimum
//                       through block_argmin), then successors, predecessors, gains and the chain numbers.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int SMAX = STITCH_MAX_FRAGS;
constexpr int DW = STITCH_DESC;
static_assert(SMAX == 256 && STITCH_THREADS == 256 && STITCH_ROW_THREADS == 64 && DW == 28, "a lane per fragment of a clip");

struct StitchDev {
  const int *clip_offsets, *frag_offsets, *frames;
  const double* boxes;
  const float *betas, *var;
  int C, P, N, max_gap, fit_len;
  double u_ref, motion_tol, shape_tol, shape_floor, shape_w;
  double* G;
  int *succ, *pred, *chain;
  double *gain, *desc;
  int* status;
};

__device__ __forceinline__ bool finite64(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL; }

// rows [lo, hi) of fragment p, or false where the table does not describe at least one row inside the buffers
__device__ __forceinline__ bool fragment_rows(const StitchDev& q, int p, int& lo, int& hi) {
  lo = q.frag_offsets[p];
  hi = q.frag_offsets[p + 1];
  return lo >= 0 && hi > lo && hi <= q.N;
}

// the weight of a row: (u_ref / max(mean of var[0..23], 1e-6))^2, the mean summed in ascending joint order
__device__ __forceinline__ double row_weight(const float* var, double u_ref) {
  #pragma clang fp contract(off)
  double u = (double)var[0];
  #pragma unroll
  for (int j = 1; j < 24; ++j) u = u + (double)var[j];
  u = u / 24.0;
  const double r = u_ref / (u > 1e-6 ? u : 1e-6);
  return r * r;
}

// ---- 1: the descriptor of a fragment ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STITCH_ROW_THREADS) void stitch_describe(StitchDev q) {
  #pragma clang fp contract(off)
  __shared__ double red[STITCH_ROW_THREADS];
  const int lane = threadIdx.x, p = blockIdx.x;
  if (p >= q.P) return;                                                 // block-uniform
  double* out = q.desc + (size_t)p * DW;
  int lo, hi;
  if (!fragment_rows(q, p, lo, hi)) {                                   // block-uniform: the clip ends with status 2 (stitch_assign)
    if (lane < DW) out[lane] = 0.0;
    return;
  }
  const int T = hi - lo;
  // pass 1: W, W2 and the weighted sums of the betas
  double aW = 0.0, aW2 = 0.0, ab[10];
  #pragma unroll
  for (int k = 0; k < 10; ++k) ab[k] = 0.0;
  for (int i = lane; i < T; i += STITCH_ROW_THREADS) {
    const double w = row_weight(q.var + (size_t)(lo + i) * 24, q.u_ref);
    const float* b = q.betas + (size_t)(lo + i) * 10;
    aW = aW + w;
    aW2 = aW2 + w * w;
    #pragma unroll
    for (int k = 0; k < 10; ++k) ab[k] = ab[k] + w * (double)b[k];
  }
  const double W = block_tree_sum<STITCH_ROW_THREADS>(aW, red);
  const double W2 = block_tree_sum<STITCH_ROW_THREADS>(aW2, red);
  double bbar[10];
  #pragma unroll
  for (int k = 0; k < 10; ++k) bbar[k] = block_tree_sum<STITCH_ROW_THREADS>(ab[k], red) / W;
  // pass 2: the weighted spread of the betas about their mean
  double as = 0.0;
  for (int i = lane; i < T; i += STITCH_ROW_THREADS) {
    const double w = row_weight(q.var + (size_t)(lo + i) * 24, q.u_ref);
    const float* b = q.betas + (size_t)(lo + i) * 10;
    const double d0 = (double)b[0] - bbar[0];
    double d = d0 * d0;
    #pragma unroll
    for (int k = 1; k < 10; ++k) {
      const double dk = (double)b[k] - bbar[k];
      d = d + dk * dk;
    }
    as = as + w * d;
  }
  const double sig2 = block_tree_sum<STITCH_ROW_THREADS>(as, red) / W / 10.0;
  const int s = q.frames[lo], e = q.frames[hi - 1];
  if (lane < 10) out[lane] = bbar[lane];
  if (lane == 10) out[10] = sig2;
  if (lane == 11) out[11] = W;
  if (lane == 12) out[12] = W2;
  if (lane == 13) out[13] = (double)T;
  if (lane == 14) out[26] = (double)s;
  if (lane == 15) out[27] = (double)e;
  // the six lines: lane = 3 * (0 tail | 1 head) + (0 cx | 1 cy | 2 log h), over m <= 32 rows, t centred
  if (lane < 6) {
    const int head = lane / 3, qi = lane - 3 * head;
    const int m = T < q.fit_len ? T : q.fit_len;
    const int r0 = head ? lo : hi - m;
    const long long ref = head ? s : e;
    double tsum = 0.0, qsum = 0.0;
    for (int j = 0; j < m; ++j) {
      const double* bx = q.boxes + (size_t)(r0 + j) * 4;
      tsum = tsum + (double)((long long)q.frames[r0 + j] - ref);
      qsum = qsum + (qi == 0 ? bx[0] : qi == 1 ? bx[1] : log(bx[3]));
    }
    const double tbar = tsum / (double)m, qbar = qsum / (double)m;
    double stt = 0.0, stq = 0.0;
    for (int j = 0; j < m; ++j) {
      const double* bx = q.boxes + (size_t)(r0 + j) * 4;
      const double dt = (double)((long long)q.frames[r0 + j] - ref) - tbar;
      const double dq = (qi == 0 ? bx[0] : qi == 1 ? bx[1] : log(bx[3])) - qbar;
      stt = stt + dt * dt;
      stq = stq + dt * dq;
    }
    double vel = 0.0, state = qbar;
    if (m > 1 && stt > 0.0) {
      vel = stq / stt;
      state = qbar - vel * tbar;
    }
    out[14 + 6 * head + qi] = state;
    out[17 + 6 * head + qi] = vel;
  }
}

// the clip of fragment a: the last c with clip_offsets[c] <= a (a binary search of at most 32 steps), and its clamped range
__device__ __forceinline__ int clip_of(const StitchDev& q, int a, int& clo, int& chi) {
  int l = 0, r = q.C;                                                   // the answer lies in [l, r)
  for (int it = 0; it < 32; ++it) {
    if (r - l <= 1) break;
    const int mid = l + (r - l) / 2;
    if (q.clip_offsets[mid] <= a) l = mid; else r = mid;
  }
  clo = min(max(q.clip_offsets[l], 0), q.P);
  chi = min(max(q.clip_offsets[l + 1], clo), q.P);
  return l;
}

// ---- 2: a row of the gain matrix ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STITCH_THREADS) void stitch_gains(StitchDev q) {
  #pragma clang fp contract(off)
  const int j = threadIdx.x, a = blockIdx.x;
  if (a >= q.P) return;
  int clo, chi;
  clip_of(q, a, clo, chi);
  const int n = chi - clo;
  if (a < clo || a >= chi || n > SMAX || j >= n) return;                // a clip stitch_assign ends with status 2 reads no matrix
  const int b = clo + j;
  const double* da = q.desc + (size_t)a * DW;
  const double* db = q.desc + (size_t)b * DW;
  double g = 0.0;
  const long long D = (long long)db[26] - (long long)da[27];
  if (b != a && D >= 1 && D <= (long long)q.max_gap + 1) {
    const double h = (double)D / 2.0;
    const double pax = da[14] + da[17] * h, pay = da[15] + da[18] * h, pal = da[16] + da[19] * h;
    const double pbx = db[20] - db[23] * h, pby = db[21] - db[24] * h, pbl = db[22] - db[25] * h;
    const double dx = pax - pbx, dy = pay - pby, dl = pal - pbl;
    const double cm = sqrt((dx * dx + dy * dy) / (exp(pal) * exp(pbl)) + dl * dl) / (q.motion_tol * sqrt((double)D));
    const double e0 = da[0] - db[0];
    double ss = e0 * e0;
    #pragma unroll
    for (int k = 1; k < 10; ++k) {
      const double ek = da[k] - db[k];
      ss = ss + ek * ek;
    }
    const double cs = sqrt(ss / 10.0) / sqrt((da[10] + db[10]) + q.shape_floor * q.shape_floor) / q.shape_tol;
    const bool drop = !finite64(cm) || !finite64(cs) || cm > 1.0 || (q.shape_w > 0.0 && cs > 1.0);
    if (!drop) {
      g = 1.0 - (cm * cm + q.shape_w * (cs * cs)) / (1.0 + q.shape_w);
      if (!(g > 0.0)) g = 0.0;
    }
  }
  q.G[(size_t)a * SMAX + j] = g;
}

// ---- 3: the assignment of a clip, and what follows from it ---------------------------------------------------------------------------
struct AssignShared {
  double u[SMAX];                                                       // the potential of row `lane`
  int p[SMAX], way[SMAX];                                               // the row of column `lane`; the column before it on the path
  int succ[SMAX], pred[SMAX];
  double sval[STITCH_THREADS / 64];
  int sidx[STITCH_THREADS / 64];
  int wsum[STITCH_THREADS / 64];
};

__global__ __launch_bounds__(STITCH_THREADS) void stitch_assign(StitchDev q) {
  #pragma clang fp contract(off)
  __shared__ AssignShared S;
  const int lane = threadIdx.x, c = blockIdx.x;
  if (c >= q.C) return;                                                 // block-uniform
  const int raw_lo = q.clip_offsets[c], raw_hi = q.clip_offsets[c + 1];
  const int clo = min(max(raw_lo, 0), q.P), chi = min(max(raw_hi, clo), q.P);
  const int n = min(chi - clo, SMAX);
  bool bad = raw_lo < 0 || raw_hi < raw_lo || raw_hi > q.P || raw_hi - raw_lo > SMAX;
  if (lane < n) {
    int lo, hi;
    bad = bad || !fragment_rows(q, clo + lane, lo, hi);
  }
  if (__syncthreads_or(bad ? 1 : 0)) {                                  // a table the kernel cannot read: every fragment on its own
    for (int i = clo + lane; i < chi; i += STITCH_THREADS) {
      q.succ[i] = -1;
      q.pred[i] = -1;
      q.chain[i] = i - clo;
      q.gain[i] = 0.0;
    }
    if (lane == 0) q.status[c] = 2;
    return;
  }
  const double* G = q.G + (size_t)clo * SMAX;                           // cost of (row i, column j) = -G[i * 256 + j]
  const double INF = 1.0e300;
  S.u[lane] = 0.0;
  S.p[lane] = -1;
  S.succ[lane] = -1;
  S.pred[lane] = -1;
  double v = 0.0;
  __syncthreads();
  for (int i = 0; i < n; ++i) {                                         // a row per pass: at most 256
    double minv = INF;
    int way = -1;                                                       // -1: the virtual column the path starts from
    bool used = false, in_tree = lane == i;
    int j0 = -1, i0 = i;
    for (int step = 0; step < SMAX + 1; ++step) {                       // a column joins the tree per step: at most n of them
      if (lane == j0) used = true;
      if (lane == i0) in_tree = true;
      const double ui0 = S.u[i0];
      const bool open = lane < n && !used;
      if (open) {
        const double cur = (-G[(size_t)i0 * SMAX + lane] - ui0) - v;
        if (cur < minv) { minv = cur; way = j0; }
      }
      double best = open ? minv : INF;
      int bj = open ? lane : SMAX;
      block_argmin<STITCH_THREADS / 64>(best, bj, S.sval, S.sidx);
      if (bj >= n) break;                                               // no open column: cannot happen while a row is unassigned
      if (in_tree) S.u[lane] = S.u[lane] + best;
      if (used) v = v - best;
      else if (lane < n) minv = minv - best;
      j0 = bj;
      __syncthreads();
      const int pj = S.p[j0];
      if (pj < 0) break;                                                // a free column: the path is complete
      i0 = min(pj, n - 1);
    }
    S.way[lane] = way;
    __syncthreads();
    if (lane == 0) {                                                    // walk the path back: at most n + 1 columns
      int j = j0;
      for (int step = 0; step < SMAX + 1; ++step) {
        if (j < 0) break;
        const int j1 = min(S.way[j], SMAX - 1);
        S.p[j] = j1 < 0 ? i : S.p[j1];
        j = j1;
      }
    }
    __syncthreads();
  }
  // links: column `lane` took row p; a pair of gain 0 is no link
  double my_gain = 0.0;
  if (lane < n) {
    const int r = S.p[lane];
    if (r >= 0 && r < n) {
      my_gain = G[(size_t)r * SMAX + lane];
      if (my_gain > 0.0) {
        S.pred[lane] = r;
        S.succ[r] = lane;
      }
    }
  }
  __syncthreads();
  if (lane < n) {
    const int sc = S.succ[lane], pr = S.pred[lane];
    q.succ[clo + lane] = sc < 0 ? -1 : clo + sc;
    q.pred[clo + lane] = pr < 0 ? -1 : clo + pr;
    q.gain[clo + lane] = sc < 0 ? 0.0 : G[(size_t)lane * SMAX + sc];
  }
  // chains: numbered by the index of their first fragment; its lane walks the chain (at most n fragments, D >= 1: no cycle)
  const bool first = lane < n && S.pred[lane] < 0;
  int heads = 0;
  const int number = block_exscan<STITCH_THREADS / 64, int>(first ? 1 : 0, S.wsum, &heads);
  if (first) {
    int f = lane;
    for (int step = 0; step < SMAX; ++step) {
      if (f < 0 || f >= n) break;
      q.chain[clo + f] = number;
      f = S.succ[f];
    }
  }
  if (lane == 0) q.status[c] = 0;
}

}  // namespace

void launch_track_stitch(const int* clip_offsets, const int* frag_offsets, const int* frames, const double* boxes, const float* betas,
                         const float* var, int C, int P, int N, int max_gap, int fit_len, double u_ref, double motion_tol,
                         double shape_tol, double shape_floor, double shape_w, double* scratch, int* succ, int* pred, int* chain,
                         double* gain, double* desc, int* status, hipStream_t s) {
  const StitchDev q{clip_offsets, frag_offsets, frames, boxes, betas, var, C, P, N, max_gap, fit_len, u_ref, motion_tol, shape_tol,
                    shape_floor, shape_w, scratch, succ, pred, chain, gain, desc, status};
  if (P > 0) {
    stitch_describe<<<P, STITCH_ROW_THREADS, 0, s>>>(q);
    stitch_gains<<<P, STITCH_THREADS, 0, s>>>(q);
  }
  stitch_assign<<<C, STITCH_THREADS, 0, s>>>(q);
}
