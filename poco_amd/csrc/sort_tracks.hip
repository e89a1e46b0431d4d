// Video mode's --tracker sort: SORT (Bewley et al. 2016) on per-frame person boxes - a constant-velocity Kalman filter per person and
// one optimal IoU assignment per frame - for C clips at once.  It stands where the reference's POCOTester.run_tracking calls
// multi_person_tracker's SORT behind its detector.  The contract is stated in include/poco_hip.h (poco_op_sort_tracks) and DESIGN.md
// section 32; tests/sort_np.py restates it in float64 numpy with plain loops and scipy's assignment.
//
// One launch, a block of ONE wave per clip, the frames of the clip a sequential loop inside the block; clips are independent, so no
// grid barrier, no atomics, no spin-wait: the phases of a frame are separated by __syncthreads alone.  Per frame:
//   A  lane d < D loads its detection and its corners; lane k < K predicts its tracker (state and packed symmetric covariance from
//      LDS into registers and back) and leaves the corners of the predicted box.
//   B  the D x K gated IoU matrix into LDS, a lane per pair, ceil(D K / 64) passes.
//   C  the assignment on the max(D, K) square (missing pairs cost 0): shortest augmenting paths with potentials, a lane per column,
//      the row potentials a lane per row, every minimum a butterfly over the wave; all state in registers, rows of the matrix
//      read from LDS along the lanes.  Trip bounds: 64 rows, 65 steps per row, 65 steps per augmentation.
//   D  lane d ranks the unmatched detections by ballot (births in detection order); lane k < K updates its tracker with its detection
//      and writes that detection's outputs; an unmatched lane d starts tracker K + rank and writes its own.
//   E  lane k < K + births reads its tracker, a ballot over `time_since_update <= max_age` gives its new slot, and after a barrier
//      it writes it there: the order of the trackers is kept.
// LDS 58.4 KB (the matrix 32 KB, 64 packed covariances 14 KB, states, boxes, counters): two blocks fit a CU's 160 KB.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int SM = SORT_MAX;
constexpr int NP = 28;                                                  // the lower triangle of a 7 x 7 matrix
static_assert(SORT_THREADS == 64 && SM == 64, "a wave per clip, a lane per person");

struct SortDev {
  const double* dets;
  const int *frame_offsets, *clip_offsets;
  int *tracker, *id;
  double* box;
  int *count, *status;
  double thr;
  int C, F, N, max_age, min_hits, max_trackers;
};

struct Shared {
  double g[SM * SM];                                                    // gated IoU, [d][k]
  double P[NP][SM];                                                     // packed lower triangles, element-major: lanes side by side
  double x[7][SM];
  double det[4][SM];                                                    // cx, cy, w, h
  double dc[4][SM], tc[4][SM];                                          // corners of the detections / of the predicted boxes
  int tsu[SM], streak[SM], ident[SM], tok[SM], match_t[SM], colrow[SM];
  int stop;
};
static_assert(sizeof(Shared) <= 60 * 1024, "sort_tracks: the block's LDS");

__device__ __forceinline__ double quiet_nan64() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ void load_state(const Shared& S, int k, double (&x)[7], double (&P)[7][7]) {
  #pragma unroll
  for (int i = 0; i < 7; ++i) x[i] = S.x[i][k];
  #pragma unroll
  for (int r = 0; r < 7; ++r)
    #pragma unroll
    for (int c = 0; c <= r; ++c) P[r][c] = P[c][r] = S.P[tri(r, c)][k];
}

__device__ __forceinline__ void store_state(Shared& S, int k, const double (&x)[7], const double (&P)[7][7]) {
  #pragma unroll
  for (int i = 0; i < 7; ++i) S.x[i][k] = x[i];
  #pragma unroll
  for (int r = 0; r < 7; ++r)
    #pragma unroll
    for (int c = 0; c <= r; ++c) S.P[tri(r, c)][k] = P[r][c];
}

// x <- F x, P <- F P F^T + Q on the lower triangle (the upper one is its copy)
__device__ __forceinline__ void kalman_predict(double (&x)[7], double (&P)[7][7]) {
  #pragma clang fp contract(off)
  const double Q[7] = {1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001};
  if (x[2] + x[6] <= 0.0) x[6] = 0.0;
  #pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = x[i] + x[i + 4];
  double M[7][7];
  #pragma unroll
  for (int i = 0; i < 7; ++i)
    #pragma unroll
    for (int j = 0; j < 7; ++j) M[i][j] = i < 3 ? P[i][j] + P[i + 4][j] : P[i][j];
  #pragma unroll
  for (int i = 0; i < 7; ++i)
    #pragma unroll
    for (int j = 0; j <= i; ++j) {
      double v = j < 3 ? M[i][j] + M[i][j + 4] : M[i][j];
      if (i == j) v = v + Q[i];
      P[i][j] = v;
    }
  #pragma unroll
  for (int i = 0; i < 7; ++i)
    #pragma unroll
    for (int j = 0; j < i; ++j) P[j][i] = P[i][j];
}

// the update with z = (cx, cy, w h, w / h): S = P[:4,:4] + R = L D L^T, K = P[:,:4] S^-1, x += K y, the Joseph form of P
__device__ __forceinline__ void kalman_update(double (&x)[7], double (&P)[7][7], const double (&z)[4]) {
  #pragma clang fp contract(off)
  const double R[4] = {1.0, 1.0, 10.0, 10.0};
  double y[4], S[4][4], L[4][4], D[4], K[7][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = z[i] - x[i];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) S[i][j] = i == j ? P[i][j] + R[i] : P[i][j];
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    double v = S[j][j];
    #pragma unroll
    for (int k = 0; k < j; ++k) v = v - L[j][k] * (L[j][k] * D[k]);
    D[j] = v;
    #pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double w = S[i][j];
      #pragma unroll
      for (int k = 0; k < j; ++k) w = w - L[i][k] * (L[j][k] * D[k]);
      L[i][j] = w / D[j];
    }
  }
  #pragma unroll
  for (int r = 0; r < 7; ++r) {
    double w[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      double v = P[r][i];
      #pragma unroll
      for (int k = 0; k < i; ++k) v = v - L[i][k] * w[k];
      w[i] = v;
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = w[i] / D[i];
    #pragma unroll
    for (int i = 3; i >= 0; --i) {
      double v = w[i];
      #pragma unroll
      for (int k = i + 1; k < 4; ++k) v = v - L[k][i] * K[r][k];
      K[r][i] = v;
    }
  }
  #pragma unroll
  for (int r = 0; r < 7; ++r) {
    double acc = K[r][0] * y[0];
    #pragma unroll
    for (int c = 1; c < 4; ++c) acc = acc + K[r][c] * y[c];
    x[r] = x[r] + acc;
  }
  double AP[7][7];
  #pragma unroll
  for (int r = 0; r < 7; ++r)
    #pragma unroll
    for (int j = 0; j < 7; ++j) {
      double t = K[r][0] * P[0][j];
      #pragma unroll
      for (int c = 1; c < 4; ++c) t = t + K[r][c] * P[c][j];
      AP[r][j] = P[r][j] - t;
    }
  #pragma unroll
  for (int r = 0; r < 7; ++r)
    #pragma unroll
    for (int j = 0; j <= r; ++j) {
      double t1 = AP[r][0] * K[j][0], t2 = (K[r][0] * R[0]) * K[j][0];
      #pragma unroll
      for (int c = 1; c < 4; ++c) {
        t1 = t1 + AP[r][c] * K[j][c];
        t2 = t2 + (K[r][c] * R[c]) * K[j][c];
      }
      P[r][j] = (AP[r][j] - t1) + t2;
    }
  #pragma unroll
  for (int r = 0; r < 7; ++r)
    #pragma unroll
    for (int j = 0; j < r; ++j) P[j][r] = P[r][j];
}

// (w, h) of a state: w = sqrt(s r), h = s / w
__device__ __forceinline__ void state_size(const double (&x)[7], double& w, double& h) {
  #pragma clang fp contract(off)
  w = sqrt(x[2] * x[3]);
  h = x[2] / w;
}

__device__ __forceinline__ bool finite64(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL; }

__device__ __forceinline__ double gated_iou(const Shared& S, int d, int k, double thr) {
  #pragma clang fp contract(off)
  if (!S.tok[k]) return 0.0;
  const double a0 = S.dc[0][d], a1 = S.dc[1][d], a2 = S.dc[2][d], a3 = S.dc[3][d];
  const double b0 = S.tc[0][k], b1 = S.tc[1][k], b2 = S.tc[2][k], b3 = S.tc[3][k];
  const double xx1 = a0 > b0 ? a0 : b0, yy1 = a1 > b1 ? a1 : b1, xx2 = a2 < b2 ? a2 : b2, yy2 = a3 < b3 ? a3 : b3;
  const double dw = xx2 - xx1, dh = yy2 - yy1;
  const double w = dw > 0.0 ? dw : 0.0, h = dh > 0.0 ? dh : 0.0;
  const double wh = w * h;
  const double o = wh / (((a2 - a0) * (a3 - a1) + (b2 - b0) * (b3 - b1)) - wh);
  return o >= thr ? o : 0.0;                                            // a NaN is no match
}

// The matching of the n x n square (n = max(D, K); cost -g inside D x K, 0 outside) of least cost: on return lane j < n holds the
// row of column j.  u: the potential of row `lane`, v: of column `lane`; minv, way, used: of column `lane`; in_tree: of row `lane`.
__device__ __forceinline__ int assign_columns(const Shared& S, int D, int K, int lane) {
  #pragma clang fp contract(off)
  const int n = D > K ? D : K;
  const double INF = 1.0e300;
  double u = 0.0, v = 0.0;
  int p = -1;
  for (int i = 0; i < SM; ++i) {                                        // a row per pass: at most 64
    if (i >= n) break;
    double minv = INF;
    int way = -1;                                                       // -1: the virtual column the path starts from
    bool used = false, in_tree = lane == i;
    int j0 = -1, i0 = i;
    for (int step = 0; step < SM + 1; ++step) {                         // a column joins the tree per step: at most n of them
      if (lane == j0) used = true;
      if (lane == i0) in_tree = true;
      const double ui0 = __shfl(u, i0);
      const bool open = lane < n && !used;
      if (open) {
        const double a = (i0 < D && lane < K) ? -S.g[i0 * SM + lane] : 0.0;
        const double cur = (a - ui0) - v;
        if (cur < minv) { minv = cur; way = j0; }
      }
      double best = open ? minv : INF;
      int bj = open ? lane : SM;
      #pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
      }
      if (bj >= n) break;                                               // no open column: cannot happen while a row is unassigned
      if (in_tree) u = u + best;
      if (used) v = v - best;
      else if (lane < n) minv = minv - best;
      j0 = bj;
      const int pj = __shfl(p, j0);
      if (pj < 0) break;                                                // a free column: the path is complete
      i0 = pj;
    }
    for (int step = 0; step < SM + 1; ++step) {                         // walk the path back: at most n + 1 columns
      if (j0 < 0) break;
      const int j1 = __shfl(way, j0);
      const int pn = __shfl(p, j1 & (SM - 1));
      if (lane == j0) p = j1 < 0 ? i : pn;
      j0 = j1;
    }
  }
  return p;
}

__global__ __launch_bounds__(SORT_THREADS) void sort_tracks_clips(SortDev q) {
  #pragma clang fp contract(off)
  __shared__ Shared S;
  const int lane = threadIdx.x;
  const int c = blockIdx.x;
  if (c >= q.C) return;                                                 // block-uniform
  // offsets the caller did not check cannot take a lane outside the buffers
  const int f0 = min(max(q.clip_offsets[c], 0), q.F), f1 = min(max(q.clip_offsets[c + 1], f0), q.F);
  int K = 0, next_id = 0, status = 0, stop_lo = 0;
  for (int f = f0; f < f1; ++f) {                                       // block-uniform: every lane reaches every barrier
    const int lo = q.frame_offsets[f], hi = q.frame_offsets[f + 1];
    if (lo < 0 || hi < lo || hi > q.N || hi - lo > SM) {                // not a frame of at most 64 detections inside the buffer
      status = 2;
      stop_lo = min(max(lo, 0), q.N);
      break;
    }
    const int D = hi - lo, fc = f - f0 + 1;
    // ---- A: detections, predict -------------------------------------------------------------------------------------------------
    if (lane < D) {
      const double* z = q.dets + (size_t)(lo + lane) * 4;
      const double cx = z[0], cy = z[1], w = z[2], h = z[3];
      S.det[0][lane] = cx; S.det[1][lane] = cy; S.det[2][lane] = w; S.det[3][lane] = h;
      S.dc[0][lane] = cx - w / 2.0; S.dc[1][lane] = cy - h / 2.0; S.dc[2][lane] = cx + w / 2.0; S.dc[3][lane] = cy + h / 2.0;
    }
    if (lane < K) {
      double x[7], P[7][7];
      load_state(S, lane, x, P);
      kalman_predict(x, P);
      store_state(S, lane, x, P);
      if (S.tsu[lane] > 0) S.streak[lane] = 0;
      S.tsu[lane] += 1;
      double w, h;
      state_size(x, w, h);
      S.tok[lane] = (finite64(w) && finite64(h) && finite64(x[0]) && finite64(x[1]) && w > 0.0 && h > 0.0) ? 1 : 0;
      S.tc[0][lane] = x[0] - w / 2.0; S.tc[1][lane] = x[1] - h / 2.0; S.tc[2][lane] = x[0] + w / 2.0; S.tc[3][lane] = x[1] + h / 2.0;
    }
    if (lane == 0) S.stop = 0;
    __syncthreads();
    // ---- B: the gated IoU matrix --------------------------------------------------------------------------------------------------
    for (int e = lane; e < D * K; e += SORT_THREADS) {
      const int d = e / K, k = e - d * K;
      S.g[d * SM + k] = gated_iou(S, d, k, q.thr);
    }
    __syncthreads();
    // ---- C: the assignment ---------------------------------------------------------------------------------------------------------
    const int n = D > K ? D : K;
    S.match_t[lane] = -1;
    S.colrow[lane] = SM;                                                // column of row `lane`: none
    __syncthreads();
    if (D > 0 && K > 0) {
      const int p = assign_columns(S, D, K, lane);
      if (lane < n && p >= 0 && p < n) {
        S.colrow[p] = lane;
        if (lane < K && p < D && S.g[p * SM + lane] > 0.0) S.match_t[lane] = p;
      }
    }
    __syncthreads();
    // ---- D: births in detection order, updates, outputs ----------------------------------------------------------------------------
    bool unmatched = false;
    if (lane < D) {
      const int col = S.colrow[lane];
      unmatched = !(col < K && S.match_t[col] == lane);
    }
    const unsigned long long births = __ballot(unmatched);
    const int nb = __popcll(births);
    if (K + nb > q.max_trackers) {                                      // wave-uniform: the clip stops here
      status = 1;
      stop_lo = lo;
      break;
    }
    const int rank = __popcll(births & ((1ULL << lane) - 1ULL));
    if (lane < K && S.match_t[lane] >= 0) {
      const int d = S.match_t[lane];
      double x[7], P[7][7];
      load_state(S, lane, x, P);
      const double zw = S.det[2][d], zh = S.det[3][d];
      const double z[4] = {S.det[0][d], S.det[1][d], zw * zh, zw / zh};
      kalman_update(x, P, z);
      store_state(S, lane, x, P);
      S.tsu[lane] = 0;
      const int streak = S.streak[lane] + 1;
      S.streak[lane] = streak;
      double w, h;
      state_size(x, w, h);
      const size_t at = (size_t)(lo + d);
      q.tracker[at] = S.ident[lane];
      q.id[at] = (streak >= q.min_hits || fc <= q.min_hits) ? S.ident[lane] : -1;
      q.box[at * 4 + 0] = x[0]; q.box[at * 4 + 1] = x[1]; q.box[at * 4 + 2] = w; q.box[at * 4 + 3] = h;
    }
    if (unmatched) {                                                    // lane < D; slot K + rank < max_trackers <= 64
      const int slot = K + rank;
      const double zw = S.det[2][lane], zh = S.det[3][lane];
      double x[7] = {S.det[0][lane], S.det[1][lane], zw * zh, zw / zh, 0.0, 0.0, 0.0};
      const double P0[7] = {10.0, 10.0, 10.0, 10.0, 10000.0, 10000.0, 10000.0};
      #pragma unroll
      for (int i = 0; i < 7; ++i) S.x[i][slot] = x[i];
      #pragma unroll
      for (int r = 0; r < 7; ++r)
        #pragma unroll
        for (int cc = 0; cc <= r; ++cc) S.P[tri(r, cc)][slot] = r == cc ? P0[r] : 0.0;
      S.tsu[slot] = 0;
      S.streak[slot] = 0;
      S.ident[slot] = next_id + rank;
      double w, h;
      state_size(x, w, h);
      const size_t at = (size_t)(lo + lane);
      q.tracker[at] = next_id + rank;
      q.id[at] = (0 >= q.min_hits || fc <= q.min_hits) ? next_id + rank : -1;
      q.box[at * 4 + 0] = x[0]; q.box[at * 4 + 1] = x[1]; q.box[at * 4 + 2] = w; q.box[at * 4 + 3] = h;
    }
    next_id += nb;
    K += nb;
    __syncthreads();
    // ---- E: drop the trackers not seen for more than max_age frames, keeping the order ----------------------------------------------
    const bool keep = lane < K && S.tsu[lane] <= q.max_age;
    const unsigned long long kept = __ballot(keep);
    const int Kn = __popcll(kept);
    if (Kn != K) {                                                      // wave-uniform
      double x[7], P[7][7];
      int tsu = 0, streak = 0, ident = 0;
      if (keep) {
        load_state(S, lane, x, P);
        tsu = S.tsu[lane]; streak = S.streak[lane]; ident = S.ident[lane];
      }
      __syncthreads();
      if (keep) {
        const int slot = __popcll(kept & ((1ULL << lane) - 1ULL));
        store_state(S, slot, x, P);
        S.tsu[slot] = tsu; S.streak[slot] = streak; S.ident[slot] = ident;
      }
      K = Kn;
    }
    __syncthreads();
  }
  if (status != 0) {                                                    // the rest of the clip: -1, and no box
    const int end = min(max(q.frame_offsets[f1], stop_lo), q.N);
    for (int i = stop_lo + lane; i < end; i += SORT_THREADS) {
      q.tracker[i] = -1;
      q.id[i] = -1;
      #pragma unroll
      for (int k = 0; k < 4; ++k) q.box[(size_t)i * 4 + k] = quiet_nan64();
    }
  }
  if (lane == 0) {
    q.count[c] = next_id;
    q.status[c] = status;
  }
}

}  // namespace

void launch_sort_tracks(const double* dets, const int* frame_offsets, const int* clip_offsets, int C, int F, int N, double iou_thresh,
                        int max_age, int min_hits, int max_trackers, int* tracker, int* id, double* box, int* count, int* status,
                        hipStream_t s) {
  const SortDev q{dets, frame_offsets, clip_offsets, tracker, id, box, count, status, iou_thresh, C, F, N, max_age, min_hits, max_trackers};
  sort_tracks_clips<<<C, SORT_THREADS, 0, s>>>(q);
}
