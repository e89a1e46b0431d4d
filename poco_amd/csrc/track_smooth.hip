// Video mode's uncertainty-weighted smoother (demo.py --smooth_uncert LAMBDA): per track and per joint, the nine entries of the
// rotation matrices are smoothed over time by a penalised least-squares fit whose data term is weighted by the precision
// (u_ref / u)^2 and whose penalty is the squared second divided difference over the frame indices; each solved 3x3 is then taken
// back onto SO(3).  No counterpart in the reference.  The contract is stated in include/poco_hip.h (poco_op_track_smooth) and
// DESIGN.md section 28; tests/usmooth_np.py restates it in float64 numpy with a dense solve.
//
// One launch on the caller's stream, nothing read back, no atomics.  A block of 256 threads takes one (track, group of 7 joints):
//   solve     wave 0 only, one lane per right-hand-side column: lanes 0 .. 62 = 7 joints x 9 matrix entries (the last group: 3
//             joints, then the L linear columns, which use joint 0's weights).  A = diag(w) + lambda D^T Omega D is pentadiagonal;
//             every lane forms its joint's band from the frame indices and factors it as L D L^T on the way down (redundant within
//             the nine lanes of a joint: no cross-lane traffic, no divergence), substitutes forward in the same walk and writes
//             z / d (its own column) and the two sub-diagonals of L (one lane per joint) to the caller's scratch; on the way back up
//             it substitutes backward and leaves the fp64 solution in its scratch column (the linear columns go straight out).
//             A step is 3000 of them for a long track: the inputs of the next SM_CHUNK rows are loaded while this chunk is computed.
//   project   all four waves, one lane per (row, joint) of the group: the nine solved doubles -> the nearest rotation (Horn's
//             quaternion, cyclic Jacobi with a fixed sweep count: nearest_rotation of rotation_fit.h, shared with tta_fuse.hip and
//             eval_metrics.hip) -> nine floats and the angle to the input.
// The two __syncthreads between the phases order the scratch writes of one lane before the reads of another.  Every output word
// has exactly one writer and every value is a function of its own track alone: the bits do not depend on the other tracks or on
// the grid ((track, group) pairs are dealt to the blocks by a grid-stride loop).
#include "common.h"
#include "kernels.h"
#include "rotation_fit.h"

#include <cstdint>

namespace {

constexpr int NJ = 24;
constexpr int SM_GROUP = 7;                                           // joints of a block: 7 x 9 = 63 lanes of wave 0
constexpr int SM_GROUPS = 4;                                          // 7 + 7 + 7 + 3
constexpr int SM_CHUNK = 8;                                           // rows whose inputs are in flight together

struct SmoothDev {
  const float *pose, *u, *lin;
  const int *frames, *offsets;
  double* scratch;                                                    // [N][TRACK_SMOOTH_ROW_DOUBLES + L]
  float *pose_out, *lin_out, *shift;
  int P, N, L, max_gap;
  double lam, u_ref;
};

// Row t of D, the second divided difference over frames (f0, f1, f2) at columns t - 1, t, t + 1, and g = lambda * omega_t; all
// zero when a spacing exceeds max_gap (or is not positive: the caller's frames must increase strictly; such a row is dropped).
struct PenRow {
  double a, b, c, g;
};

__device__ __forceinline__ PenRow pen_row(int f0, int f1, int f2, int max_gap, double lam) {
  #pragma clang fp contract(off)
  const long long h1i = (long long)f1 - f0, h2i = (long long)f2 - f1;
  if (h1i < 1 || h2i < 1 || h1i > max_gap || h2i > max_gap) return {0.0, 0.0, 0.0, 0.0};
  const double h1 = (double)h1i, h2 = (double)h2i, hs = h1 + h2;
  return {2.0 / (h1 * hs), -2.0 / (h1 * h2), 2.0 / (h2 * hs), lam * (hs / 2.0)};
}

struct StepIn {
  float y, u;
  int f2;                                                             // frames[i + 2] (clamped to the track)
};

__global__ __launch_bounds__(TRACK_SMOOTH_THREADS) void track_smooth_blocks(SmoothDev d) {
  #pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = TRACK_SMOOTH_ROW_DOUBLES + d.L;                        // doubles of a scratch row
  const int fac0 = NJ * 9 + d.L;                                      // the factor slots follow the columns: 25 x (l1, l2)
  const long long items = (long long)d.P * SM_GROUPS;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {       // block-uniform: every thread reaches both barriers
    const int p = (int)(it / SM_GROUPS), grp = (int)(it % SM_GROUPS);
    // a track is rows [lo, hi) of the N rows; offsets the caller did not check cannot take a lane outside the buffers
    const int lo = max(d.offsets[p], 0), hi = min(d.offsets[p + 1], d.N);
    const int T = hi - lo;
    if (T <= 0) continue;
    const int j0 = grp * SM_GROUP, nj = min(SM_GROUP, NJ - j0);        // 7, 7, 7, 3 joints
    // ---- the lane's column (wave 0) ----------------------------------------------------------------------------------
    const int npose = nj * 9;
    const int nlin = grp == SM_GROUPS - 1 ? d.L : 0;
    const bool is_pose = lane < npose, is_lin = !is_pose && lane < npose + nlin;
    const bool active = wave == 0 && (is_pose || is_lin);
    const int jl = is_pose ? j0 + lane / 9 : 0;                        // the joint whose weights the column uses
    const float* src = is_lin ? d.lin + (lane - npose) : d.pose + (is_pose ? j0 * 9 + lane : 0);
    const size_t sstride = is_lin ? (size_t)d.L : (size_t)NJ * 9;
    const int scol = is_lin ? NJ * 9 + (lane - npose) : j0 * 9 + (is_pose ? lane : 0);
    // who writes a factor slot: entry 0 of a joint; the first linear column writes slot 24 (joint 0's factor once more)
    const bool fac_writer = active && (is_pose ? lane % 9 == 0 : lane == npose);
    const int fslot = fac0 + 2 * (is_lin ? NJ : jl);
    if (active) {
      auto load = [&](int i) -> StepIn {
        const size_t r = (size_t)(lo + min(i, T - 1));
        return {src[r * sstride], d.u[r * NJ + jl], d.frames[lo + min(i + 2, T - 1)]};
      };
      StepIn nxt[SM_CHUNK];
      #pragma unroll
      for (int k = 0; k < SM_CHUNK; ++k) nxt[k] = load(k);
      PenRow rm = {0, 0, 0, 0}, r0 = {0, 0, 0, 0};                     // rows i - 1 and i of D; row 0 is zero
      int fa = d.frames[lo], fb = d.frames[lo + min(1, T - 1)];        // frames[i], frames[i + 1]
      double l1p = 0, l2p = 0, l2pp = 0, dp = 0, dpp = 0, zp = 0, zpp = 0;
      for (int i0 = 0; i0 < T; i0 += SM_CHUNK) {
        StepIn cur[SM_CHUNK];
        #pragma unroll
        for (int k = 0; k < SM_CHUNK; ++k) {
          cur[k] = nxt[k];
          nxt[k] = load(i0 + SM_CHUNK + k);
        }
        #pragma unroll
        for (int k = 0; k < SM_CHUNK; ++k) {
          const int i = i0 + k;
          if (i >= T) break;
          const double w = uncert_weight(cur[k].u, d.u_ref);
          const int fc = cur[k].f2;
          const PenRow rp = i + 1 <= T - 2 ? pen_row(fa, fb, fc, d.max_gap, d.lam) : PenRow{0, 0, 0, 0};
          const double diag = w + ((rp.g * rp.a * rp.a + r0.g * r0.b * r0.b) + rm.g * rm.c * rm.c);
          const double e1 = r0.g * r0.b * r0.c + rp.g * rp.a * rp.b;
          const double e2 = rp.g * rp.a * rp.c;
          const double dd = (diag - l1p * l1p * dp) - l2pp * l2pp * dpp;
          const double inv = 1.0 / dd;
          const double l1 = (e1 - l1p * l2p * dp) * inv;
          const double l2 = e2 * inv;
          const double z = (w * (double)cur[k].y - l1p * zp) - l2pp * zpp;
          double* row = d.scratch + (size_t)(lo + i) * S;
          row[scol] = z * inv;
          if (fac_writer) {
            row[fslot] = l1;
            row[fslot + 1] = l2;
          }
          dpp = dp; dp = dd; l2pp = l2p; l2p = l2; l1p = l1; zpp = zp; zp = z;
          rm = r0; r0 = rp; fa = fb; fb = fc;
        }
      }
    }
    __syncthreads();                                                   // the factor slots: written by one lane, read by nine
    if (active) {
      struct BackIn { double zd, l1, l2; };
      auto load = [&](int i) -> BackIn {
        const double* row = d.scratch + (size_t)(lo + max(i, 0)) * S;
        return {row[scol], row[fslot], row[fslot + 1]};
      };
      BackIn nxt[SM_CHUNK];
      #pragma unroll
      for (int k = 0; k < SM_CHUNK; ++k) nxt[k] = load(T - 1 - k);
      double x1 = 0, x2 = 0;                                           // x[i + 1], x[i + 2]
      for (int i0 = T - 1; i0 >= 0; i0 -= SM_CHUNK) {
        BackIn cur[SM_CHUNK];
        #pragma unroll
        for (int k = 0; k < SM_CHUNK; ++k) {
          cur[k] = nxt[k];
          nxt[k] = load(i0 - SM_CHUNK - k);
        }
        #pragma unroll
        for (int k = 0; k < SM_CHUNK; ++k) {
          const int i = i0 - k;
          if (i < 0) break;
          const double x = (cur[k].zd - cur[k].l1 * x1) - cur[k].l2 * x2;
          if (is_lin) d.lin_out[(size_t)(lo + i) * d.L + (lane - npose)] = (float)x;
          else d.scratch[(size_t)(lo + i) * S + scol] = x;
          x2 = x1; x1 = x;
        }
      }
    }
    __syncthreads();                                                   // the solution: written by wave 0, read by all four
    // ---- projection: one lane per (row, joint) of the group --------------------------------------------------------------
    for (int idx = tid; idx < T * nj; idx += TRACK_SMOOTH_THREADS) {
      const int t = idx / nj, j = j0 + idx % nj;
      const size_t e = (size_t)(lo + t) * NJ + j;
      const double* xs = d.scratch + (size_t)(lo + t) * S + j * 9;
      const float* Rin = d.pose + e * 9;
      double M[9], R[9], A[9];
      #pragma unroll
      for (int i = 0; i < 9; ++i) {
        M[i] = xs[i];
        A[i] = (double)Rin[i];
      }
      nearest_rotation<ROT_JACOBI_SWEEPS>(M, R);
      // the angle of A^T R: atan2 of half the norm of its skew part and (trace - 1) / 2, well conditioned at 0 and at pi
      double Q[9];
      #pragma unroll
      for (int r = 0; r < 3; ++r)
        #pragma unroll
        for (int c = 0; c < 3; ++c) Q[r * 3 + c] = (A[r] * R[c] + A[3 + r] * R[3 + c]) + A[6 + r] * R[6 + c];
      const double sx = Q[7] - Q[5], sy = Q[2] - Q[6], sz = Q[3] - Q[1];
      const double sn = 0.5 * sqrt((sx * sx + sy * sy) + sz * sz), cs = 0.5 * (((Q[0] + Q[4]) + Q[8]) - 1.0);
      #pragma unroll
      for (int i = 0; i < 9; ++i) d.pose_out[e * 9 + i] = (float)R[i];
      d.shift[e] = (float)(atan2(sn, cs) * (180.0 / 3.14159265358979323846));
    }
  }
}

}  // namespace

void launch_track_smooth(const float* pose, const float* u, const int* frames, const int* offsets, int P, int N, const float* lin, int L,
                         double lam, double u_ref, int max_gap, double* scratch, float* pose_out, float* lin_out, float* shift,
                         int max_blocks, hipStream_t s) {
  const SmoothDev d{pose, u, lin, frames, offsets, scratch, pose_out, lin_out, shift, P, N, L, max_gap, lam, u_ref};
  const int cap = max_blocks > 0 && max_blocks < TRACK_SMOOTH_MAX_BLOCKS ? max_blocks : TRACK_SMOOTH_MAX_BLOCKS;
  const long long need = (long long)P * SM_GROUPS;
  track_smooth_blocks<<<(int)(need < cap ? need : cap), TRACK_SMOOTH_THREADS, 0, s>>>(d);
}
