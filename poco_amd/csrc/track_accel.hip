// eval.py --sequences: the temporal metric of a ragged buffer of tracks - per row the mean over the joints of the norm of the
// second difference of the predicted joints (the prediction's own jitter) and of its difference to the ground truth's (the
// acceleration error of the VIBE line of work), and their fp64 sums per track and over all tracks.  No counterpart in the
// reference.  The contract is stated in include/poco_hip.h (poco_op_track_accel) and DESIGN.md section 29; tests/accel_np.py
// restates it in float64 with plain loops.
//
// Three launches on the caller's stream, nothing read back, no atomics:
//   rows    a block of 256 threads takes a tile of 64 rows.  The 66 rows it needs (one of halo on either side) are read ONCE from
//           each buffer, consecutive lanes along a row, into LDS - the caller's row stride (the evaluator's records in place:
//           416 floats of which 42 are read) never reaches the arithmetic.  64 lanes then decide which rows are valid (a binary
//           search in the offsets, three frame ids).  A half-wave takes a row, a lane a joint: the three-point stencil, the norm,
//           and a halving tree over the 32 lanes in fp64; lane 0 of the half rounds once and stores, and leaves the fp64 terms
//           in the caller's scratch.
//   tracks  a block per track: every lane adds the terms of rows t, t + 256, ... in ascending order, then a halving tree in LDS.
//   total   one block does the same over the tracks' sums.
// Every output word has one writer and every value is a function of its own track alone: the bits do not depend on the grid (tiles
// and tracks are dealt to the blocks by grid-stride loops) and repeat from run to run.
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int AC_TILE = TRACK_ACCEL_TILE;
constexpr int AC_HALO = AC_TILE + 2;                                   // rows t0 - 1 .. t0 + 64
constexpr int AC_ROW = 3 * TRACK_ACCEL_MAX_JOINTS;                     // floats of an LDS row
constexpr int AC_T = TRACK_ACCEL_THREADS;
constexpr int AC_RD = TRACK_ACCEL_ROW_DOUBLES;
static_assert(AC_T == 256 && AC_TILE == 64, "four waves, two rows per wave and pass: 64 rows in 8 passes");

struct AccelDev {
  const float *pred, *gt;
  const int *frames, *offsets;
  double* scratch;                                                    // [N][3]: acceleration error, acceleration, valid
  float *accel, *accel_err;
  double *track_sums, *total;
  int stride, M, P, N;
};

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7fc00000u); }

// |(x0 - 2 x1) + x2| of joint m from three LDS rows, and the same of the difference to the ground truth's
__device__ __forceinline__ void second_difference(const float* r0, const float* r1, const float* r2, int m, double (&a)[3]) {
  #pragma clang fp contract(off)
  #pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = ((double)r0[3 * m + c] - 2.0 * (double)r1[3 * m + c]) + (double)r2[3 * m + c];
}

__device__ __forceinline__ double norm3(const double (&v)[3]) {
  #pragma clang fp contract(off)
  return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

// the halving tree over the 32 lanes of a half-wave: every lane of the half ends with the sum
__device__ __forceinline__ double half_wave_sum(double v) {
  #pragma clang fp contract(off)
  #pragma unroll
  for (int d = 16; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 32);
  return v;
}

__global__ __launch_bounds__(AC_T) void track_accel_rows(AccelDev d) {
  #pragma clang fp contract(off)
  __shared__ float sp[AC_HALO * AC_ROW], sg[AC_HALO * AC_ROW];
  __shared__ int svalid[AC_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = 3 * d.M;                                              // floats of a row that are read
  const bool with_gt = d.gt != nullptr;
  const int tiles = (d.N + AC_TILE - 1) / AC_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {       // block-uniform: every thread reaches every barrier
    const int t0 = tile * AC_TILE;
    // ---- the 66 rows, once: consecutive lanes along a row -------------------------------------------------------------------
    for (int e = tid; e < AC_HALO * W; e += AC_T) {
      const int r = e / W, c = e - r * W;
      const int g = t0 - 1 + r;
      const bool in = g >= 0 && g < d.N;
      const size_t at = (size_t)(in ? g : 0) * (size_t)d.stride + (size_t)c;
      sp[r * AC_ROW + c] = in ? d.pred[at] : 0.f;
      if (with_gt) sg[r * AC_ROW + c] = in ? d.gt[at] : 0.f;
    }
    // ---- which rows are valid ---------------------------------------------------------------------------------------------------
    if (tid < AC_TILE) {
      const int g = t0 + tid;
      int ok = 0;
      if (g < d.N) {
        int a = 0, b = d.P - 1;                                        // the last track whose first row is <= g
        while (a < b) {
          const int mid = (a + b + 1) >> 1;
          if (d.offsets[mid] <= g) a = mid; else b = mid - 1;
        }
        // a track is rows [lo, hi) of the N rows; offsets the caller did not check cannot take a lane outside the buffers
        const int lo = max(d.offsets[a], 0), hi = min(d.offsets[a + 1], d.N);
        if (g - 1 >= lo && g + 1 < hi) {
          const long long f0 = d.frames[g - 1], f1 = d.frames[g], f2 = d.frames[g + 1];
          ok = (f0 + 1 == f1 && f1 + 1 == f2) ? 1 : 0;
        }
      }
      svalid[tid] = ok;
    }
    __syncthreads();
    // ---- a half-wave per row, a lane per joint ----------------------------------------------------------------------------------
    const int half = lane >> 5, m = lane & 31;
    #pragma unroll 1
    for (int k = 0; k < AC_TILE / 8; ++k) {
      const int r = wave * (AC_TILE / 4) + 2 * k + half;               // row of the tile; LDS row r + 1
      const int g = t0 + r;
      const bool ok = g < d.N && svalid[r] != 0;
      double acc = 0.0, err = 0.0;
      if (ok && m < d.M) {
        const float *p0 = sp + r * AC_ROW, *p1 = p0 + AC_ROW, *p2 = p1 + AC_ROW;
        double a[3];
        second_difference(p0, p1, p2, m, a);
        acc = norm3(a);
        if (with_gt) {
          const float *g0 = sg + r * AC_ROW, *g1 = g0 + AC_ROW, *g2 = g1 + AC_ROW;
          double b[3];
          second_difference(g0, g1, g2, m, b);
          const double e[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
          err = norm3(e);
        }
      }
      acc = half_wave_sum(acc) / (double)d.M;                          // every lane takes part in the shuffles
      err = half_wave_sum(err) / (double)d.M;
      if (m == 0 && g < d.N) {
        d.accel[g] = ok ? (float)acc : quiet_nan();
        if (with_gt) d.accel_err[g] = ok ? (float)err : quiet_nan();
        double* s = d.scratch + (size_t)g * AC_RD;
        s[0] = ok ? err : 0.0;
        s[1] = ok ? acc : 0.0;
        s[2] = ok ? 1.0 : 0.0;
      }
    }
    __syncthreads();                                                   // the LDS rows are overwritten by the next tile
  }
}

// sum of the AC_RD columns of rows [lo, hi) of `src`: rows lo + tid, lo + tid + 256, ... per lane, then a halving tree
__device__ __forceinline__ void block_sum3(const double* src, int lo, int hi, double (*red)[AC_RD], double* out) {
  #pragma clang fp contract(off)
  const int tid = threadIdx.x;
  double v[AC_RD] = {0.0, 0.0, 0.0};
  for (int i = lo + tid; i < hi; i += AC_T)
    #pragma unroll
    for (int c = 0; c < AC_RD; ++c) v[c] = v[c] + src[(size_t)i * AC_RD + c];
  #pragma unroll
  for (int c = 0; c < AC_RD; ++c) red[tid][c] = v[c];
  __syncthreads();
  for (int w = AC_T / 2; w >= 1; w >>= 1) {
    if (tid < w)
      #pragma unroll
      for (int c = 0; c < AC_RD; ++c) red[tid][c] = red[tid][c] + red[tid + w][c];
    __syncthreads();
  }
  if (tid < AC_RD) out[tid] = red[0][tid];
  __syncthreads();                                                     // `red` is reused by the caller's next item
}

__global__ __launch_bounds__(AC_T) void track_accel_tracks(AccelDev d) {
  __shared__ double red[AC_T][AC_RD];
  for (int p = blockIdx.x; p < d.P; p += gridDim.x) {
    const int lo = min(max(d.offsets[p], 0), d.N), hi = min(max(d.offsets[p + 1], lo), d.N);
    block_sum3(d.scratch, lo, hi, red, d.track_sums + (size_t)p * AC_RD);
  }
}

__global__ __launch_bounds__(AC_T) void track_accel_total(AccelDev d) {
  __shared__ double red[AC_T][AC_RD];
  block_sum3(d.track_sums, 0, d.P, red, d.total);
}

}  // namespace

void launch_track_accel(const float* pred, const float* gt, int stride, int M, const int* frames, const int* offsets, int P, int N,
                        double* scratch, float* accel, float* accel_err, double* track_sums, double* total, int max_blocks, hipStream_t s) {
  const AccelDev d{pred, gt, frames, offsets, scratch, accel, accel_err, track_sums, total, stride, M, P, N};
  const int cap = max_blocks > 0 && max_blocks < TRACK_ACCEL_MAX_BLOCKS ? max_blocks : TRACK_ACCEL_MAX_BLOCKS;
  const int tiles = (N + AC_TILE - 1) / AC_TILE;
  track_accel_rows<<<tiles < cap ? tiles : cap, AC_T, 0, s>>>(d);
  track_accel_tracks<<<P < cap ? P : cap, AC_T, 0, s>>>(d);
  track_accel_total<<<1, AC_T, 0, s>>>(d);
}
