// Video mode's in-fill: per track and per joint, the rotations whose uncertainty exceeds a threshold are replaced by the shortest-arc
// interpolation between the nearest confident frames on either side (demo.py --infill).  No counterpart in the reference (the paper
// used external motion models): the contract is stated in include/poco_hip.h (poco_op_track_infill) and DESIGN.md section 24;
// tests/infill_np.py restates it in float64 numpy.
//
// Two launches on the caller's stream, nothing read back, no atomics:
//   track_infill_columns  one wave64 per (track, joint) column, walking the track in chunks of 64 rows (lane = row within the chunk).
//                         Backward walk: the next reliable row of every row = an inclusive min-scan across the wave from the high
//                         lane down, with the carry of the chunks behind; written to the caller's scratch word of that entry.
//                         Forward walk: the last reliable row = an inclusive max-scan from the low lane up with the carry of the
//                         chunks before; then each lane reads back its own scratch word (the lane that wrote it: program order is
//                         enough), decides its entry's flag, converts, interpolates in fp64 and stores its own nine floats.  The
//                         wave of column 0 does the same for the row's linear block.
//   track_infill_rows     ONE block of 256 threads walks the N rows in chunks of 256: touched[r] = any flag of the row is 1 or 2;
//                         the ordered list of touched rows by ballot ranks + the four wave totals through LDS + a carried base
//                         (the scheme of pseudo_select in pseudo_gt.hip), and last the count.
// Every output word has exactly one writer and every value is a function of its column alone: the result does not depend on the
// grid (columns are dealt to the blocks by a grid-stride loop), two runs give the same bits.
#include "common.h"
#include "kernels.h"

#include <climits>
#include <cstdint>

namespace {

constexpr int NJ = 24;

struct Quat {
  double w, x, y, z;
};

// Rotation matrix (row-major, fp32) -> unit quaternion in fp64: Shepperd's largest-of-four branch (the first of equal candidates in
// the order trace, m00, m11, m22), then normalised.
__device__ __forceinline__ Quat quat_of(const float* __restrict__ R) {
  #pragma clang fp contract(off)
  const double m00 = R[0], m01 = R[1], m02 = R[2], m10 = R[3], m11 = R[4], m12 = R[5], m20 = R[6], m21 = R[7], m22 = R[8];
  const double tr = (m00 + m11) + m22;
  int k = 0;
  double best = tr;
  if (m00 > best) { k = 1; best = m00; }
  if (m11 > best) { k = 2; best = m11; }
  if (m22 > best) { k = 3; }
  Quat q;
  if (k == 0) {
    const double s = sqrt(1.0 + tr) * 2.0;
    q = {0.25 * s, (m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s};
  } else if (k == 1) {
    const double s = sqrt(((1.0 + m00) - m11) - m22) * 2.0;
    q = {(m21 - m12) / s, 0.25 * s, (m01 + m10) / s, (m02 + m20) / s};
  } else if (k == 2) {
    const double s = sqrt(((1.0 + m11) - m00) - m22) * 2.0;
    q = {(m02 - m20) / s, (m01 + m10) / s, 0.25 * s, (m12 + m21) / s};
  } else {
    const double s = sqrt(((1.0 + m22) - m00) - m11) * 2.0;
    q = {(m10 - m01) / s, (m02 + m20) / s, (m12 + m21) / s, 0.25 * s};
  }
  const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
  return {q.w / n, q.x / n, q.y / n, q.z / n};
}

// slerp(a, b, s) on the shortest arc: b is negated when a.b < 0; anchors closer than 1 - 1e-12 in |a.b| blend linearly and are
// normalised, the others go through acos and sin.
__device__ __forceinline__ Quat slerp(const Quat& a, Quat b, double s) {
  #pragma clang fp contract(off)
  double d = ((a.w * b.w + a.x * b.x) + a.y * b.y) + a.z * b.z;
  if (d < 0.0) {
    b = {-b.w, -b.x, -b.y, -b.z};
    d = -d;
  }
  if (d > 1.0 - 1e-12) {
    const Quat q = {a.w + s * (b.w - a.w), a.x + s * (b.x - a.x), a.y + s * (b.y - a.y), a.z + s * (b.z - a.z)};
    const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
    return {q.w / n, q.x / n, q.y / n, q.z / n};
  }
  const double th = acos(d), st = sin(th);
  const double wa = sin((1.0 - s) * th) / st, wb = sin(s * th) / st;
  return {wa * a.w + wb * b.w, wa * a.x + wb * b.x, wa * a.y + wb * b.y, wa * a.z + wb * b.z};
}

// unit quaternion -> rotation matrix, the standard form; rounded once to fp32 on store
__device__ __forceinline__ void store_rotmat(const Quat& q, float* __restrict__ R) {
  #pragma clang fp contract(off)
  const double w = q.w, x = q.x, y = q.y, z = q.z;
  R[0] = (float)(1.0 - 2.0 * (y * y + z * z));
  R[1] = (float)(2.0 * (x * y - w * z));
  R[2] = (float)(2.0 * (x * z + w * y));
  R[3] = (float)(2.0 * (x * y + w * z));
  R[4] = (float)(1.0 - 2.0 * (x * x + z * z));
  R[5] = (float)(2.0 * (y * z - w * x));
  R[6] = (float)(2.0 * (x * z - w * y));
  R[7] = (float)(2.0 * (y * z + w * x));
  R[8] = (float)(1.0 - 2.0 * (x * x + y * y));
}

// n 32-bit words, bit for bit (a float move could quieten a signalling NaN)
__device__ __forceinline__ void copy_words(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (int i = 0; i < n; ++i) d[i] = s[i];
}

struct InfillDev {
  const float *pose, *u, *lin;
  const int *frames, *offsets;
  int* scratch;                              // [24][N]: the next reliable row of every entry, INT_MAX = none
  float *pose_out, *lin_out;
  unsigned char* flags;
  int P, N, L, max_gap;
  float thresh;
};

__global__ __launch_bounds__(64) void track_infill_columns(InfillDev d) {
  #pragma clang fp contract(off)
  const int lane = threadIdx.x;
  for (int col = blockIdx.x; col < d.P * NJ; col += gridDim.x) {              // wave-uniform: every lane takes part in every shuffle
    const int p = col / NJ, j = col - p * NJ;
    // a track is rows [lo, hi) of the N rows; offsets the caller did not check cannot take a lane outside the buffers
    const int lo = max(d.offsets[p], 0), hi = min(d.offsets[p + 1], d.N);
    if (hi <= lo) continue;
    const int nchunk = (hi - lo + 63) >> 6;
    int* nxt = d.scratch + (size_t)j * d.N;
    // backward: next reliable row at or after each row (a reliable row names itself; only unreliable rows read it)
    int carry = INT_MAX;
    for (int c = nchunk - 1; c >= 0; --c) {
      const int r = lo + (c << 6) + lane;
      const bool in = r < hi;
      int v = (in && d.u[(size_t)r * NJ + j] <= d.thresh) ? r : INT_MAX;      // a NaN compares false: unreliable
      #pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_down(v, s);
        if (lane + s < 64) v = min(v, o);
      }
      v = min(v, carry);
      if (in) nxt[r] = v;
      carry = __shfl(v, 0);
    }
    // forward: last reliable row at or before each row, then the row's own entry
    carry = -1;
    for (int c = 0; c < nchunk; ++c) {
      const int r = lo + (c << 6) + lane;
      const bool in = r < hi;
      const bool rel = in && d.u[(size_t)r * NJ + j] <= d.thresh;
      int v = rel ? r : -1;
      #pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s);
        if (lane >= s) v = max(v, o);
      }
      v = max(v, carry);
      carry = __shfl(v, 63);
      if (!in) continue;                                                      // (after the last shuffle of this chunk)
      const size_t e = (size_t)r * NJ + j;
      const float* Rin = d.pose + e * 9;
      float* Rout = d.pose_out + e * 9;
      const float* lin_in = d.lin + (size_t)r * d.L;
      float* lin_out = d.lin_out + (size_t)r * d.L;
      const bool do_lin = j == 0 && d.L > 0;
      int flag = 0;
      if (!rel) {
        const int a = v, b = nxt[r] == INT_MAX ? -1 : nxt[r];
        const long long ft = d.frames[r], fa = a >= 0 ? d.frames[a] : 0, fb = b >= 0 ? d.frames[b] : 0;
        flag = 3;
        if (a >= 0 && b >= 0 && fb - fa <= d.max_gap) {
          flag = 1;
          const double s = (double)(ft - fa) / (double)(fb - fa);
          store_rotmat(slerp(quat_of(d.pose + ((size_t)a * NJ + j) * 9), quat_of(d.pose + ((size_t)b * NJ + j) * 9), s), Rout);
          if (do_lin) {
            const float *la = d.lin + (size_t)a * d.L, *lb = d.lin + (size_t)b * d.L;
            for (int i = 0; i < d.L; ++i) lin_out[i] = (float)((double)la[i] + s * ((double)lb[i] - (double)la[i]));
          }
        } else if (a >= 0 || b >= 0) {
          // the existing anchor nearer in frames, a tie to a; held if it is at most max_gap // 2 frames away
          const bool use_a = b < 0 || (a >= 0 && ft - fa <= fb - ft);
          const int c2 = use_a ? a : b;
          const long long dist = use_a ? ft - fa : fb - ft;
          if (dist <= d.max_gap / 2) {
            flag = 2;
            copy_words(d.pose + ((size_t)c2 * NJ + j) * 9, Rout, 9);
            if (do_lin) copy_words(d.lin + (size_t)c2 * d.L, lin_out, d.L);
          }
        }
      }
      if (flag == 0 || flag == 3) {
        copy_words(Rin, Rout, 9);
        if (do_lin) copy_words(lin_in, lin_out, d.L);
      }
      d.flags[e] = (unsigned char)flag;
    }
  }
}

// One block.  touched[r] = 1 if any of the row's 24 flags is 1 or 2; rows[0 .. count) = those rows in ascending order (both optional).
__global__ __launch_bounds__(256) void track_infill_rows(const unsigned char* __restrict__ flags, int N, unsigned char* __restrict__ touched,
                                                         int* __restrict__ rows, int* __restrict__ count) {
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < N; c0 += 256) {
    const int r = c0 + tid;
    bool t = false;
    if (r < N) {
      const unsigned char* f = flags + (size_t)r * NJ;
      for (int j = 0; j < NJ; ++j) t = t || f[j] == 1 || f[j] == 2;
      touched[r] = t ? 1 : 0;
    }
    const unsigned long long mask = __ballot(t);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wv] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
    #pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wv) off += wtot[w];
      total += wtot[w];
    }
    if (t && rows) rows[base + off + before] = r;
    base += total;
    __syncthreads();                         // wtot is rewritten by the next chunk
  }
  if (tid == 0 && count) count[0] = base;
}

}  // namespace

void launch_track_infill(const float* pose, const float* u, const int* frames, const int* offsets, int P, int N, const float* lin, int L,
                         float thresh, int max_gap, int* scratch, float* pose_out, float* lin_out, unsigned char* flags,
                         unsigned char* touched, int* rows, int* count, hipStream_t s) {
  const InfillDev d{pose, u, lin, frames, offsets, scratch, pose_out, lin_out, flags, P, N, L, max_gap, thresh};
  const long long cols = (long long)P * NJ;
  track_infill_columns<<<(int)(cols < TRACK_INFILL_MAX_BLOCKS ? cols : TRACK_INFILL_MAX_BLOCKS), 64, 0, s>>>(d);
  track_infill_rows<<<1, 256, 0, s>>>(flags, N, touched, rows, count);
}
