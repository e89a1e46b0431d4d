// Block-wide primitives of the evaluation, video and codec kernels: one definition each, instantiated with the including file's own
// block size.  Every one has a fixed order of operations, so a kernel's bits do not depend on which file it was written in.  A new
// kernel that needs one of these includes this header; it does not restate them.
#pragma once
#include <hip/hip_runtime.h>

// The fp64 sum of the THREADS values of a block, returned to every lane: a halving tree in LDS (red[THREADS]), lane t adding
// red[t + o] to red[t] for o = THREADS / 2 .. 1.  Ends with a barrier, so `red` may be reused at once.
template <int THREADS>
__device__ __forceinline__ double block_tree_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = red[t] + red[t + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Exclusive prefix sum over the 64 * WAVES threads of a block (and the total): wave scans through __shfl_up, wave totals through
// LDS (wsum[WAVES]).  Ends with a barrier, so `wsum` may be reused at once.
template <int WAVES, class T>
__device__ __forceinline__ T block_exscan(T v, T* wsum, T* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T inc = v;
  #pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  #pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const T t = wsum[w];
    if (w < wv) base += t;
    tot += t;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// The least of the 64 * WAVES values of a block and the index that came with it, returned to every lane; of equal values the lower
// index wins, so the result does not depend on the order of the lanes.  Butterflies inside the waves, the waves' results through LDS
// (sval[WAVES], sidx[WAVES]).  Ends with a barrier, so both may be reused at once.
template <int WAVES>
__device__ __forceinline__ void block_argmin(double& v, int& idx, double* sval, int* sidx) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  #pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(idx, off);
    if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  if (lane == 0) { sval[wv] = v; sidx[wv] = idx; }
  __syncthreads();
  v = sval[0];
  idx = sidx[0];
  #pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    const double ov = sval[w];
    const int oi = sidx[w];
    if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  __syncthreads();
}

// Index of (r, c), r >= c, in a lower triangle packed row by row.
__device__ __forceinline__ constexpr int tri(int r, int c) { return r * (r + 1) / 2 + c; }
