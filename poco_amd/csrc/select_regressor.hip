// Choosing between two regressors by their own per-joint uncertainty (demo.py / eval.py --cfg2 --ckpt2 --select crop|joint).  The
// reference has no code for this (the paper's experiment was offline); what it does have is the post-processing the decision is
// made on: the kinematic accumulation of pocolib/utils/poco_utils.py:21-25 and the per-crop value of poco_utils.py:50-60.  The
// contract is stated in include/poco_hip.h (poco_op_select_regressor) and DESIGN.md section 25; tests/select_np.py restates it in
// float64 numpy with plain loops.  Everything here is a decision plus copies: every output is compared bit for bit.
//
// Two launches on the caller's stream, nothing read back, no atomics:
//   select_rows     one block of 256 threads per row, rows dealt by a grid-stride loop.  Wave 0 decides: lane j < 24 accumulates
//                   the uncertainty of joint j of both models down its ancestor chain (root first: the additions of
//                   kinematic_uncert in their order), lanes 0 and 1 form the two crop scores in fp64, then every lane j < 24 takes
//                   its choice - the row's in crop mode, its own comparison in joint mode - and leaves it in LDS.  After the
//                   barrier all threads copy: the nine floats of joint j and its var from the model chosen for j, every payload
//                   row from the model chosen for joint 0.
//   select_compact  ONE block of 128 threads walks the rows in chunks of 128 (a batch is at most a few hundred rows): mixed[r] =
//                   the 24 choices of row r are not all equal; the ordered list of mixed rows by ballot ranks + the two wave
//                   totals through LDS + a carried base (the scheme of track_infill_rows in track_infill.hip), and last the count.
// Every output word has exactly one writer and every value is a function of its row alone: the result does not depend on the grid.
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int NJ = 24;
// SMPL's kinematic tree (poco_amd/synth.py SMPL_PARENTS)
__constant__ int kParent[NJ] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};
constexpr int MAX_DEPTH = 10;                                         // the longest chain (a hand) has 9 joints

struct SelectDev {
  const float *pose0, *var0, *pose1, *var1;
  float *pose_out, *var_out, *score;
  unsigned char* choice;
  SelectPayloads pl;
  double thr, scale;
  int kind0, kind1, B, kinematic, mode;
};

// The processed uncertainty of joint j: var[j], or with `kinematic` u[j] = var[j] + u[parent] = the fp32 sum down the chain from
// the root, each addition on its own.
__device__ __forceinline__ float processed_uncert(const float* __restrict__ var, int j, int kinematic) {
  #pragma clang fp contract(off)
  if (!kinematic) return var[j];
  int depth = 0;                                                      // ancestors of j
  for (int k = kParent[j]; k >= 0 && depth < MAX_DEPTH; k = kParent[k]) ++depth;
  float u = var[0];
  for (int d = depth - 1; d >= 0; --d) {                              // the ancestor d steps above j, from below the root down to j
    int k = j;
    for (int i = 0; i < d; ++i) k = kParent[k];
    u = var[k] + u;
  }
  return u;
}

// poco_utils.py:50-60 on one row, in fp64 from the fp32 u: kind 1 (cliff) the root value against 2 thr, kind 0 (pare) the mean over
// the joints, in joint order, against thr; a row over its threshold scores exactly 1.
__device__ __forceinline__ double crop_score(const float* __restrict__ u, int kind, double thr) {
  #pragma clang fp contract(off)
  const double root = (double)u[0];
  if (kind == 1) return root > 2.0 * thr ? 1.0 : root;
  if (root > thr) return 1.0;
  double s = 0.0;
  for (int j = 0; j < NJ; ++j) s = s + (double)u[j];
  return s / 24.0;
}

// a score rounded once to fp32; a NaN is stored as the one quiet NaN 0x7fc00000 (which payload an addition hands on is the
// platform's business, not the contract's)
__device__ __forceinline__ uint32_t score_bits(double s) {
  return s != s ? 0x7fc00000u : __float_as_uint((float)s);
}

// n 32-bit words of one row, bit for bit, by all threads of the block, with the widest access the two addresses allow: where source
// and destination sit at the same offset inside a 16-byte (8-byte) line, a head of single words up to the line, a body of 16-byte
// (8-byte) words and a tail of single words; otherwise single words.  Nothing outside [0, n) of either row is touched.
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int n, int tid, int nthreads) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
  int head = 0, body = 0;                                             // in words; body a multiple of the vector width
  if (((sa ^ da) & 15) == 0) {
    head = min((int)(((16 - (sa & 15)) & 15) >> 2), n);
    body = (n - head) & ~3;
    const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
    uint4* d4 = reinterpret_cast<uint4*>(d + head);
    for (int i = tid; i < (body >> 2); i += nthreads) d4[i] = s4[i];
  } else if (((sa ^ da) & 7) == 0) {
    head = min((int)(((8 - (sa & 7)) & 7) >> 2), n);
    body = (n - head) & ~1;
    const uint2* s2 = reinterpret_cast<const uint2*>(s + head);
    uint2* d2 = reinterpret_cast<uint2*>(d + head);
    for (int i = tid; i < (body >> 1); i += nthreads) d2[i] = s2[i];
  }
  const int rest = n - body;                                          // head words [0, head) and tail words [head + body, n)
  for (int i = tid; i < rest; i += nthreads) {
    const int w = i < head ? i : i + body;
    d[w] = s[w];
  }
}

__global__ __launch_bounds__(256) void select_rows(SelectDev a) {
  #pragma clang fp contract(off)
  __shared__ float su[2][NJ];
  __shared__ double ssc[2];
  __shared__ unsigned char sch[NJ];
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < a.B; t += gridDim.x) {                 // block-uniform: every thread reaches every barrier
    const size_t row = (size_t)t;
    if (tid < NJ) {
      su[0][tid] = processed_uncert(a.var0 + row * NJ, tid, a.kinematic);
      su[1][tid] = processed_uncert(a.var1 + row * NJ, tid, a.kinematic);
    }
    __syncthreads();
    if (tid < 2) {
      const double g = crop_score(su[tid], tid == 0 ? a.kind0 : a.kind1, a.thr);
      const double s = tid == 0 ? g : a.scale * g;
      ssc[tid] = s;
      reinterpret_cast<uint32_t*>(a.score)[row * 2 + tid] = score_bits(s);
    }
    __syncthreads();
    if (tid < NJ) {
      // `<` is false for a tie and for a NaN on either side: model 0
      const bool one = a.mode == 0 ? ssc[1] < ssc[0] : a.scale * (double)su[1][tid] < (double)su[0][tid];
      sch[tid] = one ? 1 : 0;
      a.choice[row * NJ + tid] = one ? 1 : 0;
    }
    __syncthreads();
    if (tid < NJ * 9) {
      const int j = tid / 9;
      const uint32_t* p = reinterpret_cast<const uint32_t*>(sch[j] ? a.pose1 : a.pose0);
      reinterpret_cast<uint32_t*>(a.pose_out)[row * (NJ * 9) + tid] = p[row * (NJ * 9) + tid];
    } else if (tid < NJ * 9 + NJ) {
      const int j = tid - NJ * 9;
      const uint32_t* v = reinterpret_cast<const uint32_t*>(sch[j] ? a.var1 : a.var0);
      reinterpret_cast<uint32_t*>(a.var_out)[row * NJ + j] = v[row * NJ + j];
    }
    const bool root1 = sch[0] != 0;
    for (int k = 0; k < a.pl.count; ++k) {
      const SelectPayload& p = a.pl.p[k];
      const size_t off = row * (size_t)p.width;
      copy_row((root1 ? p.src1 : p.src0) + off, p.dst + off, p.width, tid, blockDim.x);
    }
    __syncthreads();                                                  // su / ssc / sch are rewritten by the block's next row
  }
}

// One block.  mixed[r] = 1 if the 24 choices of row r are not all equal; rows[0 .. count) = those rows in ascending order (both
// optional).
constexpr int COMPACT_THREADS = 128, COMPACT_WAVES = COMPACT_THREADS / 64;
__global__ __launch_bounds__(COMPACT_THREADS) void select_compact(const unsigned char* __restrict__ choice, int B, unsigned char* __restrict__ mixed,
                                                      int* __restrict__ rows, int* __restrict__ count) {
  __shared__ int wtot[COMPACT_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < B; c0 += COMPACT_THREADS) {
    const int r = c0 + tid;
    bool m = false;
    if (r < B) {
      const unsigned char* c = choice + (size_t)r * NJ;
      unsigned any = 0, all = 1;
      for (int j = 0; j < NJ; ++j) {
        any |= c[j];
        all &= c[j];
      }
      m = any != all;
      mixed[r] = m ? 1 : 0;
    }
    const unsigned long long mask = __ballot(m);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wv] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
    #pragma unroll
    for (int w = 0; w < COMPACT_WAVES; ++w) {
      if (w < wv) off += wtot[w];
      total += wtot[w];
    }
    if (m && rows) rows[base + off + before] = r;
    base += total;
    __syncthreads();                                                  // wtot is rewritten by the next chunk
  }
  if (tid == 0 && count) count[0] = base;
}

}  // namespace

void launch_select_regressor(const float* pose0, const float* var0, int kind0, const float* pose1, const float* var1, int kind1, int B,
                             int kinematic, double thr, double scale, int mode, const SelectPayloads& payloads, float* pose_out,
                             float* var_out, unsigned char* choice, float* score, unsigned char* mixed, int* rows, int* count,
                             int max_blocks, hipStream_t s) {
  const SelectDev d{pose0, var0, pose1, var1, pose_out, var_out, score, choice, payloads, thr, scale, kind0, kind1, B, kinematic, mode};
  int cap = max_blocks > 0 && max_blocks < SELECT_MAX_BLOCKS ? max_blocks : SELECT_MAX_BLOCKS;
  select_rows<<<B < cap ? B : cap, 256, 0, s>>>(d);
  select_compact<<<1, COMPACT_THREADS, 0, s>>>(choice, B, mixed, rows, count);
}
