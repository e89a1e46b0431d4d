// The cluster bootstrap of eval.py --bootstrap: per-unit fp64 moments of E value planes and B resamples of the U units with replacement,
// every sum in a fixed order.  The contract is stated in include/poco_hip.h (poco_op_bootstrap) and DESIGN.md section 34;
// tests/boot_np.py restates it with plain loops and math.fsum.
//
//   center     center[e] = the mean of plane e over its n rows: tiles of BOOT_TILE rows (a block each: lane-strided fp64 sums, then a
//              halving tree over the 256 lanes) leave one partial per (plane, tile) in the scratch buffer; one block per plane adds the
//              partials the same way and divides once by n.  The tree is a function of n alone.
//   unit_mom   a wave per unit u = rows [offsets[u], offsets[u+1]) (clamped into [0, n]; no offsets: row u): column after column, lane
//              l adds the rows lo + l, lo + l + 64, ... in order, then a halving shuffle tree over the 64 lanes; lane 0 writes.  Column
//              0 = the rows, 1..E = the raw values, E+1..E+P = (v_a - center_a) * (v_b - center_b), the product rounded before it is added.
//   draws      Philox4x32-10, key = (seed low, seed high), counter = (q, 0, b, 0): its four words are draws 4q .. 4q+3 of replicate b,
//              draw j picks unit (word * U) >> 32.  Replicate 0 is the identity: draw j picks unit j.
//   resample   a block of 256 lanes per replicate.  Lane t owns the counters q = t, t + 256, ... and adds the rows unit_mom[idx] of
//              their draws 4q, 4q+1, 4q+2, 4q+3 (those below U) in that order into M accumulators; then per column a halving shuffle
//              tree inside each of the four waves and wave 0 + wave 1 + wave 2 + wave 3, left to right.  Which additions form an
//              output word is fixed by (U, M) and the draws: not by the grid, B or the order in which blocks finish.
//   counts     draw_counts is zeroed by a launch of its own, then filled with integer atomics (their result has no order).
//
// No floating-point atomics, no spin-wait, no grid barrier.  LDS: boot_center 2 KB, boot_resample 4 x BOOT_MAX_M x 8 = 1056 bytes.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "philox.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int BT_TH = BOOT_THREADS;
constexpr int BT_TILE = BOOT_TILE;
constexpr int BT_WAVES = BT_TH / 64;
static_assert(BT_TH == 256 && BT_WAVES == 4, "the trees below are written for four waves of 64");

struct BootDev {
  const float* planes;       // [E][n]
  const int32_t* offsets;    // [U + 1] or null
  long long n, U, B;
  int E, P, M, NT;
  int8_t pa[BOOT_MAX_PAIRS], pb[BOOT_MAX_PAIRS];
  uint32_t k0, k1;           // the Philox key
  double* partial;           // scratch [E][NT]
  double* center;            // [E]
  double* unit_mom;          // [U][M]
  double* out;               // [B + 1][M]
  uint32_t* counts;          // [B][U] or null
};

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double wave_tree(double v) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
  return v;                                                             // lane 0 holds the sum
}

__global__ __launch_bounds__(BT_TH) void boot_center_tiles(BootDev a) {
  __shared__ double red[BT_TH];
  const long long items = (long long)a.E * a.NT;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int e = (int)(it / a.NT), tile = (int)(it % a.NT);
    const long long r0 = (long long)tile * BT_TILE, r1 = r0 + BT_TILE < a.n ? r0 + BT_TILE : a.n;
    const float* p = a.planes + (size_t)e * (size_t)a.n;
    double acc = 0.0;
    for (long long r = r0 + threadIdx.x; r < r1; r += BT_TH) acc = acc + (double)p[r];
    acc = block_tree_sum<BT_TH>(acc, red);
    if (threadIdx.x == 0) a.partial[it] = acc;
  }
}

__global__ __launch_bounds__(BT_TH) void boot_center_final(BootDev a) {
  __shared__ double red[BT_TH];
  for (int e = blockIdx.x; e < a.E; e += gridDim.x) {
    const double* p = a.partial + (size_t)e * a.NT;
    double acc = 0.0;
    for (int i = threadIdx.x; i < a.NT; i += BT_TH) acc = acc + p[i];
    acc = block_tree_sum<BT_TH>(acc, red);
    if (threadIdx.x == 0) a.center[e] = acc / (double)a.n;
  }
}

__global__ __launch_bounds__(BT_TH) void boot_unit_mom(BootDev a) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * BT_WAVES;
  for (long long u = (long long)blockIdx.x * BT_WAVES + (threadIdx.x >> 6); u < a.U; u += waves) {
    long long lo = u, hi = u + 1;
    if (a.offsets) {
      lo = clampll(a.offsets[u], 0, a.n);
      hi = clampll(a.offsets[u + 1], lo, a.n);
    } else {
      lo = clampll(lo, 0, a.n);
      hi = clampll(hi, lo, a.n);
    }
    double* row = a.unit_mom + (size_t)u * a.M;
    if (lane == 0) row[0] = (double)(hi - lo);
    for (int e = 0; e < a.E; ++e) {
      const float* p = a.planes + (size_t)e * (size_t)a.n;
      double acc = 0.0;
      for (long long r = lo + lane; r < hi; r += 64) acc = acc + (double)p[r];
      acc = wave_tree(acc);
      if (lane == 0) row[1 + e] = acc;
    }
    for (int k = 0; k < a.P; ++k) {
      const int ea = a.pa[k], eb = a.pb[k];
      const float* p = a.planes + (size_t)ea * (size_t)a.n;
      const float* q = a.planes + (size_t)eb * (size_t)a.n;
      const double ca = a.center[ea], cb = a.center[eb];
      double acc = 0.0;
      for (long long r = lo + lane; r < hi; r += 64) {
        const double prod = ((double)p[r] - ca) * ((double)q[r] - cb);
        acc = acc + prod;
      }
      acc = wave_tree(acc);
      if (lane == 0) row[1 + a.E + k] = acc;
    }
  }
}

__global__ __launch_bounds__(BT_TH) void boot_zero_counts(uint32_t* counts, unsigned long long words) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * BT_TH + threadIdx.x; i < words; i += (unsigned long long)gridDim.x * BT_TH)
    counts[i] = 0u;
}

// MM: the compile-time bound of the accumulators (a.M <= MM), so that they stay in registers.
template <int MM>
__global__ __launch_bounds__(BT_TH) void boot_resample(BootDev a) {
  __shared__ double part[BT_WAVES][MM];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, M = a.M;
  const long long quads = (a.U + 3) / 4;
  for (long long b = blockIdx.x; b <= a.B; b += gridDim.x) {
    double acc[MM];
    #pragma unroll
    for (int m = 0; m < MM; ++m) acc[m] = 0.0;
    for (long long q = t; q < quads; q += BT_TH) {
      Philox4 x{{0u, 0u, 0u, 0u}};
      if (b > 0) x = philox4x32_10((uint32_t)q, 0u, (uint32_t)b, 0u, a.k0, a.k1);
      #pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long j = 4 * q + i;
        if (j < a.U) {
          const long long idx = b > 0 ? (long long)(((uint64_t)x.w[i] * (uint64_t)a.U) >> 32) : j;   // < U
          const double* row = a.unit_mom + (size_t)idx * M;
          // every load is issued, none behind a branch: a column past M reads the row's last word again and adds nothing
          double v[MM];
          #pragma unroll
          for (int m = 0; m < MM; ++m) v[m] = row[m < M ? m : M - 1];
          #pragma unroll
          for (int m = 0; m < MM; ++m) acc[m] = acc[m] + (m < M ? v[m] : 0.0);
          if (b > 0 && a.counts) atomicAdd(a.counts + (size_t)(b - 1) * (size_t)a.U + (size_t)idx, 1u);
        }
      }
    }
    #pragma unroll
    for (int m = 0; m < MM; ++m) {
      const double s = wave_tree(acc[m]);
      if (lane == 0) part[wave][m] = s;
    }
    __syncthreads();
    if (t < M) a.out[(size_t)b * M + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    __syncthreads();
  }
}

size_t boot_up256(size_t b) { return (b + 255) & ~(size_t)255; }

int boot_grid(long long items, int cap) { return (int)(items < 1 ? 1 : (items < cap ? items : cap)); }

}  // namespace

BootScratch boot_scratch_layout(long long n, int E) {
  BootScratch L{};
  L.NT = (int)((n + BT_TILE - 1) / BT_TILE);
  L.partial = 0;
  L.bytes = boot_up256((size_t)E * (size_t)L.NT * 8);
  return L;
}

void launch_bootstrap(const float* planes, long long n, int E, const int* pairs, int P, const int* unit_offsets, long long U, long long B,
                      unsigned long long seed, void* scratch, double* center, double* unit_mom, double* out, unsigned* draw_counts,
                      int max_blocks, hipStream_t s) {
  const BootScratch L = boot_scratch_layout(n, E);
  BootDev d{};
  d.planes = planes; d.offsets = unit_offsets;
  d.n = n; d.U = U; d.B = B;
  d.E = E; d.P = P; d.M = 1 + E + P; d.NT = L.NT;
  for (int k = 0; k < P; ++k) { d.pa[k] = (int8_t)pairs[2 * k]; d.pb[k] = (int8_t)pairs[2 * k + 1]; }
  d.k0 = (uint32_t)(seed & 0xffffffffull); d.k1 = (uint32_t)(seed >> 32);
  d.partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + L.partial);
  d.center = center; d.unit_mom = unit_mom; d.out = out; d.counts = B > 0 ? draw_counts : nullptr;
  const int cap = max_blocks > 0 && max_blocks < BOOT_MAX_BLOCKS ? max_blocks : BOOT_MAX_BLOCKS;
  boot_center_tiles<<<boot_grid((long long)E * L.NT, cap), BT_TH, 0, s>>>(d);
  boot_center_final<<<boot_grid(E, cap), BT_TH, 0, s>>>(d);
  boot_unit_mom<<<boot_grid((U + BT_WAVES - 1) / BT_WAVES, cap), BT_TH, 0, s>>>(d);
  if (d.counts) {
    const unsigned long long words = (unsigned long long)B * (unsigned long long)U;
    boot_zero_counts<<<boot_grid((long long)((words + BT_TH - 1) / BT_TH), cap), BT_TH, 0, s>>>(d.counts, words);
  }
  const int grid = boot_grid(B + 1, cap);
  if (d.M <= 4) boot_resample<4><<<grid, BT_TH, 0, s>>>(d);
  else if (d.M <= 8) boot_resample<8><<<grid, BT_TH, 0, s>>>(d);
  else if (d.M <= 12) boot_resample<12><<<grid, BT_TH, 0, s>>>(d);
  else if (d.M <= 16) boot_resample<16><<<grid, BT_TH, 0, s>>>(d);
  else if (d.M <= 20) boot_resample<20><<<grid, BT_TH, 0, s>>>(d);
  else if (d.M <= 24) boot_resample<24><<<grid, BT_TH, 0, s>>>(d);
  else if (d.M <= 28) boot_resample<28><<<grid, BT_TH, 0, s>>>(d);
  else boot_resample<BOOT_MAX_M><<<grid, BT_TH, 0, s>>>(d);
}
