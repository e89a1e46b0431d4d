// Rank-based uncertainty metrics (eval.py --rank_metrics): a stable key sort, midranks, and fp64 prefix sums taken in sorted order
// at K + 1 cut positions.  Sparsification curves, AUSE / AURG, reliability tables, the threshold table and Spearman's rho are all
// derived on the host from what this file writes (poco_amd/ranking.py).  The contract is stated in include/poco_hip.h
// (poco_op_rank_curve, poco_op_pearson64) and DESIGN.md section 27; tests/rank_np.py restates it in float64 with plain loops.
//
// Everything works on tiles of RANK_TILE consecutive positions; a block of RANK_THREADS lanes takes tiles by a grid-stride loop,
// and whatever a tile computes is a function of that tile alone, so no result depends on the grid.
//
//   sort      four passes of a least-significant-digit radix sort, 8 bits each, on the order-preserving uint32 image of the key
//             (rank_key_map) with the row index as payload.  A pass is three launches:
//               rank_hist      per tile, the 256-bin digit histogram -> hist[digit][tile]
//               rank_row_scan  per digit, the exclusive scan of its row of hist in place, and the row's total
//               rank_scatter   per tile: digit bases (a 256-entry scan of the totals) + the row scan's entry + the counts of the
//                              waves before this one in the tile + the lane's rank among its wave's equal digits
//             Inside a tile wave w owns the positions [512 w, 512 (w + 1)) and walks them 64 at a time in order.  The lanes of
//             one step that hold the same digit find each other with eight ballots (match_digit); the lowest of them is the
//             group's leader and is the only lane that adds the group's size to the wave's counter of that digit in LDS.  Earlier
//             positions therefore always land before later ones with the same digit: the pass is stable.
//   midranks  head flags on the sorted keys; rank_tile_reduce leaves per tile the last group start and the first group end in
//             it, rank_tile_scan carries them across tiles (forward max, backward min), rank_apply scans inside the tile and
//             scatters (start + end) / 2 + 1 back through the order.  A tie group may span any number of tiles.
//   cuts      prefix(c) = tprefix[c / T] + partial(tile c / T, c % T): partial is a strided per-lane sum followed by a halving
//             tree over the 256 lanes, tprefix the scan of the full tiles' totals by one block of 1024 lanes (contiguous runs per
//             lane, then a Hillis-Steele scan).  The tree that forms prefix(c) is a function of c and n alone.
//
// LDS: rank_scatter holds 4 x 256 wave counters and a 256-entry scan line, 5 KB; nothing else exceeds 8 KB.  No floating-point
// atomics anywhere; the only additions into shared counters are integer ones made by one lane per digit and wave.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"

#include <cstdint>

namespace {

constexpr int RK_T = RANK_TILE;
constexpr int RK_WAVES = RANK_THREADS / 64;
constexpr int RK_SEG = RK_T / RK_WAVES;                  // positions of a tile that one wave owns
constexpr int RK_STEPS = RK_SEG / 64;
constexpr int RK_PER = RK_T / RANK_THREADS;              // consecutive positions per lane in rank_apply
constexpr int RK_SCAN_THREADS = 1024;
constexpr int RK_INT_MAX = 0x7fffffff;
static_assert(RANK_THREADS == 256 && RK_T % RANK_THREADS == 0 && RK_SEG % 64 == 0, "a digit per lane, whole steps per wave");

// -0.0 -> +0.0, every NaN -> 0x7fc00000, then the usual order-preserving image: negative keys are complemented, the others get
// their sign bit set.  +NaN maps to 0xffc00000, above +inf (0xff800000): NaN sorts last, as numpy sorts it.
__device__ __forceinline__ uint32_t rank_key_map(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rank_key_unmap(uint32_t m) {
  return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

// The lanes of this wave that are valid and hold the digit `d`.  Every lane of the wave must call it.
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool valid) {
  unsigned long long peers = __ballot(valid);
  #pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    peers &= bit ? bal : ~bal;
  }
  return peers;
}

struct SortIn {
  const float* key;          // pass 0: the caller's keys, the payload is the position itself
  const uint32_t* kin;       // later passes: mapped keys and payload of the pass before
  const int32_t* oin;
  long long n;
  int NT, shift;
};

template <bool FIRST>
__device__ __forceinline__ uint32_t load_mapped(const SortIn& a, long long p) {
  return FIRST ? rank_key_map(__float_as_uint(a.key[p])) : a.kin[p];
}

// wh[d] += the number of positions with digit d among this wave's share of the tile.  wh = this wave's 256 counters, zeroed.
template <bool FIRST>
__device__ __forceinline__ void wave_hist(const SortIn& a, long long tile0, volatile uint32_t* wh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < RK_STEPS; ++c) {
    const long long p = tile0 + wave * RK_SEG + c * 64 + lane;
    const bool valid = p < a.n;
    const uint32_t d = valid ? (load_mapped<FIRST>(a, p) >> a.shift) & 255u : 0u;
    const unsigned long long peers = match_digit(d, valid);
    if (valid && lane == __ffsll((long long)peers) - 1) wh[d] = wh[d] + (uint32_t)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
}

// Exclusive scan of one uint32 per lane over the 256 lanes of the block; `total` = the sum.  sh = 256 words.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < RANK_THREADS; o <<= 1) {
    const uint32_t x = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  total = sh[RANK_THREADS - 1];
  __syncthreads();
  return incl - v;
}

template <bool FIRST>
__global__ __launch_bounds__(RANK_THREADS) void rank_hist(SortIn a, uint32_t* __restrict__ hist) {
  __shared__ uint32_t wh[RK_WAVES][256];
  const int t = threadIdx.x;
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    #pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) wh[w][t] = 0u;
    __syncthreads();
    wave_hist<FIRST>(a, (long long)tile * RK_T, wh[t >> 6]);
    __syncthreads();
    uint32_t s = 0;
    #pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) s += wh[w][t];
    hist[(size_t)t * a.NT + tile] = s;
    __syncthreads();
  }
}

// hist[d][0..NT) -> its exclusive scan, totals[d] = the row's sum.  One block per digit at a time.
__global__ __launch_bounds__(RANK_THREADS) void rank_row_scan(uint32_t* __restrict__ hist, uint32_t* __restrict__ totals, int NT) {
  __shared__ uint32_t sh[RANK_THREADS];
  const int t = threadIdx.x;
  for (int d = blockIdx.x; d < 256; d += gridDim.x) {
    uint32_t* row = hist + (size_t)d * NT;
    uint32_t carry = 0;
    for (int base = 0; base < NT; base += RANK_THREADS) {
      const int i = base + t;
      const uint32_t v = i < NT ? row[i] : 0u;
      uint32_t total;
      const uint32_t ex = block_excl_scan(v, sh, total);
      if (i < NT) row[i] = carry + ex;
      carry += total;
    }
    if (t == 0) totals[d] = carry;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(RANK_THREADS) void rank_scatter(SortIn a, const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals,
                                                             uint32_t* __restrict__ kout, int32_t* __restrict__ oout) {
  __shared__ uint32_t wh[RK_WAVES][256];
  __shared__ uint32_t sh[RANK_THREADS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t all;
  const uint32_t dbase = block_excl_scan(totals[t], sh, all);          // first sorted position of digit t
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    const long long tile0 = (long long)tile * RK_T;
    #pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) wh[w][t] = 0u;
    __syncthreads();
    wave_hist<FIRST>(a, tile0, wh[wave]);
    __syncthreads();
    uint32_t base = dbase + hist[(size_t)t * a.NT + tile];             // counts -> the first position each wave writes digit t to
    #pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) {
      const uint32_t c = wh[w][t];
      wh[w][t] = base;
      base += c;
    }
    __syncthreads();
    volatile uint32_t* mine = wh[wave];
    for (int c = 0; c < RK_STEPS; ++c) {
      const long long p = tile0 + wave * RK_SEG + c * 64 + lane;
      const bool valid = p < a.n;
      const uint32_t m = valid ? load_mapped<FIRST>(a, p) : 0u;
      const int32_t idx = valid ? (FIRST ? (int32_t)p : a.oin[p]) : 0;
      const uint32_t d = (m >> a.shift) & 255u;
      const unsigned long long peers = match_digit(d, valid);
      const uint32_t first = mine[d];
      __builtin_amdgcn_wave_barrier();                                 // every lane has read before a leader writes
      const uint32_t pos = first + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
      if (valid && (long long)pos < a.n) {
        kout[pos] = m;
        oout[pos] = idx;
      }
      if (valid && lane == __ffsll((long long)peers) - 1) mine[d] = first + (uint32_t)__popcll(peers);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
}

// ---- what follows reads the sorted keys (mapped) and the order ---------------------------------------------------------------------
struct CurveDev {
  const uint32_t* skey;      // [n] sorted, mapped
  const int32_t* order;      // [n]
  const float* vals;         // [E][n] or null
  long long n;
  int NT, E, K;
  int32_t *last_head, *first_end, *fwd, *bwd;      // [NT] each
  double *tsum, *tprefix;                          // [E + 1][NT], [E + 1][NT + 1]
};

__device__ __forceinline__ double plane_at(const CurveDev& a, int e, long long p) {
  if (e == 0) return (double)rank_key_unmap(a.skey[p]);
  const uint32_t row = (uint32_t)a.order[p];
  return (long long)row < a.n ? (double)a.vals[(size_t)(e - 1) * (size_t)a.n + row] : 0.0;
}

// Sum of plane e over the first r positions of the tile that starts at tile0: lane t adds positions t, t + 256, ... in order,
// then a halving tree over the lanes.  Every lane of the block must call it with the same arguments.  red = 256 doubles.
__device__ __forceinline__ double tile_partial(const CurveDev& a, int e, long long tile0, int r, double* red) {
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < r; i += RANK_THREADS) acc = acc + plane_at(a, e, tile0 + i);
  red[t] = acc;
  __syncthreads();
  for (int o = RANK_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = red[t] + red[t + o];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__device__ __forceinline__ bool is_head(const CurveDev& a, long long p) { return p == 0 || a.skey[p] != a.skey[p - 1]; }
__device__ __forceinline__ bool is_end(const CurveDev& a, long long p) { return p == a.n - 1 || a.skey[p + 1] != a.skey[p]; }

__global__ __launch_bounds__(RANK_THREADS) void rank_tile_reduce(CurveDev a) {
  __shared__ double red[RANK_THREADS];
  __shared__ int32_t imax[RANK_THREADS], imin[RANK_THREADS];
  const int t = threadIdx.x;
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    const long long tile0 = (long long)tile * RK_T;
    const long long left = a.n - tile0;
    const int r = (int)(left < RK_T ? left : RK_T);
    int32_t hi = -1, lo = RK_INT_MAX;
    for (int i = t; i < r; i += RANK_THREADS) {
      const long long p = tile0 + i;
      if (is_head(a, p) && (int32_t)p > hi) hi = (int32_t)p;
      if (is_end(a, p) && (int32_t)p < lo) lo = (int32_t)p;
    }
    imax[t] = hi; imin[t] = lo;
    __syncthreads();
    for (int o = RANK_THREADS / 2; o > 0; o >>= 1) {
      if (t < o) {
        if (imax[t + o] > imax[t]) imax[t] = imax[t + o];
        if (imin[t + o] < imin[t]) imin[t] = imin[t + o];
      }
      __syncthreads();
    }
    if (t == 0) { a.last_head[tile] = imax[0]; a.first_end[tile] = imin[0]; }
    __syncthreads();
    for (int e = 0; e <= a.E; ++e) {
      const double s = tile_partial(a, e, tile0, r, red);
      if (t == 0) a.tsum[(size_t)e * a.NT + tile] = s;
    }
  }
}

// One block: tprefix[e][j] = sum of the totals of tiles < j (j = 0..NT), fwd[j] = the last group start in tiles < j (-1: none),
// bwd[j] = the first group end in tiles > j.  Lane t owns the run of C = ceil(NT / 1024) tiles from t C on.
__global__ __launch_bounds__(RK_SCAN_THREADS) void rank_tile_scan(CurveDev a) {
  __shared__ double shd[RK_SCAN_THREADS];
  __shared__ int32_t shi[RK_SCAN_THREADS];
  const int t = threadIdx.x, NT = a.NT;
  const int C = (NT + RK_SCAN_THREADS - 1) / RK_SCAN_THREADS;
  const int j0 = t * C < NT ? t * C : NT, j1 = j0 + C < NT ? j0 + C : NT;
  for (int e = 0; e <= a.E; ++e) {
    const double* ts = a.tsum + (size_t)e * NT;
    double* tp = a.tprefix + (size_t)e * (NT + 1);
    double s = 0.0;
    for (int j = j0; j < j1; ++j) s = s + ts[j];
    shd[t] = s;
    __syncthreads();
    for (int o = 1; o < RK_SCAN_THREADS; o <<= 1) {
      const double x = t >= o ? shd[t - o] : 0.0;
      __syncthreads();
      if (t >= o) shd[t] = shd[t] + x;
      __syncthreads();
    }
    double run = t > 0 ? shd[t - 1] : 0.0;
    __syncthreads();
    for (int j = j0; j < j1; ++j) { tp[j] = run; run = run + ts[j]; }
    if (j1 == NT && j0 < NT) tp[NT] = run;
  }
  // forward: the last group start before tile j
  {
    int32_t m = -1;
    for (int j = j0; j < j1; ++j) m = a.last_head[j] > m ? a.last_head[j] : m;
    shi[t] = m;
    __syncthreads();
    for (int o = 1; o < RK_SCAN_THREADS; o <<= 1) {
      const int32_t x = t >= o ? shi[t - o] : -1;
      __syncthreads();
      if (x > shi[t]) shi[t] = x;
      __syncthreads();
    }
    int32_t run = t > 0 ? shi[t - 1] : -1;
    __syncthreads();
    for (int j = j0; j < j1; ++j) { a.fwd[j] = run; run = a.last_head[j] > run ? a.last_head[j] : run; }
  }
  // backward: the same walk over the tiles in reverse, tile NT - 1 - j in place of j
  {
    int32_t m = RK_INT_MAX;
    for (int j = j0; j < j1; ++j) { const int32_t v = a.first_end[NT - 1 - j]; m = v < m ? v : m; }
    shi[t] = m;
    __syncthreads();
    for (int o = 1; o < RK_SCAN_THREADS; o <<= 1) {
      const int32_t x = t >= o ? shi[t - o] : RK_INT_MAX;
      __syncthreads();
      if (x < shi[t]) shi[t] = x;
      __syncthreads();
    }
    int32_t run = t > 0 ? shi[t - 1] : RK_INT_MAX;
    __syncthreads();
    for (int j = j0; j < j1; ++j) { const int32_t v = a.first_end[NT - 1 - j]; a.bwd[NT - 1 - j] = run; run = v < run ? v : run; }
  }
}

// rank[order[p]] = (start(p) + end(p)) / 2 + 1 with start / end the first / last sorted position of p's tie group.  Lane t owns the
// RK_PER consecutive positions from tile0 + t RK_PER on.
__global__ __launch_bounds__(RANK_THREADS) void rank_apply(CurveDev a, double* __restrict__ rank) {
  __shared__ int32_t sf[RANK_THREADS], sb[RANK_THREADS];
  const int t = threadIdx.x;
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    const long long p0 = (long long)tile * RK_T + (long long)t * RK_PER;
    int32_t start[RK_PER], end[RK_PER];
    int32_t run = -1;
    #pragma unroll
    for (int i = 0; i < RK_PER; ++i) {
      const long long p = p0 + i;
      if (p < a.n && is_head(a, p)) run = (int32_t)p;
      start[i] = run;
    }
    sf[t] = run;
    run = RK_INT_MAX;
    #pragma unroll
    for (int i = RK_PER - 1; i >= 0; --i) {
      const long long p = p0 + i;
      if (p < a.n && is_end(a, p)) run = (int32_t)p;
      end[i] = run;
    }
    sb[t] = run;
    __syncthreads();
    for (int o = 1; o < RANK_THREADS; o <<= 1) {                       // inclusive: max over lanes <= t, min over lanes >= t
      const int32_t xf = t >= o ? sf[t - o] : -1;
      const int32_t xb = t + o < RANK_THREADS ? sb[t + o] : RK_INT_MAX;
      __syncthreads();
      if (xf > sf[t]) sf[t] = xf;
      if (xb < sb[t]) sb[t] = xb;
      __syncthreads();
    }
    int32_t before = a.fwd[tile], after = a.bwd[tile];
    if (t > 0 && sf[t - 1] > before) before = sf[t - 1];
    if (t + 1 < RANK_THREADS && sb[t + 1] < after) after = sb[t + 1];
    #pragma unroll
    for (int i = 0; i < RK_PER; ++i) {
      const long long p = p0 + i;
      if (p < a.n) {
        const int32_t s = start[i] > before ? start[i] : before;
        const int32_t e = end[i] < after ? end[i] : after;
        const uint32_t row = (uint32_t)a.order[p];
        if ((long long)row < a.n) rank[row] = ((double)s + (double)e + 2.0) * 0.5;
      }
    }
    __syncthreads();
  }
}

// cuts[e][k] = prefix of plane e at c_k = floor(k n / K); cut_keys[k] = the sorted key at max(c_k, 1) - 1.
__global__ __launch_bounds__(RANK_THREADS) void rank_cuts(CurveDev a, double* __restrict__ cuts, float* __restrict__ cut_keys) {
  __shared__ double red[RANK_THREADS];
  const int planes = a.E + 1, items = (a.K + 1) * planes;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int k = w / planes, e = w % planes;
    const long long c = (long long)k * a.n / a.K;
    const int j = (int)(c / RK_T), r = (int)(c % RK_T);
    double v = a.tprefix[(size_t)e * (a.NT + 1) + j];
    if (r > 0) v = v + tile_partial(a, e, (long long)j * RK_T, r, red);
    if (threadIdx.x == 0) {
      cuts[(size_t)e * (a.K + 1) + k] = v;
      if (e == 0) cut_keys[k] = rank_key_unmap(a.skey[(c > 1 ? c : 1) - 1]);
    }
  }
}

// ---- Pearson's r of two fp64 arrays: one block, two walks (means, then centred sums), fixed order --------------------------------
__global__ __launch_bounds__(RK_SCAN_THREADS) void pearson64_kernel(const double* __restrict__ x, const double* __restrict__ y, long long n,
                                                                    double* __restrict__ out) {
  #pragma clang fp contract(off)
  __shared__ double red[RK_SCAN_THREADS];
  __shared__ int flat[2];
  const int t = threadIdx.x;
  if (t < 2) flat[t] = 1;
  __syncthreads();
  double sx = 0.0, sy = 0.0;
  const double x0 = x[0], y0 = y[0];
  bool cx = true, cy = true;                                           // every element seen so far equals the first one
  for (long long i = t; i < n; i += RK_SCAN_THREADS) {
    const double a = x[i], b = y[i];
    sx = sx + a; sy = sy + b;
    cx = cx && a == x0; cy = cy && b == y0;
  }
  if (!cx) flat[0] = 0;                                                // racing stores of the same value
  if (!cy) flat[1] = 0;
  sx = block_tree_sum<RK_SCAN_THREADS>(sx, red); sy = block_tree_sum<RK_SCAN_THREADS>(sy, red);
  const double mx = sx / (double)n, my = sy / (double)n;
  double cxx = 0.0, cyy = 0.0, cxy = 0.0;
  for (long long i = t; i < n; i += RK_SCAN_THREADS) {
    const double a = x[i] - mx, b = y[i] - my;
    cxx = cxx + a * a; cyy = cyy + b * b; cxy = cxy + a * b;
  }
  cxx = block_tree_sum<RK_SCAN_THREADS>(cxx, red); cyy = block_tree_sum<RK_SCAN_THREADS>(cyy, red);
  cxy = block_tree_sum<RK_SCAN_THREADS>(cxy, red);
  if (t == 0) {
    double r = cxy / (sqrt(cxx) * sqrt(cyy));
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);                         // a NaN stays a NaN
    if (flat[0] || flat[1]) r = __longlong_as_double(0x7ff8000000000000ll);
    out[0] = r;
  }
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

RankScratch rank_scratch_layout(long long n, int E) {
  RankScratch L{};
  const size_t NT = (size_t)((n + RK_T - 1) / RK_T), planes = (size_t)E + 1;
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
  L.NT = (int)NT;
  L.key_a = take((size_t)n * 4); L.key_b = take((size_t)n * 4); L.order_a = take((size_t)n * 4);
  L.hist = take(256 * NT * 4); L.totals = take(256 * 4);
  L.last_head = take(NT * 4); L.first_end = take(NT * 4); L.fwd = take(NT * 4); L.bwd = take(NT * 4);
  L.tsum = take(planes * NT * 8); L.tprefix = take(planes * (NT + 1) * 8);
  L.bytes = off;
  return L;
}

void launch_rank_curve(const float* key, const float* vals, long long n, int E, int K, void* scratch, int32_t* order, double* rank,
                       double* cuts, float* cut_keys, int max_blocks, hipStream_t s) {
  const RankScratch L = rank_scratch_layout(n, E);
  char* base = static_cast<char*>(scratch);
  uint32_t* key_a = reinterpret_cast<uint32_t*>(base + L.key_a);
  uint32_t* key_b = reinterpret_cast<uint32_t*>(base + L.key_b);
  int32_t* order_a = reinterpret_cast<int32_t*>(base + L.order_a);
  uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
  uint32_t* totals = reinterpret_cast<uint32_t*>(base + L.totals);
  const int cap = max_blocks > 0 && max_blocks < RANK_MAX_BLOCKS ? max_blocks : RANK_MAX_BLOCKS;
  const int tiles = L.NT < cap ? L.NT : cap, rows = 256 < cap ? 256 : cap;
  // keys, payload -> keys, payload: (caller's, position) -> (a, a) -> (b, order) -> (a, a) -> (b, order)
  const SortIn in[4] = {{key, nullptr, nullptr, n, L.NT, 0}, {nullptr, key_a, order_a, n, L.NT, 8}, {nullptr, key_b, order, n, L.NT, 16},
                        {nullptr, key_a, order_a, n, L.NT, 24}};
  uint32_t* const kout[4] = {key_a, key_b, key_a, key_b};
  int32_t* const oout[4] = {order_a, order, order_a, order};
  rank_hist<true><<<tiles, RANK_THREADS, 0, s>>>(in[0], hist);
  rank_row_scan<<<rows, RANK_THREADS, 0, s>>>(hist, totals, L.NT);
  rank_scatter<true><<<tiles, RANK_THREADS, 0, s>>>(in[0], hist, totals, kout[0], oout[0]);
  for (int pass = 1; pass < 4; ++pass) {
    rank_hist<false><<<tiles, RANK_THREADS, 0, s>>>(in[pass], hist);
    rank_row_scan<<<rows, RANK_THREADS, 0, s>>>(hist, totals, L.NT);
    rank_scatter<false><<<tiles, RANK_THREADS, 0, s>>>(in[pass], hist, totals, kout[pass], oout[pass]);
  }
  const CurveDev d{key_b, order, vals, n, L.NT, E, K,
                   reinterpret_cast<int32_t*>(base + L.last_head), reinterpret_cast<int32_t*>(base + L.first_end),
                   reinterpret_cast<int32_t*>(base + L.fwd), reinterpret_cast<int32_t*>(base + L.bwd),
                   reinterpret_cast<double*>(base + L.tsum), reinterpret_cast<double*>(base + L.tprefix)};
  rank_tile_reduce<<<tiles, RANK_THREADS, 0, s>>>(d);
  rank_tile_scan<<<1, RK_SCAN_THREADS, 0, s>>>(d);
  rank_apply<<<tiles, RANK_THREADS, 0, s>>>(d, rank);
  const int items = (K + 1) * (E + 1);
  rank_cuts<<<items < cap ? items : cap, RANK_THREADS, 0, s>>>(d, cuts, cut_keys);
}

void launch_pearson64(const double* x, const double* y, long long n, double* r, hipStream_t s) {
  pearson64_kernel<<<1, RK_SCAN_THREADS, 0, s>>>(x, y, n, r);
}
