// Calibration of the uncertainty (eval.py --calibrate, demo.py --calibration): isotonic regression of S ragged segments in one call, and
// the fitted maps evaluated on new uncertainties.  The contract is stated in include/poco_hip.h (poco_op_isotonic,
// poco_op_calib_apply) and DESIGN.md section 33; tests/calib_np.py restates both with plain loops and a stack.
//
// Everything is indexed by POSITION in the ragged buffer, p in [0, N).  A block of the fit is a range of positions that starts at a
// unit head; it is described at its two ends:   at its first position h:  sum[h] (fp64), len[h] (rows; 0 = "h starts no block")
//                                               at its last position e:   head[e] = h, lsum[e] = sum[h]
// so a walk to the right reads (sum, len) at the next head and a walk to the left reads (head, lsum) at the position before the
// current start: one round trip per step either way.  flags[p] bit 0 = p starts a unit, bit 1 = p starts a segment.
//
//   gather    ys[p] = y[order[p]], the mapped key, the flags (the segment of p by a binary search of seg_offsets), len[p] = 0
//   units     a segmented sum over tiles of ISO_TILE positions: iso_seg_reduce leaves per tile its first and last head, its number
//             of heads and the sum of the positions before its first head (the part of a unit that began in an earlier tile);
//             iso_seg_scan (one block) carries these across tiles; iso_seg_apply scans inside the tile (8 positions per lane, then
//             a Hillis-Steele scan over the 256 lanes) and writes every unit at its two ends.  A unit may span any number of tiles.
//   nh        nh[p] = the first unit head at or after p.  The fit works on a binary tree over the POSITIONS [0, 2^L): the node
//             [a, b) owns the units whose head lies in it, the positions [nh[a], nh[b]).  Units are never cut, whatever the tree.
//   merges    level l joins the two fitted children of every node of 2^(l+1) positions: iso_merge_node looks at the one boundary
//             m = nh[a + 2^l] between them.  If m starts a segment, or the means on its two sides are ordered, nothing happens.
//             Otherwise the two blocks pool, and the pooled block absorbs its left neighbour while mean_left >= mean, its right
//             neighbour while mean >= mean_right, until neither (one lane per node; a `for` of at most hi - lo trips).  A merge
//             only ever pools across its boundary, and a block that is absorbed is never looked at again, so the absorptions over
//             all levels number at most the units.  Levels 0..10 (nodes inside one tile) run in ONE launch, a block per tile with a
//             block barrier between levels; every level above is a launch.
//   values    the same segmented sum with "len[p] > 0" as the head flag: the block's mean from its own rows, the block's first
//             position for every position, the blocks' ranks (a scan of the head counts) and the knot table; iso_fill spreads the
//             mean over the block, iso_seg_blocks looks up the rank at every segment's start.
//
// No floating-point atomics, no spin-wait, no grid barrier; nothing depends on the grid: what a tile or a node computes is a function
// of that tile or node alone.  LDS: iso_seg_apply 13 KB, iso_seg_scan 16 KB, the others less.
#include "common.h"
#include "kernels.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int IS_T = ISO_TILE;
constexpr int IS_TH = ISO_THREADS;
constexpr int IS_PER = IS_T / IS_TH;                     // consecutive positions per lane in iso_seg_apply
constexpr int IS_LOW = 11;                               // levels 0..IS_LOW-1 join nodes inside one tile
constexpr int IS_SCAN = 1024;
constexpr int IS_INT_MAX = 0x7fffffff;
static_assert((1 << IS_LOW) == IS_T && IS_T % IS_TH == 0, "the fused levels end at the tile");

struct IsoDev {
  const float* key;          // [M]
  const float* y;            // [M]
  const int32_t* order;      // [N]
  const int32_t* seg;        // [S + 1]
  int M, N, S, NT;
  float* ys;                 // [N] y in position order
  uint32_t* ukey;            // [N] mapped canonical key
  uint8_t* flags;            // [N]
  double *sum, *lsum;        // [N]; after the merges sum[h] is reused for the block's mean
  int32_t *len, *head, *nh;  // [N]; after the merges nh[h] is reused for the block's rank
  double *cp, *after;        // [NT]
  int32_t *fh, *lh, *fwd, *bwd, *nheads, *hbase, *total;   // [NT] each, total [1]
  int32_t* block;            // outputs
  double* fit;
  int32_t* seg_blocks;
  double* knots;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the order-preserving uint32 image of a canonical key (rank_curve.hip: rank_key_map / rank_key_unmap)
__device__ __forceinline__ uint32_t iso_key_map(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float iso_key_unmap(uint32_t m) { return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m); }

__global__ __launch_bounds__(IS_TH) void iso_gather(IsoDev a) {
  for (long long q = (long long)blockIdx.x * IS_TH + threadIdx.x; q < a.N; q += (long long)gridDim.x * IS_TH) {
    const int p = (int)q;
    const int r = clampi(a.order[p], 0, a.M - 1);
    const uint32_t k = iso_key_map(__float_as_uint(a.key[r]));
    int lo = 0, hi = a.S;                                              // the last s in [0, S) with seg[s] <= p
    for (int it = 0; it < 13 && hi - lo > 1; ++it) {
      const int mid = (lo + hi) >> 1;
      if (clampi(a.seg[mid], 0, a.N) <= p) lo = mid; else hi = mid;
    }
    const bool start = p == 0 || clampi(a.seg[lo], 0, a.N) == p;
    bool unit = start;
    if (!unit) unit = iso_key_map(__float_as_uint(a.key[clampi(a.order[p - 1], 0, a.M - 1)])) != k;
    a.ys[p] = a.y[r];
    a.ukey[p] = k;
    a.flags[p] = (uint8_t)((unit ? 1 : 0) | (start ? 2 : 0));
    a.len[p] = 0;
  }
}

// UNITS: a head is the start of a unit.  Otherwise: the start of a fitted block.
template <bool UNITS>
__device__ __forceinline__ bool iso_is_head(const IsoDev& a, int p) { return UNITS ? (a.flags[p] & 1) != 0 : a.len[p] > 0; }

template <bool UNITS>
__global__ __launch_bounds__(IS_TH) void iso_seg_reduce(IsoDev a) {
  __shared__ double red[IS_TH];
  __shared__ int32_t imin[IS_TH], imax[IS_TH], icnt[IS_TH];
  const int t = threadIdx.x;
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    const int tile0 = tile * IS_T;
    const int r = a.N - tile0 < IS_T ? a.N - tile0 : IS_T;
    int32_t lo = IS_INT_MAX, hi = -1, c = 0;
    for (int i = t; i < r; i += IS_TH) {
      const int p = tile0 + i;
      if (iso_is_head<UNITS>(a, p)) { lo = p < lo ? p : lo; hi = p > hi ? p : hi; ++c; }
    }
    imin[t] = lo; imax[t] = hi; icnt[t] = c;
    __syncthreads();
    for (int o = IS_TH / 2; o > 0; o >>= 1) {
      if (t < o) {
        if (imin[t + o] < imin[t]) imin[t] = imin[t + o];
        if (imax[t + o] > imax[t]) imax[t] = imax[t + o];
        icnt[t] += icnt[t + o];
      }
      __syncthreads();
    }
    const int32_t first = imin[0];
    double acc = 0.0;                                                  // the positions before the tile's first head
    for (int i = t; i < r && tile0 + i < first; i += IS_TH) acc = acc + (double)a.ys[tile0 + i];
    red[t] = acc;
    __syncthreads();
    for (int o = IS_TH / 2; o > 0; o >>= 1) {
      if (t < o) red[t] = red[t] + red[t + o];
      __syncthreads();
    }
    if (t == 0) { a.fh[tile] = first; a.lh[tile] = imax[0]; a.nheads[tile] = icnt[0]; a.cp[tile] = red[0]; }
    __syncthreads();
  }
}

// One block.  fwd[j] = the last head in tiles < j (-1: none), bwd[j] = the first head in tiles > j (N: none), hbase[j] = the heads in
// tiles < j, total[0] = all heads, after[j] = the sum of cp over the tiles after j up to and including the first that holds a head.
// Lane t owns the run of C = ceil(NT / 1024) tiles from t C on.
__global__ __launch_bounds__(IS_SCAN) void iso_seg_scan(IsoDev a) {
  __shared__ double shd[IS_SCAN];
  __shared__ int32_t shi[IS_SCAN], shc[IS_SCAN];
  const int t = threadIdx.x, NT = a.NT;
  const int C = (NT + IS_SCAN - 1) / IS_SCAN;
  const int j0 = t * C < NT ? t * C : NT, j1 = j0 + C < NT ? j0 + C : NT;
  {                                                                    // forward: max of the last heads, sum of the head counts
    int32_t m = -1, c = 0;
    for (int j = j0; j < j1; ++j) { m = a.lh[j] > m ? a.lh[j] : m; c += a.nheads[j]; }
    shi[t] = m; shc[t] = c;
    __syncthreads();
    for (int o = 1; o < IS_SCAN; o <<= 1) {
      const int32_t x = t >= o ? shi[t - o] : -1, xc = t >= o ? shc[t - o] : 0;
      __syncthreads();
      if (x > shi[t]) shi[t] = x;
      shc[t] += xc;
      __syncthreads();
    }
    int32_t run = t > 0 ? shi[t - 1] : -1, cnt = t > 0 ? shc[t - 1] : 0;
    if (t == IS_SCAN - 1) a.total[0] = shc[t];
    __syncthreads();
    for (int j = j0; j < j1; ++j) {
      a.fwd[j] = run; a.hbase[j] = cnt;
      run = a.lh[j] > run ? a.lh[j] : run; cnt += a.nheads[j];
    }
  }
  {                                                                    // backward: min of the first heads
    int32_t m = IS_INT_MAX;
    for (int j = j0; j < j1; ++j) m = a.fh[j] < m ? a.fh[j] : m;
    shi[t] = m;
    __syncthreads();
    for (int o = 1; o < IS_SCAN; o <<= 1) {
      const int32_t x = t + o < IS_SCAN ? shi[t + o] : IS_INT_MAX;
      __syncthreads();
      if (x < shi[t]) shi[t] = x;
      __syncthreads();
    }
    int32_t run = t + 1 < IS_SCAN ? shi[t + 1] : IS_INT_MAX;
    __syncthreads();
    for (int j = j1 - 1; j >= j0; --j) { a.bwd[j] = run < a.N ? run : a.N; run = a.fh[j] < run ? a.fh[j] : run; }
  }
  {                                                                    // backward, segmented: (s1, c1) + (s2, c2) = c1 ? (s1, 1) : (s1 + s2, c2)
    double s = 0.0; int32_t closed = 0;
    for (int j = j1 - 1; j >= j0; --j) {
      const bool cj = a.fh[j] != IS_INT_MAX;
      s = cj ? a.cp[j] : a.cp[j] + s;
      closed = cj ? 1 : closed;
    }
    shd[t] = s; shc[t] = closed;
    __syncthreads();
    for (int o = 1; o < IS_SCAN; o <<= 1) {
      const double xs = t + o < IS_SCAN ? shd[t + o] : 0.0;
      const int32_t xc = t + o < IS_SCAN ? shc[t + o] : 0;
      __syncthreads();
      if (!shc[t]) { shd[t] = shd[t] + xs; shc[t] = xc; }
      __syncthreads();
    }
    s = t + 1 < IS_SCAN ? shd[t + 1] : 0.0;
    closed = t + 1 < IS_SCAN ? shc[t + 1] : 0;
    __syncthreads();
    for (int j = j1 - 1; j >= j0; --j) {
      a.after[j] = s;
      const bool cj = a.fh[j] != IS_INT_MAX;
      s = cj ? a.cp[j] : a.cp[j] + s;
      closed = cj ? 1 : closed;
    }
  }
}

// Per tile: block[p] = the head at or before p; every head's total = the scanned sum at its last position inside the tile (+ after[tile]
// if it runs on), written at the unit's two ends (UNITS) or as the block's mean, rank and knot row.  Lane t owns the IS_PER positions
// from tile0 + t IS_PER on.
template <bool UNITS>
__global__ __launch_bounds__(IS_TH) void iso_seg_apply(IsoDev a) {
  __shared__ double shs[IS_TH];
  __shared__ int32_t shf[IS_TH], shm[IS_TH], shc[IS_TH];
  __shared__ int32_t rk[IS_T];
  const int t = threadIdx.x;
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    const int tile0 = tile * IS_T, p0 = tile0 + t * IS_PER;
    const int tile_end = a.N - tile0 < IS_T ? a.N : tile0 + IS_T;
    double v[IS_PER];
    int32_t hb[IS_PER];
    double run = 0.0;
    int32_t seen = 0, mh = -1, cnt = 0;
    #pragma unroll
    for (int i = 0; i < IS_PER; ++i) {
      const int p = p0 + i;
      if (p < tile_end) {
        const double y = (double)a.ys[p];
        if (iso_is_head<UNITS>(a, p)) { run = y; seen = 1; mh = p; rk[p - tile0] = cnt; ++cnt; }
        else run = run + y;
      }
      v[i] = run; hb[i] = mh;
    }
    shs[t] = run; shf[t] = seen; shm[t] = mh; shc[t] = cnt;
    __syncthreads();
    for (int o = 1; o < IS_TH; o <<= 1) {
      const double xs = t >= o ? shs[t - o] : 0.0;
      const int32_t xf = t >= o ? shf[t - o] : 0, xm = t >= o ? shm[t - o] : -1, xc = t >= o ? shc[t - o] : 0;
      __syncthreads();
      if (t >= o) {
        if (!shf[t]) shs[t] = xs + shs[t];
        shf[t] |= xf;
        if (xm > shm[t]) shm[t] = xm;
        shc[t] += xc;
      }
      __syncthreads();
    }
    const double ps = t > 0 ? shs[t - 1] : 0.0;
    int32_t pm = a.fwd[tile];
    if (t > 0 && shm[t - 1] > pm) pm = shm[t - 1];
    const int32_t pc = a.hbase[tile] + (t > 0 ? shc[t - 1] : 0);
    #pragma unroll
    for (int i = 0; i < IS_PER; ++i) {
      const int p = p0 + i;
      if (p < tile_end) {
        if (hb[i] < 0) v[i] = ps + v[i];                               // no head in this lane's run so far: the run began before it
        else if (hb[i] == p) rk[p - tile0] += pc;
        if (hb[i] < pm) hb[i] = pm;
        if (hb[i] < 0) hb[i] = 0;                                      // position 0 is a head by construction
        a.block[p] = hb[i];
      }
    }
    __syncthreads();
    const int32_t next_tile_head = a.bwd[tile];
    const double after = a.after[tile];
    #pragma unroll
    for (int i = 0; i < IS_PER; ++i) {
      const int p = p0 + i;
      if (p < tile_end && hb[i] >= tile0) {
        const int nxt = p + 1;
        if (nxt == tile_end || iso_is_head<UNITS>(a, nxt)) {           // p is the last position of its block inside this tile
          const int h = hb[i];
          const int next_head = nxt < tile_end ? nxt : next_tile_head;
          double total = v[i];
          if (next_head > tile_end) total = total + after;
          const int rows = next_head - h, last = next_head - 1;
          if (UNITS) {
            a.sum[h] = total; a.len[h] = rows; a.head[last] = h; a.lsum[last] = total;
          } else {
            const double mean = total / (double)rows;
            const int32_t b = rk[h - tile0];
            a.sum[h] = mean;
            a.nh[h] = b;
            if (b >= 0 && b < a.N) {
              double* kn = a.knots + (size_t)b * 4;
              kn[0] = (double)iso_key_unmap(a.ukey[h]); kn[1] = (double)iso_key_unmap(a.ukey[last]); kn[2] = mean; kn[3] = (double)rows;
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// nh[p] = the first unit head at or after p (N: none).  Reads the units as iso_seg_apply<true> left them.
__global__ __launch_bounds__(IS_TH) void iso_next_head(IsoDev a) {
  for (long long q = (long long)blockIdx.x * IS_TH + threadIdx.x; q < a.N; q += (long long)gridDim.x * IS_TH) {
    const int p = (int)q;
    int v = p;
    if (!(a.flags[p] & 1)) {
      const int h = clampi(a.block[p], 0, p);
      v = clampi(h + clampi(a.len[h], 1, a.N - h), p + 1, a.N);
    }
    a.nh[p] = v;
  }
}

// The node [a0, a0 + 2 half): its children's blocks are fitted; pool across the boundary between them until the means are ordered.
__device__ __forceinline__ void iso_merge_node(const IsoDev& a, long long a0, int half) {
  const long long m0 = a0 + half, b0 = a0 + 2ll * half;
  if (m0 >= a.N) return;
  const int lo = clampi(a.nh[a0], 0, a.N), m = clampi(a.nh[m0], 0, a.N), hi = b0 >= a.N ? a.N : clampi(a.nh[b0], 0, a.N);
  if (!(lo < m && m < hi)) return;                                     // a child without a unit of its own
  if (a.flags[m] & 2) return;                                          // two segments
  int start = clampi(a.head[m - 1], lo, m - 1);
  int end = m + clampi(a.len[m], 1, hi - m);
  const double sl = a.lsum[m - 1], sr = a.sum[m];
  if (!(sl * (double)(end - m) >= sr * (double)(m - start))) return;   // mean_left < mean_right
  double s = sl + sr;
  a.len[m] = 0;
  const int bound = hi - lo;
  for (int it = 0; it < bound; ++it) {
    bool changed = false;
    if (start > lo && !(a.flags[start] & 2)) {
      const int e1 = start - 1, h2 = clampi(a.head[e1], lo, e1);
      const double s2 = a.lsum[e1];
      if (s2 * (double)(end - start) >= s * (double)(start - h2)) {
        a.len[start] = 0;
        start = h2; s = s2 + s; changed = true;
      }
    }
    if (end < hi && !(a.flags[end] & 2)) {
      const int c2 = clampi(a.len[end], 1, hi - end);
      const double s2 = a.sum[end];
      if (s * (double)c2 >= s2 * (double)(end - start)) {
        a.len[end] = 0;
        end += c2; s = s + s2; changed = true;
      }
    }
    if (!changed) break;
  }
  a.sum[start] = s; a.len[start] = end - start; a.head[end - 1] = start; a.lsum[end - 1] = s;
}

// Levels 0 .. levels-1 of one tile after another, a block barrier between levels: a node's blocks lie in [nh[a0], nh[b0]), which no
// other node of the level and no other tile touches.  The levels hand their blocks on through GLOBAL memory: this rests on
// __syncthreads() making one wave's global stores visible to the other waves of the block.  It does: the barrier carries a
// workgroup-scope release / acquire fence, and on gfx950 the waves of a block run on one CU and share its L1 (no threadgroup-split
// mode is used).  An LDS stack would not need the assumption; the in-tile fit depends on it.
__global__ __launch_bounds__(IS_TH) void iso_merge_low(IsoDev a, int levels) {
  for (int tile = blockIdx.x; tile < a.NT; tile += gridDim.x) {
    const long long tile0 = (long long)tile * IS_T;
    for (int l = 0; l < levels; ++l) {
      const int half = 1 << l, nodes = IS_T >> (l + 1);
      for (int k = threadIdx.x; k < nodes; k += IS_TH) iso_merge_node(a, tile0 + (long long)k * 2 * half, half);
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(64) void iso_merge_level(IsoDev a, int l) {
  const int half = 1 << l;
  const long long nodes = ((long long)a.N + 2ll * half - 1) / (2ll * half);
  for (long long k = (long long)blockIdx.x * 64 + threadIdx.x; k < nodes; k += (long long)gridDim.x * 64) iso_merge_node(a, k * 2 * half, half);
}

__global__ __launch_bounds__(IS_TH) void iso_fill(IsoDev a) {
  for (long long q = (long long)blockIdx.x * IS_TH + threadIdx.x; q < a.N; q += (long long)gridDim.x * IS_TH)
    a.fit[q] = a.sum[clampi(a.block[q], 0, a.N - 1)];
}

// seg_blocks[s] = the rank of the block that starts at seg_offsets[s] (an empty segment: that of the next one; past the end: all).
__global__ __launch_bounds__(IS_TH) void iso_seg_blocks(IsoDev a) {
  const int total = a.N > 0 ? clampi(a.total[0], 0, a.N) : 0;
  for (int s = blockIdx.x * IS_TH + threadIdx.x; s <= a.S; s += gridDim.x * IS_TH) {
    const int p = clampi(a.seg[s], 0, a.N);
    a.seg_blocks[s] = p >= a.N ? total : clampi(a.nh[p], 0, total);
  }
}

struct ApplyDev {
  const float* x;
  const int32_t *ids, *offs;
  const double* knots;
  float* out;
  long long n;
  int S, P, B;
};

__global__ __launch_bounds__(IS_TH) void calib_apply_kernel(ApplyDev a) {
  for (long long q = (long long)blockIdx.x * IS_TH + threadIdx.x; q < a.n; q += (long long)gridDim.x * IS_TH) {
    const int c = (int)(q % a.S), m = clampi(a.ids[c], 0, a.P - 1);
    const int k0 = clampi(a.offs[m], 0, a.B), k1 = clampi(a.offs[m + 1], k0, a.B);
    const float xf = a.x[q];
    const double x = (double)xf;
    double r = __longlong_as_double(0x7ff8000000000000ll);
    if (k1 > k0 && xf == xf) {
      int lo = k0, hi = k1;                                            // the last block whose lowest key is <= x, or the first block
      for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.knots[(size_t)mid * 4] <= x) lo = mid; else hi = mid;
      }
      const double* kb = a.knots + (size_t)lo * 4;
      const double hi_b = kb[1], v_b = kb[2];
      if (x <= hi_b || lo + 1 >= k1) r = v_b;
      else {
        const double lo_n = kb[4], v_n = kb[6];
        r = v_b + (v_n - v_b) * ((x - hi_b) / (lo_n - hi_b));
      }
    }
    a.out[q] = (float)r;
  }
}

size_t iso_up256(size_t b) { return (b + 255) & ~(size_t)255; }

int iso_grid(long long items, int cap) { return (int)(items < 1 ? 1 : (items < cap ? items : cap)); }

}  // namespace

IsoScratch iso_scratch_layout(long long N) {
  IsoScratch L{};
  const size_t n = (size_t)N, NT = (size_t)((N + IS_T - 1) / IS_T);
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off += iso_up256(bytes); return at; };
  L.NT = (int)NT;
  L.sum = take(n * 8); L.lsum = take(n * 8);
  L.ys = take(n * 4); L.ukey = take(n * 4); L.len = take(n * 4); L.head = take(n * 4); L.nh = take(n * 4);
  L.flags = take(n);
  L.cp = take(NT * 8); L.after = take(NT * 8);
  L.fh = take(NT * 4); L.lh = take(NT * 4); L.fwd = take(NT * 4); L.bwd = take(NT * 4); L.nheads = take(NT * 4); L.hbase = take(NT * 4);
  L.total = take(4);
  L.bytes = off;
  return L;
}

void launch_isotonic(const float* key, const float* y, int M, const int* order, int N, const int* seg_offsets, int S, void* scratch,
                     int* block, double* fit, int* seg_blocks, double* knots, int max_blocks, hipStream_t s) {
  const IsoScratch L = iso_scratch_layout(N);
  char* base = static_cast<char*>(scratch);
  IsoDev d{};
  d.key = key; d.y = y; d.order = order; d.seg = seg_offsets;
  d.M = M; d.N = N; d.S = S; d.NT = L.NT;
  d.ys = reinterpret_cast<float*>(base + L.ys); d.ukey = reinterpret_cast<uint32_t*>(base + L.ukey);
  d.flags = reinterpret_cast<uint8_t*>(base + L.flags);
  d.sum = reinterpret_cast<double*>(base + L.sum); d.lsum = reinterpret_cast<double*>(base + L.lsum);
  d.len = reinterpret_cast<int32_t*>(base + L.len); d.head = reinterpret_cast<int32_t*>(base + L.head);
  d.nh = reinterpret_cast<int32_t*>(base + L.nh);
  d.cp = reinterpret_cast<double*>(base + L.cp); d.after = reinterpret_cast<double*>(base + L.after);
  d.fh = reinterpret_cast<int32_t*>(base + L.fh); d.lh = reinterpret_cast<int32_t*>(base + L.lh);
  d.fwd = reinterpret_cast<int32_t*>(base + L.fwd); d.bwd = reinterpret_cast<int32_t*>(base + L.bwd);
  d.nheads = reinterpret_cast<int32_t*>(base + L.nheads); d.hbase = reinterpret_cast<int32_t*>(base + L.hbase);
  d.total = reinterpret_cast<int32_t*>(base + L.total);
  d.block = block; d.fit = fit; d.seg_blocks = seg_blocks; d.knots = knots;
  const int cap = max_blocks > 0 && max_blocks < ISO_MAX_BLOCKS ? max_blocks : ISO_MAX_BLOCKS;
  const int segs = iso_grid((S + 1 + IS_TH - 1) / IS_TH, cap);
  if (N == 0) {
    iso_seg_blocks<<<segs, IS_TH, 0, s>>>(d);
    return;
  }
  const int rows = iso_grid(((long long)N + IS_TH - 1) / IS_TH, cap), tiles = iso_grid(L.NT, cap);
  int levels = 0;
  while ((1ll << levels) < (long long)N) ++levels;                     // ceil(log2 N): the root is the node [0, 2^levels)
  iso_gather<<<rows, IS_TH, 0, s>>>(d);
  iso_seg_reduce<true><<<tiles, IS_TH, 0, s>>>(d);
  iso_seg_scan<<<1, IS_SCAN, 0, s>>>(d);
  iso_seg_apply<true><<<tiles, IS_TH, 0, s>>>(d);
  iso_next_head<<<rows, IS_TH, 0, s>>>(d);
  iso_merge_low<<<tiles, IS_TH, 0, s>>>(d, levels < IS_LOW ? levels : IS_LOW);
  for (int l = IS_LOW; l < levels; ++l) {
    const long long nodes = ((long long)N + (2ll << l) - 1) / (2ll << l);
    iso_merge_level<<<iso_grid((nodes + 63) / 64, cap), 64, 0, s>>>(d, l);
  }
  iso_seg_reduce<false><<<tiles, IS_TH, 0, s>>>(d);
  iso_seg_scan<<<1, IS_SCAN, 0, s>>>(d);
  iso_seg_apply<false><<<tiles, IS_TH, 0, s>>>(d);
  iso_fill<<<rows, IS_TH, 0, s>>>(d);
  iso_seg_blocks<<<segs, IS_TH, 0, s>>>(d);
}

void launch_calib_apply(const float* x, long long R, int S, const int* map_ids, const int* map_offsets, int P, const double* knots,
                        int B, float* out, int max_blocks, hipStream_t s) {
  const ApplyDev d{x, map_ids, map_offsets, knots, out, R * S, S, P, B};
  const int cap = max_blocks > 0 && max_blocks < ISO_MAX_BLOCKS ? max_blocks : ISO_MAX_BLOCKS;
  calib_apply_kernel<<<iso_grid((d.n + IS_TH - 1) / IS_TH, cap), IS_TH, 0, s>>>(d);
}
