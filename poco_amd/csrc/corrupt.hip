// Image degradation of raw crops for eval.py --corrupt: per crop a chain of at most four steps - Gaussian blur, motion blur, pixelation,
// contrast, gamma, Gaussian pixel noise, and the byte rounding that precedes a JPEG round trip - one launch per chain position over
// all crops, the record choosing the kind per crop.  The contract is stated in include/poco_hip.h (poco_op_corrupt) and DESIGN.md
// section 35; tests/corrupt_np.py restates it with plain float64 loops.
//
//   grid       (tiles of 32 x 32 pixels, 3 channels, crops); a block of 256 lanes = 32 columns x 8 rows, each lane four rows of its
//              column.  The kind is uniform in a block, so every branch on it is wave-uniform.
//   arithmetic every step reads fp32, evaluates in fp64 (no contraction), clamps to [0, 255] and rounds once to fp32 on the store.
//   border     a tap outside the plane is mirrored without repeating the edge (scipy.ndimage mode='mirror'), as often as needed.
//   blur       the weights exp(-k^2 / (2 sigma^2)), k = -r .. r, r = int(3 sigma + 0.5) <= 15, are normalised by lane 0 in order.  The
//              horizontal pass of the tile's 32 + 2r rows stays fp64 in LDS ([62][32] doubles = 15.5 KB); the vertical pass reads it
//              column-wise: the 32 lanes of a half-wave read 32 consecutive doubles, one 256-byte bank row, free of conflicts.
//   pixelate   column sums over each cell's rows (LDS), then a lane per cell adds its columns left to right and divides by the
//              cell's pixel count; a cell cut by a tile border is summed by both tiles in the same order, hence to the same bits.
//   contrast   the block of tile 0 serves its whole plane (the other tiles of a contrast crop return at once): lane-strided fp64
//              sums in row-major order, block_tree_sum, one division; then mean + c (x - mean).
//   noise      Philox4x32-10, key = the record's seed, counter = (e / 4, 0, stream, chain position) for element e of the crop's
//              [3, res, res] block: two Box-Muller pairs in fp64 for elements 4q .. 4q + 3.
//
// No floating-point atomics, no allocation, no synchronisation.  LDS: 16 KB + 2.8 KB.  A record is device data: the kernel clamps the
// kind, every integer parameter and every coordinate it derives from a record, so a bad record gives wrong pixels, never a wild access.
#include "../../include/poco_hip.h"
#include "block_prims.h"
#include "common.h"
#include "philox.h"

#include <cmath>
#include <cstdint>
#include <string>

#pragma clang fp contract(off)

namespace {

constexpr int CR_TILE = 32;                 // pixels per tile side
constexpr int CR_TH = 256;                  // lanes: 32 columns x 8 rows
constexpr int CR_RMAX = 15;                 // blur radius bound = int(3 * 5 + 0.5)
constexpr int CR_BUF = 2048;                // doubles: blur (32 + 2 * 15) * 32 = 1984; pixelate column sums <= 18 * 96 = 1728; tree 256
constexpr int CR_CELLS = 18;                // cells of one tile along an axis: f = 2 gives 16; an unaligned start would add two
static_assert((CR_TILE + 2 * CR_RMAX) * CR_TILE <= CR_BUF && CR_CELLS * (CR_TILE + 2 * 32) <= CR_BUF && CR_TH <= CR_BUF, "LDS plan");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// scipy.ndimage mode='mirror': ... 2 1 | 0 1 2 .. n-1 | n-2 n-3 ...; any i, n >= 1
__device__ __forceinline__ int mirror(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  int m = i % period;
  if (m < 0) m += period;
  return m < n ? m : period - m;
}

__device__ __forceinline__ double clamp_pix(double v) { return fmin(fmax(v, 0.0), 255.0); }   // NaN becomes 0

__device__ __forceinline__ void store_pix(float* __restrict__ dst, size_t i, int c, double v, int normalize) {
  float f = (float)clamp_pix(v);
  if (normalize) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    f = (f / 255.0f - mean[c]) / stdv[c];                                                    // oracle/crop_np.normalize_np, float32
  }
  dst[i] = f;
}

// steps [N][L]; pos < L: the records' position; pos >= L: every crop is copied (and normalised).
__global__ __launch_bounds__(CR_TH) void corrupt_step_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             const poco_corrupt_step_t* __restrict__ steps, int L, int pos, int res,
                                                             int tiles_x, int normalize) {
  __shared__ double buf[CR_BUF];
  __shared__ double cellmean[CR_CELLS * CR_CELLS];
  __shared__ double wts[2 * CR_RMAX + 1];
  const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int x0 = (tile % tiles_x) * CR_TILE, y0 = (tile / tiles_x) * CR_TILE;
  const size_t plane = (size_t)res * res, base = ((size_t)n * 3 + c) * plane;
  const float* __restrict__ src = in + base;
  float* __restrict__ dst = out + base;
  poco_corrupt_step_t st{};
  if (pos < L) st = steps[(size_t)n * L + pos];
  const int kind = (st.kind < 0 || st.kind > POCO_CORRUPT_JPEG) ? POCO_CORRUPT_NONE : st.kind;
  const int x = x0 + tx;

  if (kind == POCO_CORRUPT_CONTRAST) {
    if (tile != 0) return;
    double acc = 0.0;
    for (size_t i = t; i < plane; i += CR_TH) acc = acc + (double)src[i];
    const double mean = block_tree_sum<CR_TH>(acc, buf) / (double)plane;
    const double cc = (double)st.p0;
    for (size_t i = t; i < plane; i += CR_TH) store_pix(dst, i, c, mean + cc * ((double)src[i] - mean), normalize);
    return;
  }

  if (kind == POCO_CORRUPT_GAUSSIAN_BLUR) {
    const double sigma = fmin(fmax((double)st.p0, 1e-3), 5.0);
    const int r = clampi((int)(3.0 * sigma + 0.5), 0, CR_RMAX);
    if (t <= 2 * r) { const double k = (double)(t - r); wts[t] = exp(-(k * k) / (2.0 * sigma * sigma)); }
    __syncthreads();
    if (t == 0) {
      double s = 0.0;
      for (int k = 0; k <= 2 * r; ++k) s = s + wts[k];
      for (int k = 0; k <= 2 * r; ++k) wts[k] = wts[k] / s;
    }
    __syncthreads();
    const int rows = CR_TILE + 2 * r;
    for (int j = ty; j < rows; j += CR_TH / 32) {                      // the horizontal pass, fp64 into LDS
      double h = 0.0;
      if (x < res) {
        const float* __restrict__ row = src + (size_t)mirror(y0 - r + j, res) * res;
        for (int k = -r; k <= r; ++k) h = h + wts[k + r] * (double)row[mirror(x + k, res)];
      }
      buf[j * CR_TILE + tx] = h;
    }
    __syncthreads();
    for (int j = ty; j < CR_TILE; j += CR_TH / 32) {                   // the vertical pass
      const int y = y0 + j;
      if (x < res && y < res) {
        double v = 0.0;
        for (int k = -r; k <= r; ++k) v = v + wts[k + r] * buf[(j + r + k) * CR_TILE + tx];
        store_pix(dst, (size_t)y * res + x, c, v, normalize);
      }
    }
    return;
  }

  if (kind == POCO_CORRUPT_PIXELATE) {
    const int f = clampi(st.ival, 2, 32);
    const int x1 = min(x0 + CR_TILE, res), y1 = min(y0 + CR_TILE, res);                  // the tile's pixels [x0, x1) x [y0, y1)
    const int cx0 = x0 / f, cy0 = y0 / f;
    const int ncx = min((x1 - 1) / f - cx0 + 1, CR_CELLS), ncy = min((y1 - 1) / f - cy0 + 1, CR_CELLS);
    const int sx0 = cx0 * f, span = min(min((cx0 + ncx) * f, res) - sx0, CR_TILE + 2 * 32);   // the columns of those cells
    for (int it = t; it < ncy * span; it += CR_TH) {                                     // column sums over each cell row
      const int cy = it / span, xx = sx0 + it % span;
      const int ya = (cy0 + cy) * f, yb = min(ya + f, res);
      double s = 0.0;
      for (int yy = ya; yy < yb; ++yy) s = s + (double)src[(size_t)yy * res + xx];
      buf[it] = s;
    }
    __syncthreads();
    for (int it = t; it < ncy * ncx; it += CR_TH) {
      const int cy = it / ncx, cx = it % ncx;
      const int xa = (cx0 + cx) * f, xb = min(xa + f, res), ya = (cy0 + cy) * f, yb = min(ya + f, res);
      double s = 0.0;
      for (int xx = xa; xx < xb; ++xx) s = s + buf[cy * span + min(xx - sx0, span - 1)];
      cellmean[cy * CR_CELLS + cx] = s / (double)((xb - xa) * (yb - ya));
    }
    __syncthreads();
    for (int j = ty; j < CR_TILE; j += CR_TH / 32) {
      const int y = y0 + j;
      if (x < res && y < res)
        store_pix(dst, (size_t)y * res + x, c, cellmean[clampi(y / f - cy0, 0, CR_CELLS - 1) * CR_CELLS + clampi(x / f - cx0, 0, CR_CELLS - 1)],
                  normalize);
    }
    return;
  }

  // the pointwise kinds and the motion blur: a pixel per lane and row
  for (int j = ty; j < CR_TILE; j += CR_TH / 32) {
    const int y = y0 + j;
    if (x >= res || y >= res) continue;
    const size_t i = (size_t)y * res + x;
    double v = (double)src[i];
    if (kind == POCO_CORRUPT_MOTION_BLUR) {
      const int Lm = clampi(st.ival, 3, 31) | 1, half = (Lm - 1) / 2;
      const double dx = (double)st.p0, dy = (double)st.p1;
      double s = 0.0;
      for (int k = -half; k <= half; ++k) {
        const double sx = fmin(fmax((double)x + (double)k * dx, -1.0e6), 1.0e6), sy = fmin(fmax((double)y + (double)k * dy, -1.0e6), 1.0e6);
        const double fx0 = floor(sx), fy0 = floor(sy), fx = sx - fx0, fy = sy - fy0;
        const int xa = mirror((int)fx0, res), xb = mirror((int)fx0 + 1, res), ya = mirror((int)fy0, res), yb = mirror((int)fy0 + 1, res);
        const double v00 = (double)src[(size_t)ya * res + xa], v01 = (double)src[(size_t)ya * res + xb];
        const double v10 = (double)src[(size_t)yb * res + xa], v11 = (double)src[(size_t)yb * res + xb];
        const double top = (1.0 - fx) * v00 + fx * v01, bot = (1.0 - fx) * v10 + fx * v11;
        s = s + ((1.0 - fy) * top + fy * bot);
      }
      v = s / (double)Lm;
    } else if (kind == POCO_CORRUPT_GAMMA) {
      v = 255.0 * pow(v / 255.0, (double)st.p0);
    } else if (kind == POCO_CORRUPT_GAUSSIAN_NOISE) {
      const size_t e = (size_t)c * plane + i;
      const Philox4 w = philox4x32_10((uint32_t)(e >> 2), 0u, st.stream, (uint32_t)pos, st.seed[0], st.seed[1]);
      const int q = (int)(e & 3), pr = q >> 1;
      const double u1 = ((double)w.w[2 * pr] + 1.0) * 0x1p-32, u2 = (double)w.w[2 * pr + 1] * 0x1p-32;
      const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586 * u2;
      const double z = (q & 1) ? rad * sin(ang) : rad * cos(ang);
      v = v + (double)st.p0 * z;
    } else if (kind == POCO_CORRUPT_JPEG) {
      v = floor(v + 0.5);
    }
    store_pix(dst, i, c, v, normalize);
  }
}

int corrupt_bad(const std::string& m) {
  poco_set_error("poco_op_corrupt: " + m);
  return POCO_ERR_ARG;
}

// a record's parameters against the ranges of the header; empty = fine
std::string step_error(const poco_corrupt_step_t& s) {
  auto fin = [](float v) { return std::isfinite(v); };
  switch (s.kind) {
    case POCO_CORRUPT_NONE: return "";
    case POCO_CORRUPT_GAUSSIAN_BLUR: return fin(s.p0) && s.p0 > 0.f && s.p0 <= 5.f ? "" : "gaussian_blur needs sigma in (0, 5]";
    case POCO_CORRUPT_MOTION_BLUR:
      if (s.ival < 3 || s.ival > 31 || !(s.ival & 1)) return "motion_blur needs an odd length in 3..31";
      if (!fin(s.p0) || !fin(s.p1) || std::fabs((double)s.p0 * s.p0 + (double)s.p1 * s.p1 - 1.0) > 1e-5) return "motion_blur needs a unit direction";
      return "";
    case POCO_CORRUPT_PIXELATE: return s.ival >= 2 && s.ival <= 32 ? "" : "pixelate needs a factor in 2..32";
    case POCO_CORRUPT_CONTRAST: return fin(s.p0) && s.p0 >= 0.f && s.p0 <= 2.f ? "" : "contrast needs c in [0, 2]";
    case POCO_CORRUPT_GAMMA: return fin(s.p0) && s.p0 >= 0.2f && s.p0 <= 5.f ? "" : "gamma needs g in [0.2, 5]";
    case POCO_CORRUPT_GAUSSIAN_NOISE: return fin(s.p0) && s.p0 >= 0.f && s.p0 <= 255.f ? "" : "gaussian_noise needs sigma in [0, 255]";
    case POCO_CORRUPT_JPEG: return s.ival >= 1 && s.ival <= 100 ? "" : "jpeg needs a quality in 1..100";
    default: return "unknown kind " + std::to_string(s.kind);
  }
}

}  // namespace

extern "C" int poco_op_corrupt(const float* d_in, const poco_corrupt_step_t* d_steps, const poco_corrupt_step_t* h_steps, int N, int chain_len,
                               int pos_begin, int pos_end, int res, int normalize, float* d_tmp, float* d_out, void* stream) {
  if (!d_in || !d_steps || !h_steps || !d_tmp || !d_out) return corrupt_bad("null pointer");
  if (N < 1) return corrupt_bad("N must be at least 1");
  if (res < 1 || res > 4096) return corrupt_bad("res must be in 1..4096");
  if (chain_len < 1 || chain_len > POCO_CORRUPT_MAX_STEPS)
    return corrupt_bad("a chain of " + std::to_string(chain_len) + " steps: chain_len must be in 1.." + std::to_string(POCO_CORRUPT_MAX_STEPS));
  if (pos_begin < 0 || pos_end < pos_begin || pos_end > chain_len) return corrupt_bad("need 0 <= pos_begin <= pos_end <= chain_len");
  if (d_tmp == d_out || d_in == d_out || d_in == d_tmp) return corrupt_bad("d_in, d_tmp and d_out must be three buffers");
  int last = pos_begin;                                      // one past the last position in the range at which a crop has a step
  for (int n = 0; n < N; ++n) {
    bool ended = false;
    for (int p = 0; p < chain_len; ++p) {
      const poco_corrupt_step_t& s = h_steps[(size_t)n * chain_len + p];
      const std::string e = step_error(s);
      if (!e.empty()) return corrupt_bad("step " + std::to_string(p) + " of crop " + std::to_string(n) + ": " + e);
      if (s.kind == POCO_CORRUPT_NONE) ended = true;
      else if (ended) return corrupt_bad("step " + std::to_string(p) + " of crop " + std::to_string(n) + " follows an empty step");
      else if (p >= pos_begin && p < pos_end && p + 1 > last) last = p + 1;
    }
  }
  // positions pos_begin .. last - 1; none: one launch that copies (and normalises).  The last launch writes d_out.
  const int launches = last > pos_begin ? last - pos_begin : 1;
  const int tiles_x = (res + CR_TILE - 1) / CR_TILE;
  const float* src = d_in;
  for (int l = 0; l < launches; ++l) {
    float* dst = ((launches - 1 - l) & 1) ? d_tmp : d_out;
    const int pos = last > pos_begin ? pos_begin + l : chain_len;
    const int norm = (l == launches - 1 && normalize) ? 1 : 0;
    for (int n0 = 0; n0 < N; n0 += 65535) {                  // gridDim.z limit
      const int nn = N - n0 < 65535 ? N - n0 : 65535;
      const size_t off = (size_t)n0 * 3 * res * res;
      hipLaunchKernelGGL(corrupt_step_kernel, dim3(tiles_x * tiles_x, 3, nn), dim3(CR_TH), 0, (hipStream_t)stream, src + off, dst + off,
                         d_steps + (size_t)n0 * chain_len, chain_len, pos, res, tiles_x, norm);
    }
    src = dst;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { poco_set_error(std::string("poco_op_corrupt: ") + hipGetErrorString(e)); return POCO_ERR_HIP; }
  return POCO_OK;
}
