// Scoring of a part-segmentation head against label maps: the reference's losses/segmentation.py:CrossEntropy (bilinear upsample
// with align_corners=True, then nn.CrossEntropyLoss) and the per-class counts of pixel accuracy and IoU, in one pass over the label
// pixels.  The contract is stated in include/poco_hip.h and DESIGN.md section 21; tests/segm_np.py restates it.
//
//   segm_score    a block owns SEGM tile rows of one crop: it stages the (at most four) source rows of every channel in LDS, then per
//                 label pixel interpolates the C logits twice (argmax and maximum, then the sum of exponentials), accumulates the
//                 counts with LDS integer atomics and the cross-entropy in fp64 registers; one global integer add per class and one
//                 fp64 partial per block
//   segm_reduce   per crop: the partials of its blocks added in block order -> word 0 of the record
// The same input gives the same bits on every run: integer adds commute, every floating-point sum has a fixed order.
#include "common.h"
#include "kernels.h"

// one fixed float32 expression order for the interpolation, as tests/segm_np.py evaluates it
#pragma clang fp contract(off)

namespace {

constexpr int SEGM_BLOCK = 256;
constexpr int SEGM_SRC_ROWS = 4;

// source coordinate of destination index i under align_corners=True: scale * i with scale = (n_src - 1) / (n_dst - 1) (0 for n_dst = 1)
struct Tap {
  int i0, i1;
  float l, h;
};
__device__ __forceinline__ Tap segm_tap(int i, float scale, int n_src) {
  const float s = scale * (float)i;
  Tap t;
  t.i0 = min((int)s, n_src - 1);
  t.i1 = min(t.i0 + 1, n_src - 1);
  t.l = s - (float)t.i0;
  t.h = 1.f - t.l;
  return t;
}

__global__ __launch_bounds__(SEGM_BLOCK) void segm_score(const float* __restrict__ logits, const unsigned char* __restrict__ labels, int C,
                                                         int h, int w, int H, int W, int tile_rows, float scale_h, float scale_w,
                                                         unsigned long long* __restrict__ records, double* __restrict__ partials) {
  extern __shared__ float smem[];                       // [SEGM_SRC_ROWS][C][w] source rows
  __shared__ int cnt[1 + 3 * POCO_SEGM_MAX_CLASSES];    // correct, then per class intersection / predicted / ground truth
  __shared__ double wave_sum[SEGM_BLOCK / 64];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int r_lo = tile * tile_rows, r_hi = min(H, r_lo + tile_rows);
  const int y_lo = segm_tap(r_lo, scale_h, h).i0;
  for (int i = tid; i < 1 + 3 * C; i += SEGM_BLOCK) cnt[i] = 0;
  // stage source rows y_lo .. y_lo + 3 (clamped to the last row) of every channel
  const float* src = logits + (size_t)b * C * h * w;
  for (int i = tid; i < SEGM_SRC_ROWS * C * w; i += SEGM_BLOCK) {
    const int x = i % w, c = (i / w) % C, k = i / (w * C);
    smem[i] = src[((size_t)c * h + min(y_lo + k, h - 1)) * w + x];
  }
  __syncthreads();
  double ce = 0.0;
  int correct = 0;
  const int npix = (r_hi - r_lo) * W;
  const size_t rec = (size_t)b * (2 + 3 * C);
  for (int i = tid; i < npix; i += SEGM_BLOCK) {
    const int r = r_lo + i / W, col = i % W;
    const int lab = labels[((size_t)b * H + r) * W + col];
    if (lab >= C) continue;                             // not a class of this head: counted nowhere
    const Tap ty = segm_tap(r, scale_h, h), tx = segm_tap(col, scale_w, w);
    // rows relative to the staged window; the host sizes tile_rows so that both lie in it (the min only guards the LDS bound)
    const int k0 = min(ty.i0 - y_lo, SEGM_SRC_ROWS - 1), k1 = min(ty.i1 - y_lo, SEGM_SRC_ROWS - 1);
    const float* row0 = smem + (size_t)k0 * C * w;
    const float* row1 = smem + (size_t)k1 * C * w;
    float best = 0.f, at_label = 0.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const float* p0 = row0 + c * w;
      const float* p1 = row1 + c * w;
      const float v = ty.h * (tx.h * p0[tx.i0] + tx.l * p0[tx.i1]) + ty.l * (tx.h * p1[tx.i0] + tx.l * p1[tx.i1]);
      if (c == 0 || v > best) { best = v; arg = c; }   // strict: the lowest channel wins a tie
      if (c == lab) at_label = v;
    }
    float se = 0.f;
    for (int c = 0; c < C; ++c) {
      const float* p0 = row0 + c * w;
      const float* p1 = row1 + c * w;
      const float v = ty.h * (tx.h * p0[tx.i0] + tx.l * p0[tx.i1]) + ty.l * (tx.h * p1[tx.i0] + tx.l * p1[tx.i1]);
      se += expf(v - best);
    }
    ce += (double)((best + logf(se)) - at_label);       // -log_softmax[label]
    atomicAdd(&cnt[1 + 3 * arg + 1], 1);
    atomicAdd(&cnt[1 + 3 * lab + 2], 1);
    if (arg == lab) {
      atomicAdd(&cnt[1 + 3 * arg], 1);
      ++correct;
    }
  }
  // cross-entropy of the block: lanes in a fixed butterfly, then the waves in order
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ce += __shfl_down(ce, o, 64);
    correct += __shfl_down(correct, o, 64);
  }
  if ((tid & 63) == 0) {
    wave_sum[tid >> 6] = ce;
    if (correct) atomicAdd(&cnt[0], correct);
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    #pragma unroll
    for (int k = 0; k < SEGM_BLOCK / 64; ++k) s += wave_sum[k];
    partials[(size_t)b * gridDim.x + tile] = s;
  }
  for (int i = tid; i < 1 + 3 * C; i += SEGM_BLOCK)
    if (cnt[i]) atomicAdd(records + rec + 1 + i, (unsigned long long)cnt[i]);
}

__global__ __launch_bounds__(64) void segm_reduce(const double* __restrict__ partials, int B, int tiles, int words,
                                                  unsigned long long* __restrict__ records) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < tiles; ++k) s += partials[(size_t)b * tiles + k];
  records[(size_t)b * words] = (unsigned long long)__double_as_longlong(s);
}

// the demo's picture: the class the scorer would call predicted, per pixel; logits read through the cache (56 x 56 x C floats a crop)
__global__ __launch_bounds__(SEGM_BLOCK) void segm_argmax(const float* __restrict__ logits, int C, int h, int w, int H, int W,
                                                          float scale_h, float scale_w, unsigned char* __restrict__ out) {
  const int i = blockIdx.x * SEGM_BLOCK + threadIdx.x, b = blockIdx.y;
  if (i >= H * W) return;
  const Tap ty = segm_tap(i / W, scale_h, h), tx = segm_tap(i % W, scale_w, w);
  const float* src = logits + (size_t)b * C * h * w;
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float* p0 = src + ((size_t)c * h + ty.i0) * w;
    const float* p1 = src + ((size_t)c * h + ty.i1) * w;
    const float v = ty.h * (tx.h * p0[tx.i0] + tx.l * p0[tx.i1]) + ty.l * (tx.h * p1[tx.i0] + tx.l * p1[tx.i1]);
    if (c == 0 || v > best) { best = v; arg = c; }
  }
  out[(size_t)b * H * W + i] = (unsigned char)arg;
}

}  // namespace

// label rows per block: the largest count (at most 8) whose source rows fit the staged window.  Rows r .. r + n - 1 reach source
// rows floor(s r) .. floor(s (r + n - 1)) + 1; with (n - 1) s <= 1.75 the floors differ by at most 2 (the quarter is the margin for
// the float32 rounding of s r), so four rows hold them.
int segm_tile_rows(int h, int H) {
  if (H <= 1 || h <= 1) return 8;
  const double s = (double)(h - 1) / (double)(H - 1);
  const int n = (int)(1.75 / s) + 1;
  return n < 1 ? 1 : (n > 8 ? 8 : n);
}

size_t segm_score_lds_bytes(int C, int w) { return (size_t)SEGM_SRC_ROWS * C * w * sizeof(float); }

void launch_segm_score(const float* logits, const unsigned char* labels, int B, int C, int h, int w, int H, int W,
                       unsigned long long* records, double* partials, hipStream_t s) {
  const int rows = segm_tile_rows(h, H), tiles = (H + rows - 1) / rows;
  const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
  segm_score<<<dim3(tiles, B), SEGM_BLOCK, segm_score_lds_bytes(C, w), s>>>(logits, labels, C, h, w, H, W, rows, sh, sw, records, partials);
  segm_reduce<<<(B + 63) / 64, 64, 0, s>>>(partials, B, tiles, 2 + 3 * C, records);
}

void launch_segm_argmax(const float* logits, int B, int C, int h, int w, int H, int W, unsigned char* out, hipStream_t s) {
  const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
  segm_argmax<<<dim3((H * W + SEGM_BLOCK - 1) / SEGM_BLOCK, B), SEGM_BLOCK, 0, s>>>(logits, C, h, w, H, W, sh, sw, out);
}
