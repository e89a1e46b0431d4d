// The reference's DATASET crop on the device (eval.py --crop dataset, poco_amd/datacrop.py): BaseDataset.rgb_processing
// (pocolib/dataset/base_dataset.py:201-221) = crop_cv2 (pocolib/utils/image_utils.py:189-206) on the float32 image -> np.fliplr ->
// per-channel pixel noise with clamp -> / 255 -> Normalize, for a whole batch cut from images of mixed sizes, in ONE launch.
// Contract and exactness argument: include/poco_hip.h poco_dataset_crop and DESIGN.md section 22; tests/datacrop_np.py restates it.
//
//   host   gen_trans_from_patch_cv up to the three float32 source points (float32 rotate_2d with numpy's sin / cos): the records
//   device getAffineTransform (LU in double) and warpAffine's inversion (crop_affine.h, shared with the demo crop), the 10-bit
//          fixed-point coordinates with 1/32-pixel fractions, then cv2's FLOAT bilinear blend: weights (32-fx)(32-fy)/1024 ... of
//          byte-valued taps.  Every product and the four-term sum are multiples of 1/1024 below 256, exact in float32 in any order,
//          so the blend is done in integers: raw = (sum_i v_i m_i) / 1024 with sum_i m_i = 1024, taps outside the image = 0.
//
// Launch shape: 256 threads = one 16 x 16 tile of output pixels at a time (a rotated tile still maps to a compact source patch of
// about 16s x 16s pixels for a box/res ratio s; a 256 x 1 row would smear a rotated read over 256 source rows), all three channels
// per thread (the RGB bytes of a tap are adjacent).  A block walks a fixed 2 x 2 group of tiles so that the affine solve - the same
// ~400 dependent fp64 operations for every pixel of a crop - is paid once per wave and 1024 pixels instead of once per 256.  Every
// wave solves for itself with uniform operands: no LDS, no barrier, no atomics, no data-dependent loop.
//
// poco_dataset_crop_occ is the same launch with the reference's synthetic occluders
// (pocolib/dataset/occlusion.py:109-149,247-288) pasted between the flip and the noise: a thread walks its crop's objects in drawn
// order, tests the paste rectangle and computes the ONE texel of cv2.resize(cut-out, INTER_AREA) it needs straight from the atlas -
// the decimation tables are derived on the fly in double, the accumulation is cv2's float32 sequence with no contraction - then blends
// as paste_over does.  No scratch image of resized occluders exists: each resized texel is used by exactly one pixel.  The two entries
// share one kernel body; the plain one instantiates it without the occluder code and keeps its arguments and arithmetic.
// poco_dataset_crop_occ_mask is a third instantiation: it also stores, per pixel, whether a pasted texel with
// alpha > 0 touched it - the condition `cover` counts - as one byte of a [N, res, res] mask.
#include "../../include/poco_hip.h"
#include "common.h"
#include "crop_affine.h"
#include <cmath>
#include <cstdint>

namespace {
constexpr int DC_TILE = 16, DC_GROUP = 2;          // tile side; tiles per block side
constexpr int DC_SPAN = DC_TILE * DC_GROUP;        // output pixels per block side

struct OccArgs {
  const unsigned int* atlas;                 // packed RGBA texels (R in the low byte)
  long long texels;                          // texels in the atlas: every tap is checked against it
  const poco_occluder_t* table;
  int n_occ;
  const poco_occ_record_t* recs;
  int* cover;                                // [N, groups^2] or null
  unsigned char* mask;                       // [N, res, res]: written by the DC_OCC_MASK instantiation only
};

// One axis of cv::computeResizeAreaTab (opencv/modules/imgproc/src/resize.cpp) for destination index d: the entries are the
// consecutive source indices first .. first + n - 1 with weights lead (if has_lead), mid ..., trail (if has_trail).
struct AxisTab {
  int first, n;
  bool has_lead, has_trail;
  float lead, mid, trail;
  __device__ __forceinline__ float weight(int k) const {
    return (has_lead && k == 0) ? lead : ((has_trail && k == n - 1) ? trail : mid);
  }
};

__device__ __forceinline__ AxisTab area_tab(int d, int ssize, int dsize) {
#pragma clang fp contract(off)
  const double scale = (double)ssize / (double)dsize;
  const double f1 = d * scale;
  const double f2 = f1 + scale;
  const double cell = fmin(scale, ssize - f1);
  int s1 = (int)ceil(f1), s2 = (int)floor(f2);
  s2 = min(s2, ssize - 1);
  s1 = min(s1, s2);
  AxisTab t;
  t.has_lead = s1 - f1 > 1e-3;
  t.has_trail = f2 - s2 > 1e-3;
  t.lead = (float)((s1 - f1) / cell);
  t.mid = (float)(1.0 / cell);
  t.trail = (float)(fmin(fmin(f2 - s2, 1.), cell) / cell);
  t.first = s1 - (t.has_lead ? 1 : 0);
  t.n = (t.has_lead ? 1 : 0) + (s2 - s1) + (t.has_trail ? 1 : 0);
  return t;
}

__device__ __forceinline__ bool is_integer_scale(int ssize, int dsize) {
  const double scale = (double)ssize / (double)dsize;
  return fabs(scale - rint(scale)) < 2.220446049250313e-16;
}

// a texel of the cut-out, memory-safe for any table: row and column clamped into the cut-out, the index checked against the atlas
__device__ __forceinline__ unsigned int occ_tap(const OccArgs& oa, long long off, int h, int w, int sy, int sx) {
  sy = min(max(sy, 0), h - 1);
  sx = min(max(sx, 0), w - 1);
  const long long i = off + (long long)sy * w + sx;
  return (i >= 0 && i < oa.texels) ? oa.atlas[i] : 0u;
}

__device__ __forceinline__ unsigned int byte_of(float v) { return (unsigned int)fminf(255.0f, fmaxf(0.0f, rintf(v))); }   // saturate_cast<uchar>

// texel (u, v) of cv2.resize(cut-out [h, w, 4] uint8, (dw, dh), interpolation=INTER_AREA), packed like the atlas
// Every multiply and add below is an operation of its own, as in cv2's scalar loops: `#pragma clang fp contract(off)` on the plain
// operators does that.  The __fmul_rn / __fadd_rn intrinsics do NOT: the headers define them as inline x * y and x + y compiled under
// the default contraction, and after inlining the backend fuses them again.
__device__ unsigned int resized_texel(const OccArgs& oa, long long off, int h, int w, int dw, int dh, int u, int v) {
#pragma clang fp contract(off)
  if (is_integer_scale(w, dw) && is_integer_scale(h, dh)) {
    // resizeAreaFast_: integer sums over sx x sy blocks (1 x 1 is the copy of dsize == ssize)
    const int bx = w / dw, by = h / dh;
    long long s[4] = {0, 0, 0, 0};
    for (int j = 0; j < by; ++j)
      for (int i = 0; i < bx; ++i) {
        const unsigned int t = occ_tap(oa, off, h, w, v * by + j, u * bx + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += (t >> (8 * c)) & 255u;
      }
    unsigned int r = 0;
    const float inv = 1.f / (float)(bx * by);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const unsigned int b = (bx == 2 && by == 2) ? (unsigned int)((s[c] + 2) >> 2) : byte_of((float)s[c] * inv);
      r |= b << (8 * c);
    }
    return r;
  }
  const AxisTab tx = area_tab(u, w, dw), ty = area_tab(v, h, dh);
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < ty.n; ++j) {
    float buf[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < tx.n; ++i) {
      const unsigned int t = occ_tap(oa, off, h, w, ty.first + j, tx.first + i);
      const float a = tx.weight(i);
#pragma unroll
      for (int c = 0; c < 4; ++c) buf[c] = buf[c] + (float)((t >> (8 * c)) & 255u) * a;
    }
    const float b = ty.weight(j);
#pragma unroll
    for (int c = 0; c < 4; ++c) sum[c] = j == 0 ? b * buf[c] : sum[c] + b * buf[c];
  }
  return byte_of(sum[0]) | (byte_of(sum[1]) << 8) | (byte_of(sum[2]) << 16) | (byte_of(sum[3]) << 24);
}

// which of the three kernels the body is instantiated for: the plain crop, the crop with occluders, and that with the mask output
constexpr int DC_PLAIN = 0, DC_OCC = 1, DC_OCC_MASK = 2;

template <int MODE>
__device__ __forceinline__ void dataset_crop_body(const unsigned char* const* __restrict__ images, const int* __restrict__ img_hw, int n_images,
                                                  const poco_dataset_crop_param_t* __restrict__ params, float* __restrict__ out, int res,
                                                  int groups_x, int normalize, const OccArgs& oa) {
#pragma clang fp contract(off)
  constexpr bool OCC = MODE != DC_PLAIN;
  const int n = blockIdx.y;
  const poco_dataset_crop_param_t p = params[n];
  // (device data cannot be validated on the host: an index outside the table is clamped into it, as poco_crop_normalize_multi does)
  const int im = min(max(p.img, 0), n_images - 1);
  const unsigned char* __restrict__ frame = images[im];
  const int H = max(img_hw[2 * im], 0), W = max(img_hw[2 * im + 1], 0);      // a size below 1 is an empty image: every tap is outside
  double Mi[6];
  {
    const float sx[3] = {p.src[0], p.src[2], p.src[4]}, sy[3] = {p.src[1], p.src[3], p.src[5]};
    const float half = (float)(res * 0.5);
    const float dx[3] = {half, half, half + half}, dy[3] = {half, half + half, half};
    crop_affine::inverse_affine_from_points(sx, sy, dx, dy, Mi);
  }
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const float pn[3] = {p.pn[0], p.pn[1], p.pn[2]};
  const bool flip = p.flip != 0;
  const int gx = blockIdx.x % groups_x, gy = blockIdx.x / groups_x;
  const int tx = threadIdx.x & (DC_TILE - 1), ty = threadIdx.x / DC_TILE;
  const size_t cs = (size_t)res * res;
  int n_obj = 0, touched = 0;
  if (OCC) n_obj = min(max(oa.recs[n].count, 0), POCO_OCC_MAX_OBJECTS);
#pragma unroll
  for (int t = 0; t < DC_GROUP * DC_GROUP; ++t) {
    const int x = gx * DC_SPAN + (t % DC_GROUP) * DC_TILE + tx, y = gy * DC_SPAN + (t / DC_GROUP) * DC_TILE + ty;
    if (x >= res || y >= res) continue;
    const int xc = flip ? res - 1 - x : x;            // np.fliplr after the warp: output column x shows crop column res - 1 - x
    const int adelta = crop_affine::cv_round(Mi[0] * xc * 1024.0), bdelta = crop_affine::cv_round(Mi[3] * xc * 1024.0);
    const int X0 = crop_affine::cv_round((Mi[1] * y + Mi[2]) * 1024.0) + 16, Y0 = crop_affine::cv_round((Mi[4] * y + Mi[5]) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const int sx = max(-32768, min(32767, X >> 5)), sy = max(-32768, min(32767, Y >> 5));
    const int fx = X & 31, fy = Y & 31;
    const int m00 = (32 - fy) * (32 - fx), m01 = (32 - fy) * fx, m10 = fy * (32 - fx), m11 = fy * fx;     // sum = 1024
    int acc[3];
    if (sx >= 0 && sy >= 0 && sx <= W - 3 && sy + 1 < H) {
      // interior: the 2 x 2 x RGB neighbourhood is bytes 0..5 of two unaligned 8-byte windows (they end inside the image: sx <= W - 3)
      typedef unsigned long long __attribute__((aligned(1))) u64u;
      const unsigned char* p00 = frame + ((size_t)sy * W + sx) * 3;
      const unsigned long long r0 = *reinterpret_cast<const u64u*>(p00);
      const unsigned long long r1 = *reinterpret_cast<const u64u*>(p00 + (size_t)W * 3);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v00 = (int)((r0 >> (8 * c)) & 255), v01 = (int)((r0 >> (8 * (3 + c))) & 255);
        const int v10 = (int)((r1 >> (8 * c)) & 255), v11 = (int)((r1 >> (8 * (3 + c))) & 255);
        acc[c] = m00 * v00 + m01 * v01 + m10 * v10 + m11 * v11;
      }
    } else {
      const bool x0ok = (unsigned)sx < (unsigned)W, x1ok = (unsigned)(sx + 1) < (unsigned)W;
      const bool y0ok = (unsigned)sy < (unsigned)H, y1ok = (unsigned)(sy + 1) < (unsigned)H;
      const unsigned char* p00 = frame + ((long long)sy * W + sx) * 3;      // only dereferenced where the *ok flags allow
      const unsigned char* p10 = p00 + (long long)W * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v00 = (x0ok && y0ok) ? p00[c] : 0, v01 = (x1ok && y0ok) ? p00[3 + c] : 0;
        const int v10 = (x0ok && y1ok) ? p10[c] : 0, v11 = (x1ok && y1ok) ? p10[3 + c] : 0;
        acc[c] = m00 * v00 + m01 * v01 + m10 * v10 + m11 * v11;
      }
    }
    // acc <= 255 * 1024 < 2^24: exact in float32, and so is the division by 1024
    float raw[3] = {(float)acc[0] * (1.0f / 1024.0f), (float)acc[1] * (1.0f / 1024.0f), (float)acc[2] * (1.0f / 1024.0f)};
    if (OCC) {
      // paste_over (occlusion.py:247-279) for the objects in drawn order: the paste rectangle starts at centre - size // 2; its clip to
      // the crop is the range of (x, y) itself.  The objects are pasted after the flip, so (x, y) is the output pixel.
      bool hit = false;
      for (int k = 0; k < n_obj; ++k) {
        const poco_occ_object_t ob = oa.recs[n].obj[k];
        const int id = min(max(ob.id, 0), oa.n_occ - 1);
        const poco_occluder_t oc = oa.table[id];
        const int h = min(max(oc.h, 1), 4096), w = min(max(oc.w, 1), 4096);
        const int dw = min(max(ob.dst_w, 1), 4096), dh = min(max(ob.dst_h, 1), 4096);
        const long long u = (long long)x - ((long long)ob.cx - dw / 2), v = (long long)y - ((long long)ob.cy - dh / 2);
        if (u < 0 || u >= dw || v < 0 || v >= dh) continue;
        const unsigned int texel = resized_texel(oa, oc.offset, h, w, dw, dh, (int)u, (int)v);
        const unsigned int a8 = texel >> 24;
        hit = hit || a8 != 0;
        const float alpha = (float)a8 / 255.0f;
        const float rest = 1.0f - alpha;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          raw[c] = alpha * (float)((texel >> (8 * c)) & 255u) + rest * raw[c];
      }
      touched += hit ? 1 : 0;
      if (MODE == DC_OCC_MASK) oa.mask[((size_t)n * res + y) * res + x] = hit ? 1 : 0;
    }
    float* o = out + (((size_t)n * 3) * res + y) * res + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = raw[c];
      v = fminf(255.0f, fmaxf(0.0f, v * pn[c]));          // base_dataset.py:216-218 on a float32 array (pn rounded to float32)
      if (normalize) v = (v / 255.0f - mean[c]) / stdv[c];  // base_dataset.py:220 and normalize_img, float32
      o[c * cs] = v;
    }
  }
  if (OCC) {
    if (oa.cover) {                                   // uniform: every block writes its own cell, so the buffer needs no memset
      __shared__ int wave_sum[4];
      int s = touched;
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
      if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) oa.cover[(size_t)n * gridDim.x + blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    }
  }
}

__global__ void __launch_bounds__(256)
dataset_crop_kernel(const unsigned char* const* __restrict__ images, const int* __restrict__ img_hw, int n_images,
                    const poco_dataset_crop_param_t* __restrict__ params, float* __restrict__ out, int res, int groups_x, int normalize) {
  dataset_crop_body<DC_PLAIN>(images, img_hw, n_images, params, out, res, groups_x, normalize, OccArgs{});
}

__global__ void __launch_bounds__(256)
dataset_crop_occ_kernel(const unsigned char* const* __restrict__ images, const int* __restrict__ img_hw, int n_images,
                        const poco_dataset_crop_param_t* __restrict__ params, float* __restrict__ out, int res, int groups_x, int normalize,
                        OccArgs oa) {
  dataset_crop_body<DC_OCC>(images, img_hw, n_images, params, out, res, groups_x, normalize, oa);
}

__global__ void __launch_bounds__(256)
dataset_crop_occ_mask_kernel(const unsigned char* const* __restrict__ images, const int* __restrict__ img_hw, int n_images,
                             const poco_dataset_crop_param_t* __restrict__ params, float* __restrict__ out, int res, int groups_x,
                             int normalize, OccArgs oa) {
  dataset_crop_body<DC_OCC_MASK>(images, img_hw, n_images, params, out, res, groups_x, normalize, oa);
}

// the checks the entries share; `who` names the entry in the message
int check_crop_args(const char* who, const void* d_images, const void* d_img_hw, int n_images, const void* d_params,
                    const poco_dataset_crop_param_t* h_params, int N, int res, const void* d_out) {
  const std::string w(who);
  if (!d_images || !d_img_hw || !d_params || !h_params || !d_out) { poco_set_error(w + ": null pointer"); return POCO_ERR_ARG; }
  if (N < 1 || n_images < 1) { poco_set_error(w + ": N and n_images must be at least 1"); return POCO_ERR_ARG; }
  if (res < 1 || res > 4096) { poco_set_error(w + ": res must be in 1..4096"); return POCO_ERR_ARG; }
  for (int n = 0; n < N; ++n) {
    const poco_dataset_crop_param_t& p = h_params[n];
    bool finite = true;
    for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(p.src[k]);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(p.pn[k]);
    if (!finite) { poco_set_error(w + ": crop " + std::to_string(n) + " has a non-finite parameter"); return POCO_ERR_ARG; }
    if (p.bb < 1) {
      poco_set_error(w + ": the box side of crop " + std::to_string(n) + " rounds to " + std::to_string(p.bb) + " pixels");
      return POCO_ERR_ARG;
    }
  }
  return POCO_OK;
}
}  // namespace

extern "C" int poco_dataset_crop(const unsigned char* const* d_images, const int* d_img_hw, int n_images,
                                 const poco_dataset_crop_param_t* d_params, const poco_dataset_crop_param_t* h_params, int N, int res,
                                 int normalize, float* d_out, void* stream) {
  if (int rc = check_crop_args("poco_dataset_crop", d_images, d_img_hw, n_images, d_params, h_params, N, res, d_out)) return rc;
  const int groups = (res + DC_SPAN - 1) / DC_SPAN;
  for (int n0 = 0; n0 < N; n0 += 65535) {             // gridDim.y limit
    const int nn = N - n0 < 65535 ? N - n0 : 65535;
    hipLaunchKernelGGL(dataset_crop_kernel, dim3(groups * groups, nn), dim3(256), 0, (hipStream_t)stream, d_images, d_img_hw, n_images,
                       d_params + n0, d_out + (size_t)n0 * 3 * res * res, res, groups, normalize ? 1 : 0);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { poco_set_error(std::string("poco_dataset_crop: ") + hipGetErrorString(e)); return POCO_ERR_HIP; }
  return POCO_OK;
}

// poco_dataset_crop_occ (want_mask = false: d_mask is not looked at) and poco_dataset_crop_occ_mask behind one set of checks
static int crop_occ_entry(const std::string& who, bool want_mask, const unsigned char* const* d_images, const int* d_img_hw, int n_images,
                          const poco_dataset_crop_param_t* d_params, const poco_dataset_crop_param_t* h_params, int N, int res,
                          int normalize, const unsigned char* d_atlas, long long atlas_texels, const poco_occluder_t* d_occluders,
                          const poco_occluder_t* h_occluders, int n_occluders, const poco_occ_record_t* d_occ,
                          const poco_occ_record_t* h_occ, float* d_out, int* d_cover, unsigned char* d_mask, void* stream) {
  if (want_mask && !d_mask) { poco_set_error(who + ": null pointer"); return POCO_ERR_ARG; }
  if (!d_atlas || !d_occluders || !h_occluders || !d_occ || !h_occ) { poco_set_error(who + ": null pointer"); return POCO_ERR_ARG; }
  if (reinterpret_cast<uintptr_t>(d_atlas) & 3) { poco_set_error(who + ": the atlas must be 4-byte aligned"); return POCO_ERR_ARG; }
  if (int rc = check_crop_args(who.c_str(), d_images, d_img_hw, n_images, d_params, h_params, N, res, d_out)) return rc;
  if (res > 256) { poco_set_error(who + ": res must be at most 256 (a larger crop would upscale cut-outs: INTER_LINEAR is not built)"); return POCO_ERR_ARG; }
  if (n_occluders < 1 || atlas_texels < 1) { poco_set_error(who + ": the atlas is empty"); return POCO_ERR_ARG; }
  for (int k = 0; k < n_occluders; ++k) {
    const poco_occluder_t& oc = h_occluders[k];
    if (oc.h < 1 || oc.h > 4096 || oc.w < 1 || oc.w > 4096) {
      poco_set_error(who + ": cut-out " + std::to_string(k) + " is " + std::to_string(oc.h) + " x " + std::to_string(oc.w) + ": sides must be in 1..4096");
      return POCO_ERR_ARG;
    }
    if (oc.offset < 0 || oc.offset + (long long)oc.h * oc.w > atlas_texels) {
      poco_set_error(who + ": cut-out " + std::to_string(k) + " does not lie inside the atlas");
      return POCO_ERR_ARG;
    }
  }
  for (int n = 0; n < N; ++n) {
    const poco_occ_record_t& r = h_occ[n];
    if (r.count < 0 || r.count > POCO_OCC_MAX_OBJECTS) {
      poco_set_error(who + ": crop " + std::to_string(n) + " has " + std::to_string(r.count) + " objects (0.." + std::to_string(POCO_OCC_MAX_OBJECTS) + ")");
      return POCO_ERR_ARG;
    }
    for (int k = 0; k < r.count; ++k) {
      const poco_occ_object_t& ob = r.obj[k];
      const std::string what = who + ": object " + std::to_string(k) + " of crop " + std::to_string(n);
      if (ob.id < 0 || ob.id >= n_occluders) { poco_set_error(what + " names cut-out " + std::to_string(ob.id) + " outside the table"); return POCO_ERR_ARG; }
      const poco_occluder_t& oc = h_occluders[ob.id];
      if (ob.dst_w < 1 || ob.dst_h < 1 || ob.dst_w > oc.w || ob.dst_h > oc.h) {
        poco_set_error(what + " resizes a " + std::to_string(oc.w) + " x " + std::to_string(oc.h) + " cut-out to " + std::to_string(ob.dst_w) + " x " +
                       std::to_string(ob.dst_h) + ": each side must be in 1..source (INTER_AREA only)");
        return POCO_ERR_ARG;
      }
    }
  }
  const int groups = (res + DC_SPAN - 1) / DC_SPAN;
  for (int n0 = 0; n0 < N; n0 += 65535) {             // gridDim.y limit
    const int nn = N - n0 < 65535 ? N - n0 : 65535;
    OccArgs oa{reinterpret_cast<const unsigned int*>(d_atlas), atlas_texels, d_occluders, n_occluders, d_occ + n0,
               d_cover ? d_cover + (size_t)n0 * groups * groups : nullptr, want_mask ? d_mask + (size_t)n0 * res * res : nullptr};
    if (want_mask)
      hipLaunchKernelGGL(dataset_crop_occ_mask_kernel, dim3(groups * groups, nn), dim3(256), 0, (hipStream_t)stream, d_images, d_img_hw,
                         n_images, d_params + n0, d_out + (size_t)n0 * 3 * res * res, res, groups, normalize ? 1 : 0, oa);
    else
      hipLaunchKernelGGL(dataset_crop_occ_kernel, dim3(groups * groups, nn), dim3(256), 0, (hipStream_t)stream, d_images, d_img_hw, n_images,
                         d_params + n0, d_out + (size_t)n0 * 3 * res * res, res, groups, normalize ? 1 : 0, oa);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { poco_set_error(who + ": " + hipGetErrorString(e)); return POCO_ERR_HIP; }
  return POCO_OK;
}

extern "C" int poco_dataset_crop_occ(const unsigned char* const* d_images, const int* d_img_hw, int n_images,
                                     const poco_dataset_crop_param_t* d_params, const poco_dataset_crop_param_t* h_params, int N, int res,
                                     int normalize, const unsigned char* d_atlas, long long atlas_texels, const poco_occluder_t* d_occluders,
                                     const poco_occluder_t* h_occluders, int n_occluders, const poco_occ_record_t* d_occ,
                                     const poco_occ_record_t* h_occ, float* d_out, int* d_cover, void* stream) {
  return crop_occ_entry("poco_dataset_crop_occ", false, d_images, d_img_hw, n_images, d_params, h_params, N, res, normalize, d_atlas,
                        atlas_texels, d_occluders, h_occluders, n_occluders, d_occ, h_occ, d_out, d_cover, nullptr, stream);
}

extern "C" int poco_dataset_crop_occ_mask(const unsigned char* const* d_images, const int* d_img_hw, int n_images,
                                          const poco_dataset_crop_param_t* d_params, const poco_dataset_crop_param_t* h_params, int N,
                                          int res, int normalize, const unsigned char* d_atlas, long long atlas_texels,
                                          const poco_occluder_t* d_occluders, const poco_occluder_t* h_occluders, int n_occluders,
                                          const poco_occ_record_t* d_occ, const poco_occ_record_t* h_occ, float* d_out, int* d_cover,
                                          unsigned char* d_mask, void* stream) {
  return crop_occ_entry("poco_dataset_crop_occ_mask", true, d_images, d_img_hw, n_images, d_params, h_params, N, res, normalize, d_atlas,
                        atlas_texels, d_occluders, h_occluders, n_occluders, d_occ, h_occ, d_out, d_cover, d_mask, stream);
}
