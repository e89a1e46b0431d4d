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
#include "../../include/poco_hip.h"
#include "common.h"
#include "crop_affine.h"
#include <cmath>

namespace {
constexpr int DC_TILE = 16, DC_GROUP = 2;          // tile side; tiles per block side
constexpr int DC_SPAN = DC_TILE * DC_GROUP;        // output pixels per block side

__global__ void __launch_bounds__(256)
dataset_crop_kernel(const unsigned char* const* __restrict__ images, const int* __restrict__ img_hw, int n_images,
                    const poco_dataset_crop_param_t* __restrict__ params, float* __restrict__ out, int res, int groups_x, int normalize) {
#pragma clang fp contract(off)
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
    float* o = out + (((size_t)n * 3) * res + y) * res + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // acc <= 255 * 1024 < 2^24: exact in float32, and so is the division by 1024
      float v = (float)acc[c] * (1.0f / 1024.0f);
      v = fminf(255.0f, fmaxf(0.0f, v * pn[c]));          // base_dataset.py:216-218 on a float32 array (pn rounded to float32)
      if (normalize) v = (v / 255.0f - mean[c]) / stdv[c];  // base_dataset.py:220 and normalize_img, float32
      o[c * cs] = v;
    }
  }
}
}  // namespace

extern "C" int poco_dataset_crop(const unsigned char* const* d_images, const int* d_img_hw, int n_images,
                                 const poco_dataset_crop_param_t* d_params, const poco_dataset_crop_param_t* h_params, int N, int res,
                                 int normalize, float* d_out, void* stream) {
  if (!d_images || !d_img_hw || !d_params || !h_params || !d_out) { poco_set_error("poco_dataset_crop: null pointer"); return POCO_ERR_ARG; }
  if (N < 1 || n_images < 1) { poco_set_error("poco_dataset_crop: N and n_images must be at least 1"); return POCO_ERR_ARG; }
  if (res < 1 || res > 4096) { poco_set_error("poco_dataset_crop: res must be in 1..4096"); return POCO_ERR_ARG; }
  for (int n = 0; n < N; ++n) {
    const poco_dataset_crop_param_t& p = h_params[n];
    bool finite = true;
    for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(p.src[k]);
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(p.pn[k]);
    if (!finite) { poco_set_error("poco_dataset_crop: crop " + std::to_string(n) + " has a non-finite parameter"); return POCO_ERR_ARG; }
    if (p.bb < 1) {
      poco_set_error("poco_dataset_crop: the box side of crop " + std::to_string(n) + " rounds to " + std::to_string(p.bb) + " pixels");
      return POCO_ERR_ARG;
    }
  }
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
