// Body-part label maps of SMPL meshes in their crops, and the crop camera they are placed with: what the reference trains PARE's
// segmentation head against (pocolib/core/trainer.py:231-262: geometry.estimate_translation, then image_utils.generate_part_labels
// through neural_renderer).  The contract is stated in include/poco_hip.h and DESIGN.md section 21; tests/segm_np.py restates it.
//
//   part_raster    per (crop, face): project the three vertices, walk the pixel bounding box, atomicMin a 64-bit key per covered centre
//   part_resolve   per pixel: key -> face_part[winning face] + 1, or 0 where nothing was drawn
//   est_trans      per crop (one wave): the weighted 3x3 normal equations of estimate_translation_np in fp64, Cramer's rule
// Key = float bits of z << 32 | face: z >= 0.1 is positive, so its bits order as the value does; the smallest key is the nearest
// fragment and, at equal depth, the lower face index.
#include "common.h"
#include "kernels.h"
#include "raster_common.h"

// (raster_common.h turns contraction off for the rest of this file too; said again here because the depths depend on it)
#pragma clang fp contract(off)

namespace {

constexpr int PART_BLOCK = 256;
constexpr float PART_NEAR = 0.1f;

// perspective_projection (geometry.py:480-508) with an identity rotation: (x, y) = focal * (X, Y) / Z + res / 2, y down; .z = Z
__device__ __forceinline__ float4 part_project(const float* __restrict__ v, float tx, float ty, float tz, float focal, float half) {
  const float X = v[0] + tx, Y = v[1] + ty, Z = v[2] + tz;
  return make_float4(focal * X / Z + half, focal * Y / Z + half, Z, 0.f);
}

__global__ __launch_bounds__(PART_BLOCK) void part_raster(const float* __restrict__ verts, int V, const float* __restrict__ cam_t,
                                                          const int* __restrict__ faces, int F, float focal, int res,
                                                          unsigned long long* __restrict__ keys) {
  const int f = blockIdx.x * PART_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (f >= F) return;
  const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  if ((unsigned)idx[0] >= (unsigned)V || (unsigned)idx[1] >= (unsigned)V || (unsigned)idx[2] >= (unsigned)V) return;
  const float* vp = verts + (size_t)b * V * 3;
  const float tx = cam_t[3 * b], ty = cam_t[3 * b + 1], tz = cam_t[3 * b + 2];
  const float half = (float)res * 0.5f;
  float4 p[3];
  #pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = part_project(vp + 3 * idx[k], tx, ty, tz, focal, half);
  // a vertex in front of the near plane (or not a number: the comparison fails) takes the whole face out; a non-finite
  // screen position must not reach the float -> int conversions below
  if (!(p[0].z >= PART_NEAR && p[1].z >= PART_NEAR && p[2].z >= PART_NEAR)) return;
  if (!(isfinite(p[0].x) && isfinite(p[0].y) && isfinite(p[0].z) && isfinite(p[1].x) && isfinite(p[1].y) && isfinite(p[1].z) &&
        isfinite(p[2].x) && isfinite(p[2].y) && isfinite(p[2].z)))
    return;
  TriSetup t;
  if (!tri_setup_corners(p, idx, t)) return;           // both windings are set up with a positive area: back faces are filled
  const float lim = (float)res + 1.f;
  const float minx = fmaxf(fminf(fminf(p[0].x, p[1].x), p[2].x), -1.f), maxx = fminf(fmaxf(fmaxf(p[0].x, p[1].x), p[2].x), lim);
  const float miny = fmaxf(fminf(fminf(p[0].y, p[1].y), p[2].y), -1.f), maxy = fminf(fmaxf(fmaxf(p[0].y, p[1].y), p[2].y), lim);
  const int c0 = max(0, (int)ceilf(minx - 0.5f)), c1 = min(res - 1, (int)floorf(maxx - 0.5f));
  const int r0 = max(0, (int)ceilf(miny - 0.5f)), r1 = min(res - 1, (int)floorf(maxy - 0.5f));
  const float ia = 1.f / p[0].z, ib = 1.f / p[1].z, ic = 1.f / p[2].z;
  unsigned long long* kb = keys + (size_t)b * res * res;
  for (int r = r0; r <= r1; ++r) {
    const float py = (float)r + 0.5f;
    for (int c = c0; c <= c1; ++c) {
      const float px = (float)c + 0.5f;
      float w[3];
      if (!tri_cover(t, px, py, w)) continue;
      // perspective-correct depth: 1 / z is linear in screen space
      const float iz = (w[0] * ia + w[1] * ib + w[2] * ic) / t.area;
      const float z = 1.f / iz;
      if (!(z > 0.f) || !isfinite(z)) continue;                        // keeps the key's ordering argument honest
      atomicMin(kb + (size_t)r * res + c, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)f);
    }
  }
}

__global__ __launch_bounds__(PART_BLOCK) void part_resolve(const unsigned long long* __restrict__ keys, const unsigned char* __restrict__ face_part,
                                                           size_t n, unsigned char* __restrict__ labels) {
  const size_t i = (size_t)blockIdx.x * PART_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  labels[i] = key == ~0ull ? (unsigned char)0 : (unsigned char)(face_part[(unsigned)(key & 0xFFFFFFFFull)] + 1);
}

// estimate_translation_np (geometry.py:511-551).  Per joint two rows of Q = w * [[F, 0, cx - x], [0, F, cy - y]] and of
// c = w * [(x - cx) Z - F X, (y - cy) Z - F Y], w = sqrt(conf) taken in float32 as the reference takes it; A = Q^T Q and b = Q^T c are
// summed in fp64 in joint order (A01 = 0 and A11 = A00 by construction).  Lane j forms the terms of joint j, lanes 0..8 each add one
// term over the joints, lane 0 solves.
constexpr int EST_TERMS = 9;   // A00, A02, A12, A22, b0, b1, b2 (+ 2 unused)
__global__ __launch_bounds__(64) void est_trans(const float* __restrict__ j3d, const float* __restrict__ j2d, int J, float focal, int res,
                                                float* __restrict__ cam_t) {
  __shared__ double term[EST_TERMS][POCO_EST_MAX_JOINTS];
  __shared__ double sum[EST_TERMS];
  const int b = blockIdx.x, l = threadIdx.x;
  if (l < J) {
    const float* S = j3d + ((size_t)b * J + l) * 3;
    const float* k = j2d + ((size_t)b * J + l) * 3;
    const double F = (double)focal, ctr = (double)res / 2.0;
    const double w = (double)sqrtf(k[2]);
    const double X = S[0], Y = S[1], Z = S[2], x = k[0], y = k[1];
    const double qx0 = w * F, qx2 = w * (ctr - x), qy2 = w * (ctr - y);
    const double cx = w * ((x - ctr) * Z - F * X), cy = w * ((y - ctr) * Z - F * Y);
    term[0][l] = qx0 * qx0;
    term[1][l] = qx0 * qx2;
    term[2][l] = qx0 * qy2;
    term[3][l] = qx2 * qx2 + qy2 * qy2;
    term[4][l] = qx0 * cx;
    term[5][l] = qx0 * cy;
    term[6][l] = qx2 * cx + qy2 * cy;
  }
  __syncthreads();
  if (l < 7) {
    double s = 0.0;
    for (int j = 0; j < J; ++j) s += term[l][j];
    sum[l] = s;
  }
  __syncthreads();
  if (l == 0) {
    const double a = sum[0], c = sum[1], e = sum[2], g = sum[3], b0 = sum[4], b1 = sum[5], b2 = sum[6];
    // A = [[a, 0, c], [0, a, e], [c, e, g]]
    const double det = a * (a * g - e * e) - c * (a * c);
    float tx = 1.f, ty = 1.f, tz = 1.f;               // the reference's `except` branch: a singular system gives (1, 1, 1)
    if (det != 0.0 && det - det == 0.0) {
      const double d0 = b0 * (a * g - e * e) + c * (b1 * e - a * b2);
      const double d1 = a * (b1 * g - e * b2) - b0 * (0.0 - c * e) + c * (0.0 - b1 * c);
      const double d2 = a * (a * b2 - b1 * e) + b0 * (0.0 - a * c);
      tx = (float)(d0 / det); ty = (float)(d1 / det); tz = (float)(d2 / det);
    }
    cam_t[3 * b] = tx; cam_t[3 * b + 1] = ty; cam_t[3 * b + 2] = tz;
  }
}

}  // namespace

void launch_part_labels(const float* verts, int B, int V, const float* cam_t, const int* faces, int F, const unsigned char* face_part,
                        float focal, int res, unsigned long long* keys, unsigned char* labels, hipStream_t s) {
  const size_t n = (size_t)B * res * res;
  part_raster<<<dim3((F + PART_BLOCK - 1) / PART_BLOCK, B), PART_BLOCK, 0, s>>>(verts, V, cam_t, faces, F, focal, res, keys);
  part_resolve<<<(unsigned)((n + PART_BLOCK - 1) / PART_BLOCK), PART_BLOCK, 0, s>>>(keys, face_part, n, labels);
}

void launch_estimate_translation(const float* j3d, const float* j2d, int B, int J, float focal, int res, float* cam_t, hipStream_t s) {
  est_trans<<<B, 64, 0, s>>>(j3d, j2d, J, focal, res, cam_t);
}
