// Per-part visibility counts of SMPL meshes in their crops (eval.py --visibility, poco_amd/visibility.py): how much of every body
// part lies in a window around the crop, how much of that inside the crop, how much of that in front of the rest of the body, and
// how much of that outside a mask of occluded pixels.  The contract is stated in include/poco_hip.h (poco_op_part_visibility) and
// DESIGN.md section 30; tests/visibility_np.py restates it.  Camera, pixel-centre sampling, coverage rule, face exclusions and depth
// rule are those of part_labels.hip: the same expressions in the same order, so `front` counts the labels of poco_op_part_labels.
//
//   vis_raster   per (crop, face): project the three vertices, walk the pixel bounding box clipped to the WINDOW [-margin, res +
//                margin)^2; per covered centre atomicOr(1 << part) into the window's 32-bit word, and inside the frame [0, res)^2
//                also atomicMin the 64-bit depth key of part_labels.hip
//   vis_count    per window pixel (one lane each): the word's bits give total / area, the key's winner gives front / seen; per part
//                one wave64 ballot and popcount per counter, summed over the block's four waves in LDS, then one global integer
//                add per (part, counter) that is not zero.  Integer sums: the order of the additions cannot change the result.
// A fragment is a covered centre whose interpolated depth is finite and positive - the condition under which part_labels.hip draws
// it - in the frame and in the margin alike, so a pixel that counts for `front` always counts for `area` and `total`.
#include "common.h"
#include "kernels.h"
#include "raster_common.h"

// (raster_common.h turns contraction off for the rest of this file too; said again here because the depths depend on it)
#pragma clang fp contract(off)

namespace {

constexpr int VIS_BLOCK = 256;
constexpr int VIS_PARTS = 24;
constexpr float VIS_NEAR = 0.1f;

// perspective_projection with an identity rotation, as part_labels.hip: (x, y) = focal * (X, Y) / Z + res / 2, y down; .z = Z
__device__ __forceinline__ float4 vis_project(const float* __restrict__ v, float tx, float ty, float tz, float focal, float half) {
  const float X = v[0] + tx, Y = v[1] + ty, Z = v[2] + tz;
  return make_float4(focal * X / Z + half, focal * Y / Z + half, Z, 0.f);
}

__global__ __launch_bounds__(VIS_BLOCK) void vis_raster(const float* __restrict__ verts, int V, const float* __restrict__ cam_t,
                                                        const int* __restrict__ faces, int F, const unsigned char* __restrict__ face_part,
                                                        float focal, int res, int margin, unsigned long long* __restrict__ keys,
                                                        unsigned int* __restrict__ bits) {
  const int f = blockIdx.x * VIS_BLOCK + threadIdx.x;
  const int b = blockIdx.y;
  if (f >= F) return;
  const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  if ((unsigned)idx[0] >= (unsigned)V || (unsigned)idx[1] >= (unsigned)V || (unsigned)idx[2] >= (unsigned)V) return;
  const float* vp = verts + (size_t)b * V * 3;
  const float tx = cam_t[3 * b], ty = cam_t[3 * b + 1], tz = cam_t[3 * b + 2];
  const float half = (float)res * 0.5f;
  float4 p[3];
  #pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = vis_project(vp + 3 * idx[k], tx, ty, tz, focal, half);
  if (!(p[0].z >= VIS_NEAR && p[1].z >= VIS_NEAR && p[2].z >= VIS_NEAR)) return;
  if (!(isfinite(p[0].x) && isfinite(p[0].y) && isfinite(p[0].z) && isfinite(p[1].x) && isfinite(p[1].y) && isfinite(p[1].z) &&
        isfinite(p[2].x) && isfinite(p[2].y) && isfinite(p[2].z)))
    return;
  TriSetup t;
  if (!tri_setup_corners(p, idx, t)) return;           // both windings are set up with a positive area: back faces are filled
  // the bounding box is clamped as floats first (one pixel beyond the window), so the float -> int conversions see small numbers
  const float lo = -(float)margin - 1.f, hi = (float)(res + margin) + 1.f;
  const float minx = fmaxf(fminf(fminf(p[0].x, p[1].x), p[2].x), lo), maxx = fminf(fmaxf(fmaxf(p[0].x, p[1].x), p[2].x), hi);
  const float miny = fmaxf(fminf(fminf(p[0].y, p[1].y), p[2].y), lo), maxy = fminf(fmaxf(fmaxf(p[0].y, p[1].y), p[2].y), hi);
  const int c0 = max(-margin, (int)ceilf(minx - 0.5f)), c1 = min(res + margin - 1, (int)floorf(maxx - 0.5f));
  const int r0 = max(-margin, (int)ceilf(miny - 0.5f)), r1 = min(res + margin - 1, (int)floorf(maxy - 0.5f));
  const float ia = 1.f / p[0].z, ib = 1.f / p[1].z, ic = 1.f / p[2].z;
  const unsigned int bit = 1u << min((int)face_part[f], VIS_PARTS - 1);     // a part above 23 is clamped (the host check refuses it)
  const int W = res + 2 * margin;
  unsigned long long* kb = keys + (size_t)b * res * res;
  unsigned int* wb = bits + (size_t)b * W * W;
  for (int r = r0; r <= r1; ++r) {
    const float py = (float)r + 0.5f;
    for (int c = c0; c <= c1; ++c) {
      const float px = (float)c + 0.5f;
      float w[3];
      if (!tri_cover(t, px, py, w)) continue;
      // perspective-correct depth: 1 / z is linear in screen space
      const float iz = (w[0] * ia + w[1] * ib + w[2] * ic) / t.area;
      const float z = 1.f / iz;
      if (!(z > 0.f) || !isfinite(z)) continue;
      atomicOr(wb + (size_t)(r + margin) * W + (c + margin), bit);
      if ((unsigned)r < (unsigned)res && (unsigned)c < (unsigned)res)
        atomicMin(kb + (size_t)r * res + c, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)f);
    }
  }
}

// counts[b][p] = (total, area, front, seen).  No lane leaves before the ballots: a lane past the window carries an empty word.
__global__ __launch_bounds__(VIS_BLOCK) void vis_count(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ bits,
                                                       const unsigned char* __restrict__ face_part, int F,
                                                       const unsigned char* __restrict__ occ_mask, int res, int margin,
                                                       int* __restrict__ counts) {
  __shared__ int cnt[VIS_PARTS * 4];
  const int b = blockIdx.y;
  const int W = res + 2 * margin;
  const int i = blockIdx.x * VIS_BLOCK + threadIdx.x;          // W * W <= 12288^2 < 2^31
  if (threadIdx.x < VIS_PARTS * 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  unsigned int word = 0;
  int winner = -1;
  bool in_frame = false, open = false;
  if (i < W * W) {
    word = bits[(size_t)b * W * W + i];
    const int r = i / W - margin, c = i % W - margin;
    in_frame = (unsigned)r < (unsigned)res && (unsigned)c < (unsigned)res;
    if (in_frame) {
      const size_t q = ((size_t)b * res + r) * res + c;
      const unsigned long long key = keys[q];
      if (key != ~0ull) {
        const unsigned int f = (unsigned int)(key & 0xFFFFFFFFull);
        winner = f < (unsigned)F ? min((int)face_part[f], VIS_PARTS - 1) : -1;     // the key was written by vis_raster: f < F
        open = occ_mask == nullptr || occ_mask[q] == 0;
      }
    }
  }
  const bool lead = (threadIdx.x & 63) == 0;
  #pragma unroll 1
  for (int p = 0; p < VIS_PARTS; ++p) {
    const bool has = (word >> p) & 1u;
    const unsigned long long total = __ballot(has);
    if (total == 0) continue;                                  // wave-uniform; the winner's bit is always set in its pixel's word
    const unsigned long long area = __ballot(has && in_frame);
    const unsigned long long front = __ballot(winner == p);
    const unsigned long long seen = __ballot(winner == p && open);
    if (lead) {
      atomicAdd(&cnt[4 * p], __popcll(total));
      if (area) atomicAdd(&cnt[4 * p + 1], __popcll(area));
      if (front) atomicAdd(&cnt[4 * p + 2], __popcll(front));
      if (seen) atomicAdd(&cnt[4 * p + 3], __popcll(seen));
    }
  }
  __syncthreads();
  if (threadIdx.x < VIS_PARTS * 4 && cnt[threadIdx.x] != 0) atomicAdd(counts + (size_t)b * VIS_PARTS * 4 + threadIdx.x, cnt[threadIdx.x]);
}

}  // namespace

void launch_part_visibility(const float* verts, int B, int V, const float* cam_t, const int* faces, int F, const unsigned char* face_part,
                            float focal, int res, int margin, const unsigned char* occ_mask, unsigned long long* keys, unsigned int* bits,
                            int* counts, hipStream_t s) {
  const int W = res + 2 * margin;
  vis_raster<<<dim3((F + VIS_BLOCK - 1) / VIS_BLOCK, B), VIS_BLOCK, 0, s>>>(verts, V, cam_t, faces, F, face_part, focal, res, margin, keys, bits);
  vis_count<<<dim3((unsigned)(((size_t)W * W + VIS_BLOCK - 1) / VIS_BLOCK), B), VIS_BLOCK, 0, s>>>(keys, bits, face_part, F, occ_mask, res,
                                                                                                   margin, counts);
}
