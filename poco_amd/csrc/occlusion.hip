// Occlusion sensitivity sweep (demo.py --occlusion_map): the three kernels around the engine's forwards.
//   occlude_batch      one normalised crop -> m copies with a constant square painted in     (pure copy + select)
//   occlusion_records  each occluded row's engine outputs against the baseline row          (77 floats per position)
//   heat_overlay       a per-position scalar field -> per-pixel mean over the covering patches -> jet -> 50 % blend over the crop
// Declarations + contracts: include/poco_hip.h (poco_op_occlude_batch / poco_op_occlusion_records / poco_op_heat_overlay);
// numpy restatement: tests/occlusion_np.py.
#include "kernels.h"

// ---- A: occluded copies -------------------------------------------------------------------------------------------------------
// One thread per float4 (four consecutive columns of one row of one channel of one copy): a 16-byte load of the source, a
// per-element select, a 16-byte store.  A patch edge inside the quad costs nothing extra: the select is per element.  pos is
// device data and only feeds the select, never an address.
__global__ void __launch_bounds__(256) occlude_batch_kernel(const float4* __restrict__ src, const int* __restrict__ pos, int m, int res,
                                                            int patch, float f0, float f1, float f2, float4* __restrict__ out) {
  const int q = res >> 2;                                   // float4 per row
  const int per_copy = 3 * res * q;
  const long long total = (long long)m * per_copy;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int copy = (int)(i / per_copy);
  const int r = (int)(i - (long long)copy * per_copy);      // float4 index inside the crop
  const int c = r / (res * q);
  const int y = (r - c * res * q) / q;
  const int x = (r - (c * res + y) * q) * 4;
  const int y0 = pos[2 * copy], x0 = pos[2 * copy + 1];
  float4 v = src[r];
  if (y >= y0 && y < y0 + patch) {
    const float f = c == 0 ? f0 : (c == 1 ? f1 : f2);
    if (x + 0 >= x0 && x + 0 < x0 + patch) v.x = f;
    if (x + 1 >= x0 && x + 1 < x0 + patch) v.y = f;
    if (x + 2 >= x0 && x + 2 < x0 + patch) v.z = f;
    if (x + 3 >= x0 && x + 3 < x0 + patch) v.w = f;
  }
  out[i] = v;
}

void launch_occlude_batch(const float* src, const int* pos, int m, int res, int patch, const float* fill3, float* out,
                          hipStream_t s) {
  const long long total = (long long)m * 3 * res * (res >> 2);
  const unsigned blocks = (unsigned)((total + 255) / 256);
  occlude_batch_kernel<<<blocks, 256, 0, s>>>(reinterpret_cast<const float4*>(src), pos, m, res, patch, fill3[0], fill3[1], fill3[2],
                                              reinterpret_cast<float4*>(out));
}

// ---- B: records ---------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per position.  Memory-bound: 2 x V x 12 bytes per row (the baseline row stays in L2 across the
// grid).  A row of V x 3 floats starts on an 8-byte boundary when V is even (SMPL: 6890), so a thread reads two vertices as three
// float2 (24 contiguous bytes; a wave covers 1536 contiguous bytes in its three loads).
// Reduction order (fixed; no atomics): thread t sums the distances of vertex pairs t, t + 256, ... in that order (first vertex of
// a pair, then the second), the 64 lanes of a wave combine through __shfl_down with offsets 32, 16, 8, 4, 2, 1, lane 0 of each
// wave leaves its partial in LDS, thread 0 adds the four partials in wave order.  The maximum goes the same way.
constexpr int OCC_REC = 77;        // include/poco_hip.h POCO_OCCLUSION_RECORD_FLOATS
constexpr int OCC_THREADS = 256;

__device__ __forceinline__ float occ_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ void __launch_bounds__(OCC_THREADS) occlusion_records_kernel(const float* __restrict__ verts, const float* __restrict__ var,
                                                                        const float* __restrict__ j3d, int V,
                                                                        const float* __restrict__ base_verts,
                                                                        const float* __restrict__ base_var,
                                                                        const float* __restrict__ base_j3d, float* __restrict__ rec) {
  __shared__ float s_sum[OCC_THREADS / 64], s_max[OCC_THREADS / 64];
  __shared__ float s_var[24], s_dvar[24];
  const int row = blockIdx.x, t = threadIdx.x;
  const float2* a = reinterpret_cast<const float2*>(verts + (size_t)row * V * 3);
  const float2* b = reinterpret_cast<const float2*>(base_verts);
  float sum = 0.f, mx = 0.f;
  for (int p = t; p < (V >> 1); p += OCC_THREADS) {          // V is even (checked by the caller)
    const float2 a0 = a[3 * p], a1 = a[3 * p + 1], a2 = a[3 * p + 2];
    const float2 b0 = b[3 * p], b1 = b[3 * p + 1], b2 = b[3 * p + 2];
    const float d0 = occ_dist(a0.x, a0.y, a1.x, b0.x, b0.y, b1.x);
    const float d1 = occ_dist(a1.y, a2.x, a2.y, b1.y, b2.x, b2.y);
    sum += d0;
    sum += d1;
    mx = fmaxf(mx, fmaxf(d0, d1));
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
  }
  if ((t & 63) == 0) { s_sum[t >> 6] = sum; s_max[t >> 6] = mx; }
  float* out = rec + (size_t)row * OCC_REC;
  if (t < 24) {
    const float vo = var[(size_t)row * 24 + t];
    const float d = vo - base_var[t];
    s_var[t] = vo;
    s_dvar[t] = d;
    out[4 + t] = d;
  } else if (t >= 64 && t < 64 + 49) {
    const int k = t - 64;
    const float* jo = j3d + ((size_t)row * 49 + k) * 3;
    out[28 + k] = occ_dist(jo[0], jo[1], jo[2], base_j3d[3 * k], base_j3d[3 * k + 1], base_j3d[3 * k + 2]);
  }
  __syncthreads();
  if (t == 0) {
    float s = s_sum[0], m = s_max[0];
    for (int w = 1; w < OCC_THREADS / 64; ++w) { s += s_sum[w]; m = fmaxf(m, s_max[w]); }
    float sv = 0.f, sd = 0.f;
    for (int k = 0; k < 24; ++k) { sv += s_var[k]; sd += s_dvar[k]; }
    out[0] = s / (float)V;
    out[1] = m;
    out[2] = sv / 24.f;
    out[3] = sd / 24.f;
  }
}

void launch_occlusion_records(const float* verts, const float* var, const float* j3d, int m, int V, const float* base_verts,
                              const float* base_var, const float* base_j3d, float* rec, hipStream_t s) {
  occlusion_records_kernel<<<m, OCC_THREADS, 0, s>>>(verts, var, j3d, V, base_verts, base_var, base_j3d, rec);
}

// ---- C: heat map over the crop ------------------------------------------------------------------------------------------------
// One thread per pixel.  Every block first finds the field's maximum itself when the scale is "auto" (n is a few hundred floats;
// a maximum does not depend on the order it is taken in, NaN entries are skipped), so the call stays one launch without scratch.
// The per-pixel arithmetic is spelled with __fadd_rn / __fdiv_rn / __fmul_rn so that no two operations are contracted: the bytes
// equal the float32 numpy restatement.  pos and field are read at wave-uniform addresses (every lane the same entry).
__global__ void __launch_bounds__(256) heat_overlay_kernel(const float* __restrict__ field, const int* __restrict__ pos, int n,
                                                           int patch, int res, float scale, const unsigned char* __restrict__ lut,
                                                           const unsigned char* crop, unsigned char* out) {
  __shared__ float s_max[4];
  const int t = threadIdx.x;
  if (!(scale > 0.f)) {                                         // "auto" (wave-uniform: scale is a kernel argument)
    float mx = -INFINITY;
    for (int i = t; i < n; i += 256) mx = fmaxf(mx, field[i]);  // fmaxf returns the other operand for a NaN
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off, 64));
    if ((t & 63) == 0) s_max[t >> 6] = mx;
    __syncthreads();
    scale = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  }
  const int pix = blockIdx.x * 256 + t;
  if (pix >= res * res) return;
  const int y = pix / res, x = pix - y * res;
  unsigned char p0 = crop[3 * pix], p1 = crop[3 * pix + 1], p2 = crop[3 * pix + 2];
  float sum = 0.f;
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    const int y0 = pos[2 * i], x0 = pos[2 * i + 1];
    if (y >= y0 && y < y0 + patch && x >= x0 && x < x0 + patch) {
      sum = __fadd_rn(sum, field[i]);
      ++cnt;
    }
  }
  if (cnt > 0 && scale > 0.f && scale < INFINITY) {             // otherwise (no patch here, a field without a positive maximum): unchanged
    float tt = __fdiv_rn(__fdiv_rn(sum, (float)cnt), scale);
    if (!(tt > 0.f)) tt = 0.f;                                  // NaN and negative values: the cold end
    if (tt > 1.f) tt = 1.f;
    const int idx = (int)__fadd_rn(__fmul_rn(255.f, tt), 0.5f);
    p0 = (unsigned char)((128 * lut[3 * idx] + 128 * p0 + 128) >> 8);
    p1 = (unsigned char)((128 * lut[3 * idx + 1] + 128 * p1 + 128) >> 8);
    p2 = (unsigned char)((128 * lut[3 * idx + 2] + 128 * p2 + 128) >> 8);
  }
  out[3 * pix] = p0;
  out[3 * pix + 1] = p1;
  out[3 * pix + 2] = p2;
}

void launch_heat_overlay(const float* field, const int* pos, int n, int patch, int res, float scale, const unsigned char* lut,
                         const unsigned char* crop, unsigned char* out, hipStream_t s) {
  heat_overlay_kernel<<<(res * res + 255) / 256, 256, 0, s>>>(field, pos, n, patch, res, scale, lut, crop, out);
}
