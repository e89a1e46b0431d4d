// Mesh rasteriser + compositor of the demo's uncertainty-coloured SMPL overlay: replaces pyrender's offscreen render of
// pocolib/utils/vibe_renderer.py:88-151 as pocolib/core/tester.py:248-345 (folder mode) and :482-580 (video mode) call it.
// The contract (camera, fill rule, depth, painter order, shading) is stated in include/poco_hip.h and DESIGN.md
// "Renderer"; tests/render_np.py restates it in numpy.
//
// Three launches per call, all on the caller's stream, after one memset of the visibility buffer:
//   render_vertices   per (person, vertex): screen position, depth, unit shading normal (gathered through the vertex -> face CSR)
//   render_raster     per (person, triangle): walk the pixel bounding box, atomicMin a 64-bit key per covered pixel centre
//   render_shade      per pixel: decode the key, recompute the barycentrics, shade, write RGB over the frame
// Key = (P - 1 - person) << 54 | float bits of (1 - q_z) << 22 | triangle: the smallest key is the LATEST person (painter's
// order between people), then the nearest fragment, then the lower triangle index.
// The wireframe call (POCO_RENDER_WIREFRAME, DESIGN.md "Wireframe, keypoints and the crop canvas") swaps the raster and shade
// launches for render_wire_raster (per (person, triangle edge)) and render_wire_shade; render_discs stamps the keypoints.
#include "common.h"
#include "kernels.h"
#include "raster_common.h"

// The numpy restatement evaluates the same expressions in float32 without fused multiply-adds; keep hipcc from contracting
// them, so coverage decisions and depths agree bit for bit.
#pragma clang fp contract(off)

namespace {

constexpr int RENDER_BLOCK = 256;
constexpr float RENDER_PI = 3.14159265358979323846f;

// TriSetup / tri_setup / tri_cover (the watertight coverage rule): raster_common.h, shared with part_labels.hip

__global__ __launch_bounds__(RENDER_BLOCK) void render_vertices(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                                const int* __restrict__ csr_off, const int* __restrict__ csr_face,
                                                                RenderXform xf, const float* __restrict__ params, int H, int W,
                                                                float4* __restrict__ pos, float4* __restrict__ nrm) {
  const int v = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  const int p = blockIdx.y;
  if (v >= V) return;
  const float* vp = verts + (size_t)p * V * 3;
  const float* m = xf.m;
  const float x = vp[3 * v], y = vp[3 * v + 1], z = vp[3 * v + 2];
  const float qx = m[0] * x + m[1] * y + m[2] * z;
  const float qy = m[3] * x + m[4] * y + m[5] * z;
  const float qz = m[6] * x + m[7] * y + m[8] * z;
  const float* cam = params + (size_t)p * RENDER_PARAMS;          // (sx, sy, tx, ty, ...)
  const float col = (W * 0.5f) * (1.f + cam[0] * (qx + cam[2]));
  const float row = (H * 0.5f) * (1.f - cam[1] * (qy - cam[3]));
  // area-weighted vertex normal in the model frame: sum of the (unnormalised) cross products of the incident faces, in face order
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int k = csr_off[v]; k < csr_off[v + 1]; ++k) {
    const int f = csr_face[k];
    const float* a = vp + 3 * faces[3 * f];
    const float* b = vp + 3 * faces[3 * f + 1];
    const float* c = vp + 3 * faces[3 * f + 2];
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    nx += uy * wz - uz * wy;
    ny += uz * wx - ux * wz;
    nz += ux * wy - uy * wx;
  }
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  if (len > 0.f) { nx /= len; ny /= len; nz /= len; }
  const size_t o = (size_t)p * V + v;
  pos[o] = make_float4(col, row, qz, 0.f);
  nrm[o] = make_float4(m[0] * nx + m[1] * ny + m[2] * nz, m[3] * nx + m[4] * ny + m[5] * nz, m[6] * nx + m[7] * ny + m[8] * nz, 0.f);
}

__global__ __launch_bounds__(RENDER_BLOCK) void render_raster(const float4* __restrict__ pos, int V, const int* __restrict__ faces,
                                                              int F, int P, int H, int W, unsigned long long* __restrict__ vis,
                                                              int* __restrict__ count) {
  const int f = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  const int p = blockIdx.y;
  if (f >= F) return;
  const float4* pp = pos + (size_t)p * V;
  const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  const float4 a = pp[idx[0]], b = pp[idx[1]], c = pp[idx[2]];
  // a non-finite vertex (a diverged regression) covers nothing; it must not reach the float -> int conversions below
  if (!(isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z) &&
        isfinite(c.x) && isfinite(c.y) && isfinite(c.z)))
    return;
  TriSetup t;
  if (!tri_setup(pp, idx, t)) return;
  // pixel (r, c) is sampled at (c + 0.5, r + 0.5): columns whose centre lies in [min x, max x], clamped to the frame
  const float minx = fmaxf(fminf(fminf(a.x, b.x), c.x), -1.f), maxx = fminf(fmaxf(fmaxf(a.x, b.x), c.x), (float)W + 1.f);
  const float miny = fmaxf(fminf(fminf(a.y, b.y), c.y), -1.f), maxy = fminf(fmaxf(fmaxf(a.y, b.y), c.y), (float)H + 1.f);
  const int c0 = max(0, (int)ceilf(minx - 0.5f)), c1 = min(W - 1, (int)floorf(maxx - 0.5f));
  const int r0 = max(0, (int)ceilf(miny - 0.5f)), r1 = min(H - 1, (int)floorf(maxy - 0.5f));
  const unsigned long long order = (unsigned long long)(P - 1 - p) << 54;
  for (int r = r0; r <= r1; ++r) {
    const float py = (float)r + 0.5f;
    for (int cc = c0; cc <= c1; ++cc) {
      const float px = (float)cc + 0.5f;
      float w[3];
      if (!tri_cover(t, px, py, w)) continue;
      const float z = (w[0] * a.z + w[1] * b.z + w[2] * c.z) / t.area;
      if (!(fabsf(z) <= 1.f)) continue;                              // GL clipping: NDC z = -q_z outside [-1, 1]
      const unsigned long long key = order | ((unsigned long long)__float_as_uint(1.f - z) << 22) | (unsigned long long)f;
      atomicMin(vis + (size_t)r * W + cc, key);
      if (count) atomicAdd(count + (size_t)r * W + cc, 1);
    }
  }
}

__device__ __forceinline__ float sq(float x) { return x * x; }

// pyrender's metallic-roughness shading with l = v = h = +z (three directional lights along -z, ambient 0.3) of a fragment whose
// unit normal has z component nz; pr = the person's parameters; writes the three bytes of the pixel
__device__ __forceinline__ void shade_write(float nz, const float* __restrict__ pr, unsigned char* __restrict__ out) {
  const float cth = fminf(fmaxf(nz, 0.f), 1.f);
  const bool plain = pr[7] != 0.f;
  const float metal = plain ? 0.f : 0.2f, rough = plain ? 1.f : 0.8f;
  const float alpha = rough * rough, a2 = alpha * alpha;
  const float D = a2 / (RENDER_PI * sq(cth * cth * (a2 - 1.f) + 1.f));
  const float G = sq(2.f * cth / (cth + sqrtf(a2 + (1.f - a2) * cth * cth)));
  #pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float base = pr[4 + ch];
    const float F0 = 0.04f * (1.f - metal) + base * metal;
    const float cdiff = base * 0.96f * (1.f - metal);
    const float per = cth * ((1.f - F0) * cdiff / RENDER_PI + F0 * G * D / (4.f * cth * cth + 0.001f));
    const float colour = 3.f * per + 0.3f * base;
    const float g = fminf(fmaxf(powf(colour, 1.f / 2.2f), 0.f), 1.f);
    out[ch] = (unsigned char)rintf(255.f * g);
  }
}

__global__ __launch_bounds__(RENDER_BLOCK) void render_shade(const float4* __restrict__ pos, const float4* __restrict__ nrm, int V,
                                                             const int* __restrict__ faces, const float* __restrict__ params, int P,
                                                             int H, int W, const unsigned long long* __restrict__ vis,
                                                             unsigned char* __restrict__ frame) {
  const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  if (i >= H * W) return;
  const unsigned long long key = vis[i];
  if (key == ~0ull) return;                                          // no person covers this pixel: the input bytes stay
  const int p = P - 1 - (int)(key >> 54);
  const int f = (int)(key & ((1u << 22) - 1));
  const float4* pp = pos + (size_t)p * V;
  const float4* np_ = nrm + (size_t)p * V;
  const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  TriSetup t;
  tri_setup(pp, idx, t);
  float w[3];
  tri_cover(t, (float)(i % W) + 0.5f, (float)(i / W) + 0.5f, w);
  // the interpolated normal is renormalised, so the barycentric weights need not be divided by the area
  const float4 n0 = np_[idx[0]], n1 = np_[idx[1]], n2 = np_[idx[2]];
  float nx = w[0] * n0.x + w[1] * n1.x + w[2] * n2.x;
  float ny = w[0] * n0.y + w[1] * n1.y + w[2] * n2.y;
  float nz = w[0] * n0.z + w[1] * n1.z + w[2] * n2.z;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  nz = len > 0.f ? nz / len : 0.f;
  shade_write(nz, params + (size_t)p * RENDER_PARAMS, frame + (size_t)i * 3);
}

// ---- wireframe (RenderFlags.ALL_WIREFRAME of vibe_renderer.py:133-136: GL polygon mode LINE, depth test and back-face culling on) ----
// One edge of a triangle as a one-pixel line.  Edge e is the edge opposite vertex e, as in TriSetup, and is always walked from
// its lower vertex index (A) to its higher one (B), so the two triangles that share it generate bit-identical fragments.  The
// major axis (coordinate a) is the one with the larger |delta|, a tie goes to columns; b is the minor coordinate.
struct WireEdge {
  int A, B;
  float a0, a1, b0, b1;
  bool cols;                          // major axis = columns
};

// false = the edge draws nothing (a repeated vertex index, a non-finite endpoint or no extent along the major axis)
__device__ __forceinline__ bool wire_edge(const float4* pos, const int* idx, int e, WireEdge& w) {
  const int u = idx[(e + 1) % 3], v = idx[(e + 2) % 3];
  if (u == v) return false;
  w.A = u < v ? u : v;
  w.B = u < v ? v : u;
  const float4 PA = pos[w.A], PB = pos[w.B];
  if (!(isfinite(PA.x) && isfinite(PA.y) && isfinite(PA.z) && isfinite(PB.x) && isfinite(PB.y) && isfinite(PB.z))) return false;
  w.cols = fabsf(PB.x - PA.x) >= fabsf(PB.y - PA.y);
  w.a0 = w.cols ? PA.x : PA.y; w.a1 = w.cols ? PB.x : PB.y;
  w.b0 = w.cols ? PA.y : PA.x; w.b1 = w.cols ? PB.y : PB.x;
  return w.a0 != w.a1;
}

// parameter of the centre of major-axis pixel i along the edge, 0 at A and 1 at B
__device__ __forceinline__ float wire_t(const WireEdge& w, int i) { return ((float)i + 0.5f - w.a0) / (w.a1 - w.a0); }

// per (person, triangle edge): cull, walk the major axis, atomicMin one key per fragment.  Key as in the filled path with
// (triangle << 2 | edge) in the low 22 bits.
__global__ __launch_bounds__(RENDER_BLOCK) void render_wire_raster(const float* __restrict__ verts, const float4* __restrict__ pos, int V,
                                                                   const int* __restrict__ faces, int F, RenderXform xf, int P, int H,
                                                                   int W, unsigned long long* __restrict__ vis,
                                                                   int* __restrict__ count) {
  const int g = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  const int p = blockIdx.y;
  if (g >= 3 * F) return;
  const int f = g / 3, e = g - 3 * f;
  const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  // front-facing: ((q1 - q0) x (q2 - q0)).z > 0 in the transformed space (GL counter-clockwise, camera looking down -z); the
  // same expressions as render_vertices.  A zero-area or non-finite triangle fails the comparison and draws nothing.
  const float* vp = verts + (size_t)p * V * 3;
  const float* m = xf.m;
  float qx[3], qy[3];
  #pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = vp[3 * idx[k]], y = vp[3 * idx[k] + 1], z = vp[3 * idx[k] + 2];
    qx[k] = m[0] * x + m[1] * y + m[2] * z;
    qy[k] = m[3] * x + m[4] * y + m[5] * z;
  }
  const float facing = (qx[1] - qx[0]) * (qy[2] - qy[0]) - (qy[1] - qy[0]) * (qx[2] - qx[0]);
  if (!(facing > 0.f)) return;
  const float4* pp = pos + (size_t)p * V;
  WireEdge w;
  if (!wire_edge(pp, idx, e, w)) return;
  const float z0 = pp[w.A].z, z1 = pp[w.B].z;
  const int nmaj = w.cols ? W : H, nmin = w.cols ? H : W;
  // major-axis pixel i is covered when lo <= i + 0.5 < hi: a candidate range from the clamped bounds, the rule itself per pixel
  const float lo = fminf(w.a0, w.a1), hi = fmaxf(w.a0, w.a1);
  // (both bounds clamped on both sides, so the float -> int conversions stay defined for any finite coordinate)
  const float top = (float)nmaj + 1.f;
  const int i0 = max(0, (int)ceilf(fminf(fmaxf(lo, -1.f), top) - 0.5f)), i1 = min(nmaj - 1, (int)floorf(fminf(fmaxf(hi, -1.f), top) - 0.5f));
  const unsigned long long order = (unsigned long long)(P - 1 - p) << 54;
  for (int i = i0; i <= i1; ++i) {
    const float c = (float)i + 0.5f;
    if (!(lo <= c && c < hi)) continue;
    const float t = wire_t(w, i);
    const float b = floorf(w.b0 + t * (w.b1 - w.b0));
    if (!(b >= 0.f && b < (float)nmin)) continue;                   // outside the frame (or not a number)
    const float z = z0 + t * (z1 - z0);
    if (!(fabsf(z) <= 1.f)) continue;                               // GL clipping, as the filled path
    const size_t pix = w.cols ? (size_t)(int)b * W + i : (size_t)i * W + (int)b;
    const unsigned long long key = order | ((unsigned long long)__float_as_uint(1.f - z) << 22) | (unsigned long long)(f << 2 | e);
    atomicMin(vis + pix, key);
    if (count) atomicAdd(count + pix, 1);
  }
}

// per pixel: decode (person, triangle, edge), recompute t with the same setup code, interpolate and renormalise the normal, shade
__global__ __launch_bounds__(RENDER_BLOCK) void render_wire_shade(const float4* __restrict__ pos, const float4* __restrict__ nrm, int V,
                                                                  const int* __restrict__ faces, const float* __restrict__ params,
                                                                  int P, int H, int W, const unsigned long long* __restrict__ vis,
                                                                  unsigned char* __restrict__ frame) {
  const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  if (i >= H * W) return;
  const unsigned long long key = vis[i];
  if (key == ~0ull) return;                                          // no line covers this pixel: the input bytes stay
  const int p = P - 1 - (int)(key >> 54);
  const int id = (int)(key & ((1u << 22) - 1));
  const int f = id >> 2, e = id & 3;
  const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
  WireEdge w;
  wire_edge(pos + (size_t)p * V, idx, e, w);
  const float t = wire_t(w, w.cols ? i % W : i / W);
  const float4 nA = nrm[(size_t)p * V + w.A], nB = nrm[(size_t)p * V + w.B];
  const float nx = nA.x + t * (nB.x - nA.x), ny = nA.y + t * (nB.y - nA.y);
  float nz = nA.z + t * (nB.z - nA.z);
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  nz = len > 0.f ? nz / len : 0.f;
  shade_write(nz, params + (size_t)p * RENDER_PARAMS, frame + (size_t)i * 3);
}

// test hook (POCO_RENDER_IDS): the winning primitive id of each pixel (the low 22 bits of its key), -1 where nothing was drawn
__global__ __launch_bounds__(RENDER_BLOCK) void render_ids(const unsigned long long* __restrict__ vis, int n, int* __restrict__ ids) {
  const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = vis[i];
  ids[i] = key == ~0ull ? -1 : (int)(key & ((1u << 22) - 1));
}

// ---- keypoint discs (cv2.circle(img, (int(x), int(y)), r, colour, -1) of tester.py:324-328,552-554) ---------------------------
// per pixel: the highest-index point whose stamp covers it wins (points are painted in index order), found by a scan from the
// last point down - no atomics, deterministic.  A point is truncated toward zero; one that is not finite or beyond 2^30 in
// magnitude paints nothing.
__global__ __launch_bounds__(RENDER_BLOCK) void render_discs(unsigned char* __restrict__ frame, int H, int W,
                                                             const float* __restrict__ points, const unsigned char* __restrict__ rgb,
                                                             int N, int r, DiscRows rows) {
  const int i = blockIdx.x * RENDER_BLOCK + threadIdx.x;
  if (i >= H * W) return;
  const int col = i % W, row = i / W;
  for (int k = N - 1; k >= 0; --k) {
    const float x = points[2 * k], y = points[2 * k + 1];
    if (!(fabsf(x) < 1073741824.f && fabsf(y) < 1073741824.f)) continue;
    const int dy = abs(row - (int)y);
    if (dy > r) continue;
    if (abs(col - (int)x) > rows.hw[dy]) continue;
    frame[(size_t)i * 3] = rgb[3 * k];
    frame[(size_t)i * 3 + 1] = rgb[3 * k + 1];
    frame[(size_t)i * 3 + 2] = rgb[3 * k + 2];
    return;
  }
}

}  // namespace

void launch_render(const float* verts, int P, int V, const int* faces, int F, const int* csr_off, const int* csr_face,
                   const RenderXform& xf, const float* params, int H, int W, float4* pos, float4* nrm, unsigned long long* vis,
                   int* count, unsigned char* frame, hipStream_t s) {
  render_vertices<<<dim3((V + RENDER_BLOCK - 1) / RENDER_BLOCK, P), RENDER_BLOCK, 0, s>>>(verts, V, faces, csr_off, csr_face, xf,
                                                                                         params, H, W, pos, nrm);
  render_raster<<<dim3((F + RENDER_BLOCK - 1) / RENDER_BLOCK, P), RENDER_BLOCK, 0, s>>>(pos, V, faces, F, P, H, W, vis, count);
  render_shade<<<(H * W + RENDER_BLOCK - 1) / RENDER_BLOCK, RENDER_BLOCK, 0, s>>>(pos, nrm, V, faces, params, P, H, W, vis, frame);
}

void launch_render_wire(const float* verts, int P, int V, const int* faces, int F, const int* csr_off, const int* csr_face,
                        const RenderXform& xf, const float* params, int H, int W, float4* pos, float4* nrm, unsigned long long* vis,
                        int* count, unsigned char* frame, hipStream_t s) {
  render_vertices<<<dim3((V + RENDER_BLOCK - 1) / RENDER_BLOCK, P), RENDER_BLOCK, 0, s>>>(verts, V, faces, csr_off, csr_face, xf,
                                                                                         params, H, W, pos, nrm);
  render_wire_raster<<<dim3((3 * F + RENDER_BLOCK - 1) / RENDER_BLOCK, P), RENDER_BLOCK, 0, s>>>(verts, pos, V, faces, F, xf, P, H, W,
                                                                                                vis, count);
  render_wire_shade<<<(H * W + RENDER_BLOCK - 1) / RENDER_BLOCK, RENDER_BLOCK, 0, s>>>(pos, nrm, V, faces, params, P, H, W, vis, frame);
}

void launch_render_ids(const unsigned long long* vis, int n, int* ids, hipStream_t s) {
  render_ids<<<(n + RENDER_BLOCK - 1) / RENDER_BLOCK, RENDER_BLOCK, 0, s>>>(vis, n, ids);
}

void launch_render_discs(unsigned char* frame, int H, int W, const float* points, const unsigned char* rgb, int N, int r,
                         const DiscRows& rows, hipStream_t s) {
  render_discs<<<(H * W + RENDER_BLOCK - 1) / RENDER_BLOCK, RENDER_BLOCK, 0, s>>>(frame, H, W, points, rgb, N, r, rows);
}
