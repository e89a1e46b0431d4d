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
#include "common.h"
#include "kernels.h"

// The numpy restatement evaluates the same expressions in float32 without fused multiply-adds; keep hipcc from contracting
// them, so coverage decisions and depths agree bit for bit.
#pragma clang fp contract(off)

namespace {

constexpr int RENDER_BLOCK = 256;
constexpr float RENDER_PI = 3.14159265358979323846f;

// Setup of one triangle in screen space, shared by the raster and shade kernels so both take identical decisions.
// Edge i is the edge opposite vertex i.  Each edge function is evaluated in a canonical orientation (from the endpoint with the
// lower vertex index to the higher one) and then negated as needed, so the two triangles that share an edge see exactly
// opposite values: a centre on the edge is inside one of them or the other, never both or neither.
struct TriSetup {
  float ax[3], ay[3], dx[3], dy[3];   // canonical start point and direction of each edge
  float sgn[3];                       // +1 / -1: canonical value -> inward value (positive inside)
  bool tie_in[3];                     // a centre exactly on the edge (inward value 0) belongs to this triangle
  float area;                         // twice the (positive) area
};

__device__ __forceinline__ float edge_canon(const TriSetup& t, int e, float px, float py) {
  return t.dx[e] * (py - t.ay[e]) - t.dy[e] * (px - t.ax[e]);
}

// false = degenerate (zero area or a repeated vertex index): the triangle covers nothing
__device__ __forceinline__ bool tri_setup(const float4* pos, const int* idx, TriSetup& t) {
  #pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int u = idx[(e + 1) % 3], w = idx[(e + 2) % 3];
    if (u == w) return false;
    const float4 A = pos[u < w ? u : w], B = pos[u < w ? w : u];
    t.ax[e] = A.x; t.ay[e] = A.y;
    t.dx[e] = B.x - A.x; t.dy[e] = B.y - A.y;
    t.sgn[e] = u < w ? 1.f : -1.f;
  }
  // twice the signed area: the winding-order value of edge 2 (vertex 0 -> 1) at vertex 2
  const float4 C = pos[idx[2]];
  const float a2 = t.sgn[2] * edge_canon(t, 2, C.x, C.y);
  if (!(a2 != 0.f)) return false;
  const float o = a2 > 0.f ? 1.f : -1.f;
  t.area = a2 * o;
  #pragma unroll
  for (int e = 0; e < 3; ++e) {
    t.sgn[e] *= o;
    // the inward value grows along sgn * (-dy, dx): decide a zero as if the centre were nudged by (+eps, +eps^2)
    t.tie_in[e] = t.dy[e] != 0.f ? (t.sgn[e] * -t.dy[e] > 0.f) : (t.sgn[e] * t.dx[e] > 0.f);
  }
  return true;
}

// inward values of the three edges at (px, py); true = the centre is covered
__device__ __forceinline__ bool tri_cover(const TriSetup& t, float px, float py, float* w) {
  bool in = true;
  #pragma unroll
  for (int e = 0; e < 3; ++e) {
    w[e] = t.sgn[e] * edge_canon(t, e, px, py);
    in = in && (w[e] > 0.f || (w[e] == 0.f && t.tie_in[e]));
  }
  return in;
}

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
  // pyrender's metallic-roughness shading with l = v = h = +z (three directional lights along -z, ambient 0.3)
  const float cth = fminf(fmaxf(nz, 0.f), 1.f);
  const float* pr = params + (size_t)p * RENDER_PARAMS;
  const bool plain = pr[7] != 0.f;
  const float metal = plain ? 0.f : 0.2f, rough = plain ? 1.f : 0.8f;
  const float alpha = rough * rough, a2 = alpha * alpha;
  const float D = a2 / (RENDER_PI * sq(cth * cth * (a2 - 1.f) + 1.f));
  const float G = sq(2.f * cth / (cth + sqrtf(a2 + (1.f - a2) * cth * cth)));
  unsigned char* out = frame + (size_t)i * 3;
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

}  // namespace

void launch_render(const float* verts, int P, int V, const int* faces, int F, const int* csr_off, const int* csr_face,
                   const RenderXform& xf, const float* params, int H, int W, float4* pos, float4* nrm, unsigned long long* vis,
                   int* count, unsigned char* frame, hipStream_t s) {
  render_vertices<<<dim3((V + RENDER_BLOCK - 1) / RENDER_BLOCK, P), RENDER_BLOCK, 0, s>>>(verts, V, faces, csr_off, csr_face, xf,
                                                                                         params, H, W, pos, nrm);
  render_raster<<<dim3((F + RENDER_BLOCK - 1) / RENDER_BLOCK, P), RENDER_BLOCK, 0, s>>>(pos, V, faces, F, P, H, W, vis, count);
  render_shade<<<(H * W + RENDER_BLOCK - 1) / RENDER_BLOCK, RENDER_BLOCK, 0, s>>>(pos, nrm, V, faces, params, P, H, W, vis, frame);
}
