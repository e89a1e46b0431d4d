// The watertight triangle coverage rule shared by the demo renderer (render.hip) and the part-label rasteriser (part_labels.hip):
// both include this file, so a pixel centre on a shared edge or vertex is decided by the very same expressions in both.
// tests/render_np.py (tri_setup / tri_cover) restates it in float32 numpy.
#pragma once
#include <hip/hip_runtime.h>

// The numpy restatements evaluate the same expressions in float32 without fused multiply-adds; keep hipcc from contracting them,
// here and in the files that include this header, so coverage decisions and depths agree bit for bit.
#pragma clang fp contract(off)

namespace {

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

// corner[k] = screen position (x, y) of the triangle's k-th vertex, idx[k] = its vertex index (orders the endpoints of an edge).
// false = degenerate (zero area or a repeated vertex index): the triangle covers nothing
__device__ __forceinline__ bool tri_setup_corners(const float4* corner, const int* idx, TriSetup& t) {
  #pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int ku = (e + 1) % 3, kw = (e + 2) % 3;
    const int u = idx[ku], w = idx[kw];
    if (u == w) return false;
    const float4 A = corner[u < w ? ku : kw], B = corner[u < w ? kw : ku];
    t.ax[e] = A.x; t.ay[e] = A.y;
    t.dx[e] = B.x - A.x; t.dy[e] = B.y - A.y;
    t.sgn[e] = u < w ? 1.f : -1.f;
  }
  // twice the signed area: the winding-order value of edge 2 (vertex 0 -> 1) at vertex 2
  const float4 C = corner[2];
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

// the same with the positions in a per-vertex array: pos[idx[k]] is the k-th corner
__device__ __forceinline__ bool tri_setup(const float4* pos, const int* idx, TriSetup& t) {
  const float4 corner[3] = {pos[idx[0]], pos[idx[1]], pos[idx[2]]};
  return tri_setup_corners(corner, idx, t);
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

}  // namespace
