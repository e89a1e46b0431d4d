"""float32 numpy restatement of the renderer contract (include/poco_hip.h "demo renderer", DESIGN.md "Renderer"): the reference the
GPU renderer (csrc/render.hip) is tested against.  Per person, per triangle, vectorised over the triangle's pixel bounding box;
the same expressions in the same order as the kernels, without fused multiply-adds."""
from __future__ import annotations

import numpy as np

f32 = np.float32
PI = f32(3.14159265358979323846)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def xform(rotation=None) -> np.ndarray:
    """R * Rx(180 deg) as float32 [3,3]: Rx(180 deg) = diag(1, -1, -1) negates the 2nd and 3rd columns of R."""
    R = np.eye(3, dtype=f32) if rotation is None else np.asarray(rotation, f32).reshape(3, 3)
    return (R * np.array([1, -1, -1], f32)).astype(f32)


def _mv(m, x, y, z):
    return (m[0] * x + m[1] * y) + m[2] * z


def project(verts: np.ndarray, cam, H: int, W: int, rotation=None):
    """verts [V,3] -> (col, row, q_z) float32 [V] each."""
    m = xform(rotation).reshape(-1)
    x, y, z = (verts[:, i].astype(f32) for i in range(3))
    qx, qy, qz = _mv(m[0:3], x, y, z), _mv(m[3:6], x, y, z), _mv(m[6:9], x, y, z)
    sx, sy, tx, ty = (f32(c) for c in np.asarray(cam, f32)[:4])
    col = f32(W * 0.5) * (f32(1) + sx * (qx + tx))
    row = f32(H * 0.5) * (f32(1) - sy * (qy - ty))
    return col.astype(f32), row.astype(f32), qz.astype(f32)


def vertex_normals(verts: np.ndarray, faces: np.ndarray, rotation=None) -> np.ndarray:
    """Area-weighted vertex normals (sum of the incident faces' cross products in face order), normalised, then rotated by
    R * Rx: float32 [V,3]."""
    v = verts.astype(f32)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    u, w = b - a, c - a
    fn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                   u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1).astype(f32)
    n = np.zeros_like(v)
    np.add.at(n, faces.reshape(-1), np.repeat(fn, 3, axis=0))       # sequential: face order per vertex, as the CSR gather
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(f32)
    nz = ln > 0
    n[nz] = n[nz] / ln[nz, None]
    m = xform(rotation).reshape(-1)
    return np.stack([_mv(m[0:3], n[:, 0], n[:, 1], n[:, 2]), _mv(m[3:6], n[:, 0], n[:, 1], n[:, 2]),
                     _mv(m[6:9], n[:, 0], n[:, 1], n[:, 2])], 1).astype(f32)


def tri_setup(idx, col, row):
    """(ax, ay, dx, dy, sgn, tie_in, area) of one triangle, or None if it covers nothing (kernel TriSetup)."""
    ax, ay, dx, dy, sg = [], [], [], [], []
    for e in range(3):
        u, w = int(idx[(e + 1) % 3]), int(idx[(e + 2) % 3])
        if u == w:
            return None
        A, B = (u, w) if u < w else (w, u)
        ax.append(col[A]); ay.append(row[A])
        dx.append(f32(col[B] - col[A])); dy.append(f32(row[B] - row[A]))
        sg.append(f32(1) if u < w else f32(-1))
    c2 = int(idx[2])
    a2 = sg[2] * (dx[2] * (row[c2] - ay[2]) - dy[2] * (col[c2] - ax[2]))
    if not a2 != 0:
        return None
    o = f32(1) if a2 > 0 else f32(-1)
    sg = [s * o for s in sg]
    tie = [(s * -ddy > 0) if ddy != 0 else (s * ddx > 0) for s, ddx, ddy in zip(sg, dx, dy)]
    return ax, ay, dx, dy, sg, tie, f32(a2 * o)


def tri_cover(t, px, py):
    """inward edge values [3, ...] and the coverage mask at centres (px, py)."""
    ax, ay, dx, dy, sg, tie, _ = t
    w = [sg[e] * (dx[e] * (py - ay[e]) - dy[e] * (px - ax[e])) for e in range(3)]
    inside = np.ones(np.broadcast(px, py).shape, bool)
    for e in range(3):
        inside &= (w[e] > 0) | ((w[e] == 0) & tie[e])
    return w, inside


def shade(nz, base, material):
    """uint8 colour [..., 3] of pixels with normal z component nz (float32 [...]) and base colour base [3]."""
    plain = material != 0
    metal, rough = (f32(0), f32(1)) if plain else (f32(0.2), f32(0.8))
    alpha = rough * rough
    a2 = alpha * alpha
    c = np.clip(nz, f32(0), f32(1)).astype(f32)
    D = a2 / (PI * (c * c * (a2 - f32(1)) + f32(1)) ** 2)
    G = (f32(2) * c / (c + np.sqrt(a2 + (f32(1) - a2) * c * c))) ** 2
    out = []
    for ch in range(3):
        b = f32(base[ch])
        F0 = f32(0.04) * (f32(1) - metal) + b * metal
        cdiff = b * f32(0.96) * (f32(1) - metal)
        per = c * ((f32(1) - F0) * cdiff / PI + F0 * G * D / (f32(4) * c * c + f32(0.001)))
        colour = f32(3) * per + f32(0.3) * b
        g = np.clip(np.power(colour.astype(f32), f32(1) / f32(2.2)), f32(0), f32(1))
        out.append(np.rint(f32(255) * g).astype(np.uint8))
    return np.stack(out, -1)


def render_np(frame: np.ndarray, verts: np.ndarray, faces: np.ndarray, cams, colors, materials, rotation=None,
              return_vis: bool = False):
    """frame uint8 [H,W,3] (not modified), verts [P,V,3], faces [F,3], cams [P,4], colors [P,3], materials [P] ->
    uint8 [H,W,3] (and the visibility keys [H,W] uint64 with return_vis)."""
    H, W = frame.shape[:2]
    verts = np.asarray(verts, f32).reshape(-1, np.asarray(verts).shape[-2], 3)
    P = verts.shape[0]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cams = np.asarray(cams, f32).reshape(P, 4)
    colors = np.asarray(colors, f32).reshape(P, 3)
    materials = np.broadcast_to(np.asarray(materials, f32).reshape(-1), (P,))
    vis = np.full(H * W, EMPTY, np.uint64)
    proj = []
    for p in range(P):
        col, row, qz = project(verts[p], cams[p], H, W, rotation)
        proj.append((col, row, qz, vertex_normals(verts[p], faces, rotation)))
        order = np.uint64(P - 1 - p) << np.uint64(54)
        for f, idx in enumerate(faces):
            xs, ys, zs = col[idx], row[idx], qz[idx]
            if not (np.isfinite(xs).all() and np.isfinite(ys).all() and np.isfinite(zs).all()):
                continue
            t = tri_setup(idx, col, row)
            if t is None:
                continue
            minx, maxx = max(xs.min(), f32(-1)), min(xs.max(), f32(W + 1))
            miny, maxy = max(ys.min(), f32(-1)), min(ys.max(), f32(H + 1))
            c0, c1 = max(0, int(np.ceil(minx - f32(0.5)))), min(W - 1, int(np.floor(maxx - f32(0.5))))
            r0, r1 = max(0, int(np.ceil(miny - f32(0.5)))), min(H - 1, int(np.floor(maxy - f32(0.5))))
            if c0 > c1 or r0 > r1:
                continue
            cc, rr = np.meshgrid(np.arange(c0, c1 + 1), np.arange(r0, r1 + 1))
            px, py = cc.astype(f32) + f32(0.5), rr.astype(f32) + f32(0.5)
            w, inside = tri_cover(t, px, py)
            z = ((w[0] * zs[0] + w[1] * zs[1]) + w[2] * zs[2]) / t[6]
            keep = inside & (np.abs(z) <= 1)
            if not keep.any():
                continue
            dbits = (f32(1) - z[keep].astype(f32)).astype(f32).view(np.uint32).astype(np.uint64)
            key = order | (dbits << np.uint64(22)) | np.uint64(f)
            np.minimum.at(vis, (rr[keep] * W + cc[keep]).reshape(-1), key)
    out = frame.copy().reshape(-1, 3)
    hit = np.nonzero(vis != EMPTY)[0]
    keys = vis[hit]
    pers = (P - 1 - (keys >> np.uint64(54)).astype(np.int64))
    tri = (keys & np.uint64((1 << 22) - 1)).astype(np.int64)
    for p in np.unique(pers):
        col, row, _, nrm = proj[p]
        sel = pers == p
        pix_p, tri_p = hit[sel], tri[sel]
        nzs = np.empty(len(pix_p), f32)
        for f in np.unique(tri_p):
            k = tri_p == f
            idx = faces[f]
            t = tri_setup(idx, col, row)
            px, py = (pix_p[k] % W).astype(f32) + f32(0.5), (pix_p[k] // W).astype(f32) + f32(0.5)
            w, _ = tri_cover(t, px, py)
            n = [(w[0] * nrm[idx[0], j] + w[1] * nrm[idx[1], j]) + w[2] * nrm[idx[2], j] for j in range(3)]
            ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            nzs[k] = np.where(ln > 0, n[2] / np.where(ln > 0, ln, f32(1)), f32(0))
        out[pix_p] = shade(nzs, colors[p], materials[p])
    out = out.reshape(H, W, 3)
    return (out, vis.reshape(H, W)) if return_vis else out


# ---- procedural test meshes --------------------------------------------------------------------------------------------
def icosphere(subdiv: int = 2):
    """(verts [V,3] float32 on the unit sphere, faces [F,3] int32, outward counter-clockwise)."""
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                cache[k] = len(verts) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(verts, np.float32), np.array(f, np.int32)


def deformed_sphere(seed: int, subdiv: int = 2, center=(0.0, 0.0, 0.0), radius: float = 0.5):
    """A closed, smoothly deformed icosphere (the same faces for every seed)."""
    v, f = icosphere(subdiv)
    r = np.random.default_rng(seed)
    k = r.normal(size=(3, 3))
    bump = 1.0 + 0.25 * np.sin(v @ k[0] * 2.0 + k[1, 0]) * np.cos(v @ k[2] * 1.5)
    return (v * (radius * bump)[:, None] + np.asarray(center, np.float32)).astype(np.float32), f
