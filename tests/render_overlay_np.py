"""float32 numpy restatement of the wireframe and keypoint-disc contracts (include/poco_hip.h "Wireframe" / "Keypoint discs",
DESIGN.md 16): the reference csrc/render.hip's render_wire_* and render_discs kernels are tested against.  Everything shared with
the filled path (projection, vertex normals, shading, the key layout) comes from tests/render_np.py; the expressions are those of
the kernels, in the same order, without fused multiply-adds.  No GPU."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from tests import render_np
from tests.render_np import EMPTY, f32

HEADER = Path(__file__).resolve().parent.parent / "include" / "poco_hip.h"
ID_MASK = np.uint64((1 << 22) - 1)
FRAGILE = 1e-3


# ---- the line rule ---------------------------------------------------------------------------------------------------------
def segment_fragments(pA, pB, H: int, W: int):
    """One edge walked from A to B, each (col, row, q_z) float32.  Returns None if it draws nothing, else a dict:
    pix [n] (row * W + col) and z, t [n] of its fragments; cols (major axis = columns); n_fragile = how many of the fragments sit
    within FRAGILE of a decision (minor coordinate near an integer, major bound near a pixel centre); fragile_pix = every pixel
    such a near-decision could add or remove."""
    ax, ay, az = (f32(v) for v in pA)
    bx, by, bz = (f32(v) for v in pB)
    if not np.isfinite([ax, ay, az, bx, by, bz]).all():
        return None
    cols = bool(abs(f32(bx - ax)) >= abs(f32(by - ay)))
    a0, a1, b0, b1 = (ax, bx, ay, by) if cols else (ay, by, ax, bx)
    if a0 == a1:
        return None
    nmaj, nmin = (W, H) if cols else (H, W)
    lo, hi = min(a0, a1), max(a0, a1)
    top = f32(nmaj + 1)
    i0 = max(0, int(np.ceil(f32(min(max(lo, f32(-1)), top)) - f32(0.5))))
    i1 = min(nmaj - 1, int(np.floor(f32(min(max(hi, f32(-1)), top)) - f32(0.5))))
    if i0 > i1:
        return None
    i = np.arange(i0, i1 + 1)
    c = i.astype(f32) + f32(0.5)
    on = (lo <= c) & (c < hi)
    t = ((c - a0) / f32(a1 - a0)).astype(f32)
    bf = (b0 + t * f32(b1 - b0)).astype(f32)
    b = np.floor(bf)
    z = (az + t * f32(bz - az)).astype(f32)
    ok = on & (b >= 0) & (b < nmin) & (np.abs(z) <= 1)
    near_bound = (np.abs(c - lo) < FRAGILE) | (np.abs(c - hi) < FRAGILE)
    near_int = np.abs(bf - np.rint(bf)) < FRAGILE

    def pix_of(ii, bb):
        bb = bb.astype(np.int64)
        m = (bb >= 0) & (bb < nmin)
        return (bb[m] * W + ii[m]) if cols else (ii[m] * W + bb[m])

    flagged = near_bound | near_int
    fragile_pix = np.concatenate([pix_of(i[flagged], np.clip(np.rint(bf[flagged]), -1, nmin)),
                                  pix_of(i[flagged], np.clip(np.rint(bf[flagged]) - 1, -1, nmin)),
                                  pix_of(i[flagged], np.clip(b[flagged], -1, nmin))])
    return {"pix": pix_of(i[ok], b[ok]), "z": z[ok], "t": t[ok], "cols": cols, "n_fragile": int((ok & flagged).sum()),
            "fragile_pix": fragile_pix}


def line_pixels(pA, pB, H: int, W: int):
    """The set of (col, row) the segment A -> B covers (q_z = 0)."""
    fr = segment_fragments((pA[0], pA[1], 0), (pB[0], pB[1], 0), H, W)
    return set() if fr is None else {(int(p % W), int(p // W)) for p in fr["pix"]}


def edge_ends(idx, e: int):
    """(A, B): the vertices of edge e (opposite vertex e) of triangle idx, lower index first; None for a repeated index."""
    u, w = int(idx[(e + 1) % 3]), int(idx[(e + 2) % 3])
    return None if u == w else (min(u, w), max(u, w))


def front_facing(verts: np.ndarray, faces: np.ndarray, rotation=None) -> np.ndarray:
    """bool [F]: ((q1 - q0) x (q2 - q0)).z > 0 in the transformed space, float32."""
    m = render_np.xform(rotation).reshape(-1)
    x, y, z = (verts[:, i].astype(f32) for i in range(3))
    qx, qy = render_np._mv(m[0:3], x, y, z), render_np._mv(m[3:6], x, y, z)
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    with np.errstate(invalid="ignore"):
        return ((qx[b] - qx[a]) * (qy[c] - qy[a]) - (qy[b] - qy[a]) * (qx[c] - qx[a])) > 0


def wire_np(frame: np.ndarray, verts: np.ndarray, faces: np.ndarray, cams, colors, materials, rotation=None, info: dict = None):
    """The wireframe call: frame uint8 [H,W,3] (not modified) -> uint8 [H,W,3].  `info` (a dict) receives vis (the keys [H,W]
    uint64), ids ([H,W] int32, triangle << 2 | edge or -1), fragments, fragile_fragments and fragile ([H,W] bool)."""
    H, W = frame.shape[:2]
    verts = np.asarray(verts, f32).reshape(-1, np.asarray(verts).shape[-2], 3)
    P = verts.shape[0]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    cams = np.asarray(cams, f32).reshape(P, 4)
    colors = np.asarray(colors, f32).reshape(P, 3)
    materials = np.broadcast_to(np.asarray(materials, f32).reshape(-1), (P,))
    vis = np.full(H * W, EMPTY, np.uint64)
    fragile = np.zeros(H * W, bool)
    nfrag = nfragile = 0
    proj = []
    for p in range(P):
        col, row, qz = render_np.project(verts[p], cams[p], H, W, rotation)
        proj.append((col, row, render_np.vertex_normals(verts[p], faces, rotation)))
        order = np.uint64(P - 1 - p) << np.uint64(54)
        for f in np.nonzero(front_facing(verts[p], faces, rotation))[0]:
            for e in range(3):
                ends = edge_ends(faces[f], e)
                if ends is None:
                    continue
                A, B = ends
                fr = segment_fragments((col[A], row[A], qz[A]), (col[B], row[B], qz[B]), H, W)
                if fr is None:
                    continue
                fragile[fr["fragile_pix"]] = True
                nfrag += len(fr["pix"])
                nfragile += fr["n_fragile"]
                if not len(fr["pix"]):
                    continue
                dbits = (f32(1) - fr["z"]).astype(f32).view(np.uint32).astype(np.uint64)
                np.minimum.at(vis, fr["pix"], order | (dbits << np.uint64(22)) | np.uint64(int(f) << 2 | e))
    out = frame.copy().reshape(-1, 3)
    hit = np.nonzero(vis != EMPTY)[0]
    pers = P - 1 - (vis[hit] >> np.uint64(54)).astype(np.int64)
    ident = (vis[hit] & ID_MASK).astype(np.int64)
    for p in np.unique(pers):
        col, row, nrm = proj[p]
        sel = pers == p
        pix_p, id_p = hit[sel], ident[sel]
        nzs = np.empty(len(pix_p), f32)
        for k_id in np.unique(id_p):
            k = id_p == k_id
            A, B = edge_ends(faces[k_id >> 2], int(k_id & 3))
            cols = bool(abs(f32(col[B] - col[A])) >= abs(f32(row[B] - row[A])))
            a0, a1 = (col[A], col[B]) if cols else (row[A], row[B])
            i = (pix_p[k] % W) if cols else (pix_p[k] // W)
            t = ((i.astype(f32) + f32(0.5) - a0) / f32(a1 - a0)).astype(f32)
            n = [(nrm[A, j] + t * f32(nrm[B, j] - nrm[A, j])).astype(f32) for j in range(3)]
            ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            nzs[k] = np.where(ln > 0, n[2] / np.where(ln > 0, ln, f32(1)), f32(0))
        out[pix_p] = render_np.shade(nzs, colors[p], materials[p])
    if info is not None:
        ids = np.full(H * W, -1, np.int32)
        ids[hit] = ident
        info.update(vis=vis.reshape(H, W), ids=ids.reshape(H, W), fragments=nfrag, fragile_fragments=nfragile,
                    fragile=fragile.reshape(H, W))
    return out.reshape(H, W, 3)


# ---- keypoint discs --------------------------------------------------------------------------------------------------------
def disc_table() -> np.ndarray:
    """POCO_DISC_HALF_WIDTHS of include/poco_hip.h: int [max radius + 1, max radius + 1], row r holds the half-widths of
    |dy| = 0 .. r.  The one table: the library compiles the same macro."""
    txt = HEADER.read_text()
    body = re.search(r"#define POCO_DISC_HALF_WIDTHS \{(.*?)\} \}", txt, re.S).group(1) + "}"
    rows = [[int(v) for v in r.split(",")] for r in re.findall(r"\{([^{}]*)\}", body)]
    n = int(re.search(r"#define POCO_DISC_MAX_RADIUS (\d+)", txt).group(1))
    tab = np.array(rows, np.int64)
    assert tab.shape == (n + 1, n + 1)
    return tab


def midpoint_circle(r: int):
    """Half-widths of |dy| = 0 .. r by the midpoint circle: x = 0, y = r, d = 1 - r; every visited (x, y) gives row y the
    half-width x and row x the half-width y, the larger one stays."""
    hw = [-1] * (r + 1)

    def plot(x, y):
        hw[y] = max(hw[y], x)
        hw[x] = max(hw[x], y)
    x, y, d = 0, r, 1 - r
    plot(x, y)
    while x < y:
        if d < 0:
            d += 2 * x + 3
        else:
            d += 2 * (x - y) + 5
            y -= 1
        x += 1
        plot(x, y)
    return hw


def stamp_rows(r: int):
    """[(dy, half-width)] of the 2r + 1 rows of the stamp of radius r."""
    tab = disc_table()
    if not 0 <= r < tab.shape[0]:
        raise ValueError(f"radius {r} beyond the table")
    return [(dy, int(tab[r, abs(dy)])) for dy in range(-r, r + 1)]


def draw_discs_np(frame: np.ndarray, points, rgb, r: int = 4) -> np.ndarray:
    """frame uint8 [H,W,3] (not modified); points [N,2] (col, row) float32; rgb [N,3] uint8.  Painted in index order."""
    out = frame.copy()
    H, W = out.shape[:2]
    pts = np.asarray(points, f32).reshape(-1, 2)
    rgb = np.broadcast_to(np.asarray(rgb, np.uint8).reshape(-1, 3), (len(pts), 3))
    rows = stamp_rows(r)
    for (x, y), c in zip(pts, rgb):
        if not (abs(x) < 2.0 ** 30 and abs(y) < 2.0 ** 30):               # not finite, or out of range: paints nothing
            continue
        cx, cy = int(x), int(y)                                           # toward zero, as the reference's int(pt[0])
        for dy, hw in rows:
            rr = cy + dy
            if 0 <= rr < H:
                out[rr, max(0, cx - hw):max(0, min(W, cx + hw + 1))] = c
    return out


# ---- test scenes -----------------------------------------------------------------------------------------------------------
def pixel_camera(H: int, W: int):
    """sx = 2/W, sy = 2/H: col = W/2 + q_x, row = H/2 - q_y, exactly (for the small integers of the scenes below)."""
    return [2.0 / W, 2.0 / H, 0.0, 0.0]


def from_q(q) -> np.ndarray:
    """Model-space vertices whose transformed position (identity rotation) is q: v = Rx(180 deg) q = (q_x, -q_y, -q_z)."""
    return (np.asarray(q, np.float64) * np.array([1.0, -1.0, -1.0])).astype(np.float32)


def outward(q, faces) -> np.ndarray:
    """faces [F,3] of a convex solid with vertices q, each wound counter-clockwise seen from outside."""
    q = np.asarray(q, np.float64)
    out = []
    for a, b, c in faces:
        n = np.cross(q[b] - q[a], q[c] - q[a])
        out.append((a, b, c) if n @ (q[a] - q.mean(0)) > 0 else (a, c, b))
    return np.array(out, np.int32)


def int_tetrahedron(H: int = 32, W: int = 32):
    """A closed tetrahedron on integer pixel coordinates, seen face-on: the near edge 0-1 is horizontal through the centre, the
    far edge 2-3 vertical behind it.  Faces (0,1,2) and (0,1,3) face the camera, the two that share edge 2-3 face away.
    Returns (verts [4,3], faces [4,3], cam, the screen position (col, row) of each vertex)."""
    q = np.array([[-8, 0, 0.5], [8, 0, 0.5], [0, 8, -0.5], [0, -8, -0.5]], np.float64)
    faces = outward(q, [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)])
    screen = [(W // 2 + int(x), H // 2 - int(y)) for x, y, _ in q]
    return from_q(q), faces, pixel_camera(H, W), screen


def int_quads(H: int = 32, W: int = 32, back: bool = False):
    """Two quads of ONE mesh at different depths on integer pixel coordinates, both facing the camera (or both away with
    `back`): the near one (q_z = 0.5, vertices 0-3, flat: normal +z) and the far one (vertices 4-7, q_z from -0.2 at its left
    edge to -0.8 at its right one: tilted, so it shades darker), shifted so that the near quad's right edge (col W/2 + 4) crosses
    the far quad's top edge (row H/2 - 6) at pixel (W/2 + 4, H/2 - 6).  q_x, q_y are sixteenths (exact) under the camera
    (32/W, 32/H): col = W/2 + 16 q_x, row = H/2 - 16 q_y.
    Returns (verts [8,3], faces [4,3], cam, (col, row) of the crossing)."""
    near = [[-6, -4, 0.5], [4, -4, 0.5], [4, 9, 0.5], [-6, 9, 0.5]]
    far = [[-2, -9, -0.2], [10, -9, -0.8], [10, 6, -0.8], [-2, 6, -0.2]]
    q = np.array(near + far, np.float64) / np.array([16.0, 16.0, 1.0])
    faces = np.array([(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)], np.int32)          # counter-clockwise with q_y up
    if back:
        faces = faces[:, ::-1].copy()
    return from_q(q), faces, [32.0 / W, 32.0 / H, 0.0, 0.0], (W // 2 + 4, H // 2 - 6)


def tilted_quad():
    """A two-triangle quad tilted so that both the main view and the Ry(270 deg) side view see its front."""
    q = np.array([[-0.52, -0.41, 0.31], [0.47, -0.36, -0.28], [0.55, 0.43, -0.33], [-0.49, 0.38, 0.36]], np.float64)
    return from_q(q), np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def tetrahedron():
    """A closed tetrahedron on coordinates that are nothing special."""
    q = np.array([[-0.51, -0.33, 0.12], [0.57, -0.29, 0.21], [0.03, 0.61, 0.05], [0.07, -0.04, -0.58]], np.float64)
    return from_q(q), outward(q, [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)])
