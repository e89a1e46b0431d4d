"""numpy restatement of the visibility contract (include/poco_hip.h poco_op_part_visibility): the reference the
device code (csrc/part_visibility.hip, poco_amd/visibility.py) is tested against.  The rasteriser is tests/segm_np.py's - its
projection and tests/render_np.py's coverage rule, imported - in float32 in the device's expression order, walked over the window
instead of the frame; everything it gives is an integer and is compared for equality.  The statistics are restated in float64 with
numpy's own correlation and a ranking written differently from the product's."""
from __future__ import annotations

import numpy as np

from tests import render_np, segm_np

f32 = np.float32
EMPTY = segm_np.EMPTY
NEAR = segm_np.NEAR
PARTS = 24


# ---- operator ------------------------------------------------------------------------------------------------------------------------
def window_raster(verts, cam_t, faces, face_part, focal, res, margin):
    """One crop: (bits uint32 [W,W] with W = res + 2 margin: bit p set where a fragment of part p covers the window pixel,
    keys uint64 [res,res]: segm_np.part_keys' depth keys of the frame)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fp = np.minimum(np.asarray(face_part, np.int64).reshape(-1), PARTS - 1)
    x, y, z = segm_np.project(verts, cam_t, focal, res)
    W = res + 2 * margin
    bits = np.zeros(W * W, np.uint32)
    keys = np.full(res * res, EMPTY, np.uint64)
    V = x.shape[0]
    lo, hi = f32(-margin - 1), f32(res + margin + 1)
    for f, idx in enumerate(faces):
        if idx.min() < 0 or idx.max() >= V:
            continue
        xs, ys, zs = x[idx], y[idx], z[idx]
        if not (zs >= NEAR).all():
            continue
        if not (np.isfinite(xs).all() and np.isfinite(ys).all() and np.isfinite(zs).all()):
            continue
        t = render_np.tri_setup(idx, x, y)
        if t is None:
            continue
        minx, maxx = max(xs.min(), lo), min(xs.max(), hi)
        miny, maxy = max(ys.min(), lo), min(ys.max(), hi)
        c0, c1 = max(-margin, int(np.ceil(minx - f32(0.5)))), min(res + margin - 1, int(np.floor(maxx - f32(0.5))))
        r0, r1 = max(-margin, int(np.ceil(miny - f32(0.5)))), min(res + margin - 1, int(np.floor(maxy - f32(0.5))))
        if c0 > c1 or r0 > r1:
            continue
        cc, rr = np.meshgrid(np.arange(c0, c1 + 1), np.arange(r0, r1 + 1))
        px, py = cc.astype(f32) + f32(0.5), rr.astype(f32) + f32(0.5)
        w, inside = render_np.tri_cover(t, px, py)
        ia, ib, ic = f32(1) / zs[0], f32(1) / zs[1], f32(1) / zs[2]
        with np.errstate(all="ignore"):
            iz = ((w[0] * ia + w[1] * ib) + w[2] * ic) / t[6]
            zz = (f32(1) / iz).astype(f32)
        keep = inside & (zz > 0) & np.isfinite(zz)
        if not keep.any():
            continue
        r, c = rr[keep], cc[keep]
        np.bitwise_or.at(bits, (r + margin) * W + (c + margin), np.uint32(1 << int(fp[f])))
        fr = (r >= 0) & (r < res) & (c >= 0) & (c < res)
        if fr.any():
            key = (zz[keep][fr].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            np.minimum.at(keys, r[fr] * res + c[fr], key)
    return bits.reshape(W, W), keys.reshape(res, res)


def part_visibility(verts, cam_t, faces, face_part, focal=5000.0, res=224, margin=112, occ_mask=None):
    """verts [B,V,3], cam_t [B,3], faces [F,3], face_part [F], occ_mask uint8 [B,res,res] or None -> int32 [B,24,4] = (total, area,
    front, seen) per crop and part."""
    verts = np.asarray(verts, f32)
    fp = np.minimum(np.asarray(face_part, np.int64).reshape(-1), PARTS - 1)
    B = verts.shape[0]
    out = np.zeros((B, PARTS, 4), np.int32)
    for b in range(B):
        bits, keys = window_raster(verts[b], np.asarray(cam_t)[b], faces, fp, focal, res, margin)
        frame = bits[margin:margin + res, margin:margin + res]
        hit = keys != EMPTY
        winner = np.full((res, res), -1, np.int64)
        winner[hit] = fp[(keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
        free = np.ones((res, res), bool) if occ_mask is None else np.asarray(occ_mask)[b] == 0
        for p in range(PARTS):
            out[b, p] = (np.count_nonzero((bits >> np.uint32(p)) & np.uint32(1)), np.count_nonzero((frame >> np.uint32(p)) & np.uint32(1)),
                         np.count_nonzero(winner == p), np.count_nonzero((winner == p) & free))
    return out


# ---- statistics ----------------------------------------------------------------------------------------------------------------------
def ratios(counts):
    c = np.asarray(counts, np.float64)
    with np.errstate(all="ignore"):
        total, area, front, seen = (c[..., k] for k in range(4))
        return {"vis": np.where(total > 0, seen / total, np.nan), "vis_frame": np.where(total > 0, area / total, np.nan),
                "vis_self": np.where(area > 0, front / area, np.nan), "vis_obj": np.where(front > 0, seen / front, np.nan)}


def _ranks(x):
    """Average ranks by counting: rank = (values below) + (values equal + 1) / 2."""
    x = np.asarray(x, np.float64)
    return np.array([(x < v).sum() + ((x == v).sum() + 1) / 2.0 for v in x])


def corr(x, y, rank=False):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if rank:
        x, y = _ranks(x), _ranks(y)
    if x.size < 2 or x.std() == 0 or y.std() == 0:
        return float("nan")
    return float(np.corrcoef(x, y)[0, 1])


def statistics(counts, uncert, err, bins=5):
    """The numbers poco_amd.visibility.statistics gives, restated: dict with mean [24], mean_all, corr {component: (r, rho)},
    corr_joint [24,2], corr_err (r, rho), bins [K,3], valid, invalid."""
    r = ratios(counts)
    n = r["vis"].shape[0]
    u, e = np.asarray(uncert, np.float64).reshape(n, PARTS), np.asarray(err, np.float64).reshape(n, PARTS)
    ok = ~np.isnan(r["vis"])
    out = {"valid": int(ok.sum()), "invalid": int(ok.size - ok.sum()), "mean": np.full(PARTS, np.nan), "corr_joint": np.full((PARTS, 2), np.nan)}
    for j in range(PARTS):
        m = ok[:, j]
        if m.any():
            out["mean"][j] = np.mean(r["vis"][m, j])
            out["corr_joint"][j] = corr(1 - r["vis"][m, j], u[m, j]), corr(1 - r["vis"][m, j], u[m, j], True)
    out["mean_all"] = float(np.mean(r["vis"][ok])) if ok.any() else float("nan")
    out["corr"] = {}
    for k, v in r.items():
        m = ~np.isnan(v)
        out["corr"][k] = (corr(1 - v[m], u[m]), corr(1 - v[m], u[m], True))
    out["corr_err"] = (corr(1 - r["vis"][ok], e[ok]), corr(1 - r["vis"][ok], e[ok], True))
    table = np.full((bins, 3), np.nan)
    v, uu, ee = r["vis"][ok], u[ok], e[ok]
    for k in range(bins):
        m = (v >= k / bins) & ((v < (k + 1) / bins) | (k == bins - 1))
        table[k, 0] = m.sum()
        if m.any():
            table[k, 1:] = uu[m].mean(), ee[m].mean()
    out["bins"] = table
    return out


# ---- hand-made meshes ----------------------------------------------------------------------------------------------------------------
class Mesh:
    """Triangles built in SCREEN space and unprojected exactly, as segm_np.hand_mesh does: coordinates are multiples of 1/8 of a pixel
    and z / focal is a power of two, so the projection gives the coordinates back bit for bit (checked by exact())."""

    def __init__(self, res, focal=4096.0, z=64.0):
        self.res, self.focal, self.z = res, focal, z
        self.pts, self.faces, self.parts, self.screen = [], [], [], []

    def vert(self, px, py, zz=None):
        zz = self.z if zz is None else zz
        self.pts.append(((px - self.res / 2.0) * zz / self.focal, (py - self.res / 2.0) * zz / self.focal, zz))
        self.screen.append((px, py))
        return len(self.pts) - 1

    def tri(self, a, b, c, part):
        """a, b, c: vertex indices or (px, py[, z]) tuples."""
        idx = [v if isinstance(v, (int, np.integer)) else self.vert(*v) for v in (a, b, c)]
        self.faces.append(idx)
        self.parts.append(part)
        return len(self.faces) - 1

    def arrays(self):
        return np.array(self.pts, f32), np.array(self.faces, np.int32).reshape(-1, 3), np.array(self.parts, np.uint8)

    def exact(self):
        v, _, _ = self.arrays()
        x, y, _ = segm_np.project(v, np.zeros(3, f32), self.focal, self.res)
        s = np.array(self.screen, f32)
        fin = np.isfinite(s).all(1) & (v[:, 2] >= 0.1)
        return np.array_equal(x[fin], s[fin, 0]) and np.array_equal(y[fin], s[fin, 1])


def sphere(levels=3, parts=PARTS, radius=0.6):
    """An icosphere: 10 * 4^levels + 2 vertices (642 at level 3), 20 * 4^levels faces; the part of a face is the longitude band of
    its centroid, so all `parts` parts are present and every part has a front and a back side.  (verts float32 [V,3] around the
    origin, faces int32 [F,3], face_part uint8 [F])."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.array(v) * radius
    faces = np.array(f, np.int32)
    cen = verts[faces].mean(1)
    lon = (np.arctan2(cen[:, 2], cen[:, 0]) + np.pi) / (2 * np.pi)
    return verts.astype(f32), faces, np.minimum((lon * parts).astype(np.int64), parts - 1).astype(np.uint8)
