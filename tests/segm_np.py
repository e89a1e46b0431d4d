"""numpy restatement of the body-part segmentation contract (include/poco_hip.h "body-part segmentation"): the
reference the device code (csrc/part_labels.hip, csrc/segm_metrics.hip, poco_amd/segm.py) is tested against.  float32 in the
device's expression order where the tests ask for equal bits (labels, counts, argmax), float64 as the yardstick of every tolerance
(cross-entropy, translation)."""
from __future__ import annotations

import numpy as np

from tests import render_np

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NEAR = f32(0.1)


# ---- rasteriser --------------------------------------------------------------------------------------------------------------------
def project(verts, cam_t, focal, res):
    """verts [V,3], cam_t [3] -> (x, y, Z) float32 [V]: x = focal X / Z + res / 2, y = focal Y / Z + res / 2, (X, Y, Z) = v + cam_t."""
    v = np.asarray(verts, f32)
    t = np.asarray(cam_t, f32)
    X, Y, Z = v[:, 0] + t[0], v[:, 1] + t[1], v[:, 2] + t[2]
    half = f32(res) * f32(0.5)
    with np.errstate(all="ignore"):
        return (f32(focal) * X / Z + half).astype(f32), (f32(focal) * Y / Z + half).astype(f32), Z.astype(f32)


def part_keys(verts, cam_t, faces, focal, res):
    """The visibility keys uint64 [res,res] of one crop: float bits of z << 32 | face, the minimum per pixel."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    x, y, z = project(verts, cam_t, focal, res)
    keys = np.full(res * res, EMPTY, np.uint64)
    V = x.shape[0]
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
        lim = f32(res + 1)
        minx, maxx = max(xs.min(), f32(-1)), min(xs.max(), lim)
        miny, maxy = max(ys.min(), f32(-1)), min(ys.max(), lim)
        c0, c1 = max(0, int(np.ceil(minx - f32(0.5)))), min(res - 1, int(np.floor(maxx - f32(0.5))))
        r0, r1 = max(0, int(np.ceil(miny - f32(0.5)))), min(res - 1, int(np.floor(maxy - f32(0.5))))
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
        key = (zz[keep].view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        np.minimum.at(keys, (rr[keep] * res + cc[keep]).reshape(-1), key)
    return keys.reshape(res, res)


def part_labels(verts, cam_t, faces, face_part, focal=5000.0, res=224):
    """verts [B,V,3], cam_t [B,3], faces [F,3], face_part [F] -> uint8 [B,res,res]: face_part[winner] + 1, 0 where nothing is drawn."""
    verts = np.asarray(verts, f32)
    fp = np.asarray(face_part, np.uint8)
    out = np.zeros((verts.shape[0], res, res), np.uint8)
    for b in range(verts.shape[0]):
        k = part_keys(verts[b], np.asarray(cam_t)[b], faces, focal, res)
        hit = k != EMPTY
        out[b][hit] = fp[(k[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)] + 1
    return out


# ---- camera ------------------------------------------------------------------------------------------------------------------------
def estimate_translation(S, joints2d, focal=5000.0, res=224):
    """geometry.py:511-551 per crop in float64: S [B,J,3], joints2d [B,J,3] (x, y, confidence) -> [B,3]; the weight sqrt(confidence)
    is taken in float32 as the reference takes it; a singular system gives (1, 1, 1)."""
    S = np.asarray(S, f32)
    k = np.asarray(joints2d, f32)
    out = np.zeros((S.shape[0], 3), np.float64)
    F, ctr = float(focal), res / 2.0
    for b in range(S.shape[0]):
        w = np.sqrt(k[b, :, 2]).astype(np.float64)
        X, Y, Z = (S[b, :, i].astype(np.float64) for i in range(3))
        x, y = k[b, :, 0].astype(np.float64), k[b, :, 1].astype(np.float64)
        J = len(w)
        Q = np.zeros((2 * J, 3))
        Q[0::2, 0] = w * F
        Q[0::2, 2] = w * (ctr - x)
        Q[1::2, 1] = w * F
        Q[1::2, 2] = w * (ctr - y)
        c = np.zeros(2 * J)
        c[0::2] = w * ((x - ctr) * Z - F * X)
        c[1::2] = w * ((y - ctr) * Z - F * Y)
        A, rhs = Q.T @ Q, Q.T @ c
        try:
            out[b] = np.linalg.solve(A, rhs)
        except np.linalg.LinAlgError:
            out[b] = 1.0
    return out


def crop_keypoints24(part, center, scale, res=224):
    """j2d_processing without augmentation: transform() = trunc(t . (x, y, 1)) + 1 per point (image_utils.py:21-29,111-118)."""
    p = np.asarray(part, np.float64).copy()
    for n in range(p.shape[0]):
        h = 200.0 * float(np.asarray(scale).reshape(-1)[n])
        t = np.zeros((3, 3))
        t[0, 0] = t[1, 1] = float(res) / h
        t[0, 2] = res * (-float(center[n][0]) / h + 0.5)
        t[1, 2] = res * (-float(center[n][1]) / h + 0.5)
        t[2, 2] = 1.0
        for i in range(p.shape[1]):
            q = t @ np.array([p[n, i, 0], p[n, i, 1], 1.0])
            p[n, i, :2] = q[:2].astype(int) + 1
    return p.astype(f32)


# ---- scorer ------------------------------------------------------------------------------------------------------------------------
def _taps(n_dst, n_src, dtype):
    """align_corners=True taps of every destination index: (i0, i1, l, h).  float32: the device's expressions (scale and s rounded to
    float32); float64: the formula s = i (n_src - 1) / (n_dst - 1) itself."""
    i = np.arange(n_dst)
    if dtype == f32:
        scale = f32(n_src - 1) / f32(n_dst - 1) if n_dst > 1 else f32(0)
        s = (scale * i.astype(f32)).astype(f32)
    else:
        s = i.astype(np.float64) * (n_src - 1) / (n_dst - 1) if n_dst > 1 else np.zeros(n_dst)
    i0 = np.minimum(s.astype(np.int64), n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    l = (s - i0.astype(dtype)).astype(dtype)
    return i0, i1, l, (dtype(1) - l).astype(dtype)


def upsample(logits, H, W, dtype=f32):
    """logits [B,C,h,w] -> [B,C,H,W]: hy (hx v00 + lx v01) + ly (hx v10 + lx v11), in `dtype`, in this order."""
    v = np.asarray(logits).astype(dtype)
    h, w = v.shape[2:]
    y0, y1, ly, hy = _taps(H, h, dtype)
    x0, x1, lx, hx = _taps(W, w, dtype)
    ly, hy = ly[:, None], hy[:, None]
    top = hx * v[:, :, y0][:, :, :, x0] + lx * v[:, :, y0][:, :, :, x1]
    bot = hx * v[:, :, y1][:, :, :, x0] + lx * v[:, :, y1][:, :, :, x1]
    return (hy * top + ly * bot).astype(dtype)


def segm_score(logits, labels, dtype=f32):
    """(ce [B] = per-crop sum of -log_softmax[label], counts int64 [B, 1 + 3C] = correct, then per class intersection / predicted /
    ground truth, argmax uint8 [B,H,W]).  float32: per-pixel losses in float32, summed by np.sum in float32."""
    labels = np.asarray(labels).astype(np.int64)
    B, H, W = labels.shape
    C = logits.shape[1]
    up = upsample(logits, H, W, dtype)
    arg = np.argmax(up, axis=1)                                       # the first maximum: the lowest channel wins a tie
    m = up.max(axis=1)
    lse = m + np.log(np.exp(up - m[:, None]).sum(axis=1, dtype=dtype)).astype(dtype)
    at = np.take_along_axis(up, labels[:, None], axis=1)[:, 0]
    loss = (lse - at).astype(dtype)
    ce = loss.reshape(B, -1).sum(axis=1, dtype=dtype)
    counts = np.zeros((B, 1 + 3 * C), np.int64)
    for b in range(B):
        counts[b, 0] = np.count_nonzero(arg[b] == labels[b])
        for c in range(C):
            counts[b, 1 + 3 * c] = np.count_nonzero((arg[b] == c) & (labels[b] == c))
            counts[b, 2 + 3 * c] = np.count_nonzero(arg[b] == c)
            counts[b, 3 + 3 * c] = np.count_nonzero(labels[b] == c)
    return ce, counts, arg.astype(np.uint8)


def summarize(ce, counts, pixels_per_crop, C):
    """The summary SegmAccumulator.finish() gives, from per-crop sums."""
    n = len(ce) * pixels_per_crop
    tot = np.asarray(counts, np.float64).sum(0)
    cls = tot[1:].reshape(C, 3)
    union = cls[:, 1] + cls[:, 2] - cls[:, 0]
    iou = np.where(union > 0, cls[:, 0] / np.where(union > 0, union, 1), np.nan)
    return {"val_segm_ce": float(np.sum(np.asarray(ce, np.float64))) / n, "val_segm_pixel_acc": tot[0] / n, "val_segm_iou": iou,
            "val_segm_miou": float(np.nanmean(iou)), "val_segm_miou_fg": float(np.nanmean(iou[1:]))}


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------
SCORE_SHAPES = [(1, 25, 56, 56, 224, 224), (3, 25, 56, 56, 224, 224), (2, 3, 2, 2, 5, 7), (2, 32, 5, 3, 5, 3), (1, 25, 56, 56, 223, 221)]


def score_fixture(shape, seed=0):
    """(logits float32 [B,C,h,w], labels uint8 [B,H,W]) of one case: smooth logits that favour the label's class about two times in
    three, class C - 1 never the label, class 1 never the prediction (its logits are pushed down), and an exact two-way tie between
    channels 0 and 2 at pixel (0, 0) of every crop - a pixel that coincides with a source pixel, so the tie survives the upsample."""
    B, C, h, w, H, W = shape
    r = np.random.default_rng(1000 + seed + 7 * B + 13 * C + H)
    bs = max(1, min(16, H // 4))                                      # label blocks: 16 x 16 on the full maps, single pixels on the tiny ones
    blocks = r.integers(0, max(C - 1, 1), (B, (H + bs - 1) // bs, (W + bs - 1) // bs))
    labels = np.repeat(np.repeat(blocks, bs, 1), bs, 2)[:, :H, :W].astype(np.uint8)
    if C > 2:
        labels[:, H - 1, W - 1] = 1                                   # the class that is never predicted is present
    logits = r.normal(0, 1, (B, C, h, w)).astype(f32)
    ys = np.minimum(np.arange(h) * max(H - 1, 1) // max(h - 1, 1), H - 1)
    xs = np.minimum(np.arange(w) * max(W - 1, 1) // max(w - 1, 1), W - 1)
    src_lab = labels[:, ys][:, :, xs]
    boost = (r.random((B, h, w)) < 0.67) * f32(3)
    np.put_along_axis(logits, src_lab[:, None].astype(np.int64), np.take_along_axis(logits, src_lab[:, None].astype(np.int64), 1)
                      + boost[:, None].astype(f32), 1)
    if C > 2:
        logits[:, 1] -= f32(20)
        logits[:, :, 0, 0] = np.minimum(logits[:, :, 0, 0], f32(0.5))
        logits[:, 0, 0, 0] = f32(1.25)
        logits[:, 2, 0, 0] = f32(1.25)
    return logits.astype(f32), labels


def golden_logits():
    """The [3,25,56,56] / [3,224,224] case, the input of the reference's CrossEntropy in tests/golden/segm.npz."""
    return score_fixture(SCORE_SHAPES[1])


def translation_fixture(seed=5, B=6, J=24):
    """(S float32 [B,J,3], joints2d float32 [B,J,3]): joints of a body about 5000 * 2 / (224 * 0.9) m away, their projections with a
    little noise and confidences in (0, 1]; some confidences 0; the LAST row has every confidence 0: a singular system."""
    r = np.random.default_rng(seed)
    S = np.stack([r.uniform(-0.5, 0.5, (B, J)), r.uniform(-0.9, 0.8, (B, J)), r.uniform(-0.15, 0.15, (B, J))], -1)
    t = np.stack([r.uniform(-0.2, 0.2, B), r.uniform(-0.2, 0.2, B), r.uniform(30, 60, B)], -1)
    P = S + t[:, None]
    xy = 5000.0 * P[:, :, :2] / P[:, :, 2:] + 112.0 + r.normal(0, 0.7, (B, J, 2))
    conf = r.uniform(0.05, 1.0, (B, J))
    conf[r.random((B, J)) < 0.15] = 0.0
    conf[-1] = 0.0
    return S.astype(f32), np.concatenate([xy, conf[..., None]], -1).astype(f32)


# ---- test meshes -------------------------------------------------------------------------------------------------------------------
def hand_mesh(res=224, focal=4096.0, z=64.0):
    """A 40-face mesh built in SCREEN space at depth z and unprojected exactly (coordinates are multiples of 1/8 of a pixel and z and
    focal are chosen so that the projection gives them back bit for bit - asserted by the caller).  It holds
      - a fan of triangles around a vertex that sits exactly on a pixel centre, with shared edges through pixel centres;
      - two coplanar, overlapping faces of different parts (equal depth: the lower face index must win);
      - a back-facing (clockwise) triangle; a triangle that straddles the crop's border; a face behind Z = 0.1; a face with a NaN vertex.
    Returns (verts float32 [V,3] for cam_t = 0, faces int32 [40,3], face_part uint8 [40])."""
    pts, faces, parts = [], [], []

    def vert(px, py, zz=z):
        pts.append(((px - res / 2.0) * zz / focal, (py - res / 2.0) * zz / focal, zz))
        return len(pts) - 1

    def tri(a, b, c, part):
        faces.append((a, b, c))
        parts.append(part)

    # fan: centre on the pixel centre (40.5, 40.5); the rim passes through pixel centres, its edges through others
    c = vert(40.5, 40.5)
    rim = [vert(40.5 + dx, 40.5 + dy) for dx, dy in [(16, 0), (16, 16), (0, 16), (-16, 16), (-16, 0), (-16, -16), (0, -16), (16, -16)]]
    for k in range(8):
        tri(c, rim[k], rim[(k + 1) % 8], k)
    # a grid of 4 x 3 quads (24 triangles) whose vertices lie on pixel centres: every edge runs through centres
    gx, gy = 80.5, 20.5
    grid = [[vert(gx + 12 * i, gy + 10 * j, z + 0.5 * i) for i in range(5)] for j in range(4)]
    n = 0
    for j in range(3):
        for i in range(4):
            a, b, d, e = grid[j][i], grid[j][i + 1], grid[j + 1][i], grid[j + 1][i + 1]
            tri(a, b, e, 8 + n % 12)
            tri(a, e, d, 8 + (n + 5) % 12)
            n += 1
    # two coplanar overlapping faces at the same depth (face 32 before face 33)
    q = [vert(30.25, 100.25), vert(90.75, 100.25), vert(60.5, 150.5), vert(50.25, 90.75), vert(110.5, 120.5), vert(50.25, 150.25)]
    tri(q[0], q[1], q[2], 20)
    tri(q[3], q[4], q[5], 21)
    # back-facing (the winding of the fan reversed), in front of part of the grid
    tri(vert(100.5, 30.5, z - 1), vert(100.5, 60.5, z - 1), vert(130.5, 45.5, z - 1), 22)
    # straddles the border on two sides
    tri(vert(-30.25, 180.5), vert(40.5, 250.75), vert(60.5, 170.25), 23)
    # behind the near plane (one vertex at Z = 0.05), and a NaN vertex
    tri(vert(150.5, 150.5), vert(200.5, 150.5), vert(175.5, 200.5, 0.05), 1)
    tri(vert(150.5, 100.5), vert(200.5, 100.5), vert(float("nan"), 130.5), 2)
    # two more ordinary faces far behind everything, covering most of the crop: the background of the others
    far = [vert(5.5, 5.5, 2 * z), vert(215.5, 5.5, 2 * z), vert(215.5, 215.5, 2 * z), vert(5.5, 215.5, 2 * z)]
    tri(far[0], far[1], far[2], 3)
    tri(far[0], far[2], far[3], 4)
    assert len(faces) == 40
    return np.array(pts, f32), np.array(faces, np.int32), np.array(parts, np.uint8)
