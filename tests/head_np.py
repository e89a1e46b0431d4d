"""Plain numpy statements of the head kernels' operations (tests/test_head_kernels_gpu.py).  Every function takes the dtype it
evaluates in: float64 is the reference, float32 the same formula at the kernels' precision - its distance from the reference is the
first term of the tolerance procedure (NOTEBOOK.md, "Head kernels alone")."""
import numpy as np

SMPL_PARENT = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)


def camera(cam, joints49, cliff, focal=None, scale=None, center=None, orig_shape=None, dtype=np.float64):
    """cam [B,3] = (s, tx, ty), joints49 [B,49,3] -> (cam_t [B,3], fullimg_cam_t [B,3] | None, joints2d [B,49,2]).
    PARE: weak perspective -> perspective with focal 5000 on the 224 crop, projected and divided by 112.  CLIFF: the translation in
    full-image coordinates (focal [B], scale [B] = box height / 200, center [B,2] = (x, y), orig_shape [B,2] = (h, w)), projected
    with the crop's focal length about the image centre."""
    t = lambda a: np.asarray(a, dtype=dtype)
    cam, J = t(cam), t(joints49)
    s, tx, ty = cam[:, 0], cam[:, 1], cam[:, 2]
    cam_t = np.stack([tx, ty, dtype(2) * dtype(5000) / (dtype(224) * s + dtype(1e-9))], -1)
    if not cliff:
        P = J + cam_t[:, None]
        uv = dtype(5000) * (P[..., :2] / P[..., 2:3]) / dtype(112)
        return cam_t, None, uv
    focal, scale, center, shape = t(focal), t(scale), t(center), t(orig_shape)
    bh = scale * dtype(200)
    h, w = shape[:, 0], shape[:, 1]
    tz = dtype(2) * focal / (bh / dtype(224) * dtype(224) * s)
    ox = dtype(2) * (center[:, 0] - w / dtype(2)) / (s * bh)
    oy = dtype(2) * (center[:, 1] - h / dtype(2)) / (s * bh)
    full = np.stack([tx + ox, ty + oy, tz], -1)
    P = J + full[:, None]
    uv = focal[:, None, None] * (P[..., :2] / P[..., 2:3]) + np.stack([w, h], -1)[:, None] / dtype(2)
    return cam_t, full, uv


def rot6d(x, dtype=np.float64):
    """x [..., 6] = a 3x2 matrix row-major -> [..., 3, 3] with columns b1, b2, b3: Gram-Schmidt with F.normalize's clamp (a norm
    below 1e-12 is replaced by 1e-12, so a zero vector stays zero instead of becoming NaN)."""
    x = np.asarray(x, dtype=dtype).reshape(x.shape[:-1] + (3, 2))
    a1, a2 = x[..., 0], x[..., 1]
    eps = dtype(1e-12)
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(-1, keepdims=True)), eps)
    u = a2 - (b1 * a2).sum(-1, keepdims=True) * b1
    b2 = u / np.maximum(np.sqrt((u * u).sum(-1, keepdims=True)), eps)
    return np.stack([b1, b2, np.cross(b1, b2)], -1)


def lc2d(x, w, dtype=np.float64):
    """x [B,128,24], w [6,128,24] -> [B,24,6]: a separate 128 -> 6 linear map per joint."""
    return np.einsum("bcj,ocj->bjo", np.asarray(x, dtype=dtype), np.asarray(w, dtype=dtype))


def part_attention(feat, heat, dtype=np.float64):
    """feat [B,C,H,W], heat [B,24,H,W] -> [B,C,24]: softmax over the pixels of every part map, then the weighted feature sum."""
    B, C = feat.shape[:2]
    f = np.asarray(feat, dtype=dtype).reshape(B, C, -1)
    h = np.asarray(heat, dtype=dtype).reshape(B, 24, -1)
    e = np.exp(h - h.max(-1, keepdims=True))
    return np.einsum("bcp,bjp->bcj", f, e / e.sum(-1, keepdims=True))


def linear(x, W, b, act=0, res=None, dtype=np.float64):
    """act(b + x W^T (+ res)): act 0 none, 1 ReLU, 2 sigmoid."""
    y = np.asarray(x, dtype=dtype) @ np.asarray(W, dtype=dtype).T + np.asarray(b, dtype=dtype)
    if res is not None:
        y = y + np.asarray(res, dtype=dtype)
    if act == 1:
        y = np.maximum(y, 0)
    elif act == 2:
        y = dtype(1) / (dtype(1) + np.exp(-y))
    return y


def confidence(var, cliff, kinematic, thr, dtype=np.float64):
    """var [B,24] -> [B]: accumulate along the SMPL tree (children in the order 1..23), a crop whose root exceeds the threshold
    (2 thr for CLIFF) counts as 1 everywhere, CLIFF takes the root and PARE the mean, clipped to [0, 0.99]."""
    v = np.array(var, dtype=dtype)
    if kinematic:
        for j in range(1, 24):
            v[:, j] += v[:, SMPL_PARENT[j]]
    v[v[:, 0] > dtype((2 if cliff else 1) * thr)] = 1
    g = v[:, 0] if cliff else v.sum(-1) / dtype(24)
    return np.clip(g, 0, dtype(0.99))
