"""numpy restatement of the occlusion sensitivity sweep (poco_amd/occlusion.py, csrc/occlusion.hip): the sweep
positions, kernel A (occluded copies, bit-exact), kernel B (records, float64) and kernel C (heat map over the crop, float32 in the
kernel's operation order, byte-exact).  Not a test module."""
import numpy as np

REC = 77


def sweep_positions(res=224, patch=40, stride=10):
    """(y0, x0) row-major: per axis k * stride, k = 0 .. ceil((res - patch) / stride), the last clamped to res - patch."""
    if res < 1 or not 1 <= patch <= res or stride < 1:
        raise ValueError("need 1 <= patch <= res and stride >= 1")
    axis = []
    k = 0
    while True:
        axis.append(min(k * stride, res - patch))
        if k * stride >= res - patch:
            break
        k += 1
    return np.array([(y, x) for y in axis for x in axis], np.int32).reshape(-1, 2)


def occlude_batch(src, positions, patch, fill=(0.0, 0.0, 0.0)):
    """src float32 [3,res,res] -> [m,3,res,res]: the source everywhere, fill[c] inside each copy's patch."""
    src = np.asarray(src, np.float32)
    pos = np.asarray(positions).reshape(-1, 2)
    out = np.repeat(src[None], len(pos), 0)
    res = src.shape[1]
    for i, (y0, x0) in enumerate(pos):
        ys, xs = slice(max(int(y0), 0), max(min(int(y0) + patch, res), 0)), slice(max(int(x0), 0), max(min(int(x0) + patch, res), 0))
        for c in range(3):
            out[i, c, ys, xs] = np.float32(fill[c])
    return out


def occlusion_records(verts, var_pose, joints3d, base_verts, base_var, base_joints3d):
    """float64 [m,77] from float32 inputs: [0] mean, [1] max of |v_occ - v_base| over the vertices, [2] mean var_occ, [3] mean of
    var_occ - var_base, [4:28] var_occ - var_base, [28:77] |j3d_occ - j3d_base| of the 49 joints."""
    v = np.asarray(verts, np.float64)
    m = v.shape[0]
    bv = np.asarray(base_verts, np.float64).reshape(-1, 3)
    va, ba = np.asarray(var_pose, np.float64).reshape(m, 24), np.asarray(base_var, np.float64).reshape(24)
    j, bj = np.asarray(joints3d, np.float64).reshape(m, 49, 3), np.asarray(base_joints3d, np.float64).reshape(49, 3)
    rec = np.zeros((m, REC), np.float64)
    d = np.sqrt(((v - bv[None]) ** 2).sum(-1))
    rec[:, 0] = d.mean(1)
    rec[:, 1] = d.max(1)
    rec[:, 2] = va.mean(1)
    rec[:, 3] = (va - ba[None]).mean(1)
    rec[:, 4:28] = va - ba[None]
    rec[:, 28:77] = np.sqrt(((j - bj[None]) ** 2).sum(-1))
    return rec


def heat_overlay(field, positions, patch, crop, lut_u8, scale="auto"):
    """crop uint8 [res,res,3] -> the blended heat map, in the kernel's float32 operation order: per pixel the field is summed over
    the covering patches in position order, divided by their count, divided by the scale, clamped (NaN -> 0), index =
    int(255 t + 0.5) into lut_u8 [256,3], out = (128 lut + 128 crop + 128) >> 8.  scale "auto" = the field's maximum (NaN
    skipped); a maximum that is no positive finite number leaves the crop unchanged."""
    f = np.asarray(field, np.float32).reshape(-1)
    pos = np.asarray(positions).reshape(-1, 2)
    crop = np.asarray(crop, np.uint8)
    res = crop.shape[0]
    if isinstance(scale, str):
        assert scale == "auto"
        sc = np.float32(np.fmax.reduce(f, initial=np.float32(-np.inf)))
    else:
        sc = np.float32(scale)
    if not (sc > 0 and np.isfinite(sc)):
        return crop.copy()
    total = np.zeros((res, res), np.float32)
    count = np.zeros((res, res), np.int32)
    for i, (y0, x0) in enumerate(pos):                     # position order: every float32 add is rounded on its own
        ys, xs = slice(max(int(y0), 0), max(min(int(y0) + patch, res), 0)), slice(max(int(x0), 0), max(min(int(x0) + patch, res), 0))
        total[ys, xs] = total[ys, xs] + f[i]
        count[ys, xs] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        value = total / np.maximum(count, 1).astype(np.float32)
        t = value / sc
    t = np.where(t > 0, t, np.float32(0))                 # NaN and negatives -> 0
    t = np.where(t > 1, np.float32(1), t).astype(np.float32)
    idx = (np.float32(255) * t + np.float32(0.5)).astype(np.int32)
    col = np.asarray(lut_u8, np.uint8)[idx].astype(np.int32)
    out = ((128 * col + 128 * crop.astype(np.int32) + 128) >> 8).astype(np.uint8)
    return np.where((count > 0)[..., None], out, crop)


def field_of(records, metric="v2v"):
    r = np.asarray(records)
    if metric == "v2v":
        return np.ascontiguousarray(r[:, 0], np.float32)
    if metric == "var":
        return np.ascontiguousarray(r[:, 3], np.float32)
    if metric == "joints":
        return r[:, 28:77].astype(np.float32).mean(1, dtype=np.float32)
    return np.ascontiguousarray(r[:, 4 + int(str(metric).split(":")[-1])], np.float32)


def period_crop(res=224, period=64, seed=0):
    """A uint8 [res,res,3] test crop: one seeded period x period tile repeated over the crop."""
    tile = np.random.default_rng(seed).integers(0, 256, (period, period, 3), dtype=np.uint8)
    reps = -(-res // period)
    return np.ascontiguousarray(np.tile(tile, (reps, reps, 1))[:res, :res])
