"""Numpy restatement of the reference's synthetic occluders (pocolib/dataset/occlusion.py:109-149,247-288) inside the dataset crop -
the yardstick of tests/test_occlude_*.py.  Built on tests/datacrop_np.py for everything around the step:

  draws      occlude_with_pascal_objects_kp up to its two calls that touch pixels, on numpy's and Python's GLOBAL generators as the
             reference uses them (poco_amd/datacrop.py occlusion_params restates the same on generator objects)
  resize     cv2.resize(uint8 RGBA, dsize, interpolation=INTER_AREA) from OpenCV's published algorithm
             (modules/imgproc/src/resize.cpp: resizeAreaFast_, computeResizeAreaTab, ResizeArea_Invoker), every dtype spelled out
  paste      paste_over on the float32 crop
cv2 is absent here: the resize is restated, not run (tools/validate_assets.py --occlusion compares where opencv-python is
installed).  The two cases in which the reference raises are settled as DESIGN.md section 23 says: no visible keypoint leaves the
sample unoccluded after its count draw; a new size with a zero side skips that object after its draws."""
import random

import numpy as np

from tests import datacrop_np

DBL_EPSILON = 2.220446049250313e-16
F32 = np.float32


# ---- cv2.resize(..., INTER_AREA) -------------------------------------------------------------------------------------------------
def area_tab(ssize: int, dsize: int):
    """cv::computeResizeAreaTab for one axis: per destination index the list of (source index, float32 weight), in table order."""
    scale = ssize / float(dsize)
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = int(np.ceil(f1)), int(np.floor(f2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        ent = []
        if s1 - f1 > 1e-3:
            ent.append((s1 - 1, F32((s1 - f1) / cell)))
        for s in range(s1, s2):
            ent.append((s, F32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            ent.append((s2, F32(min(min(f2 - s2, 1.), cell) / cell)))
        tab.append(ent)
    return tab


def _integer_scale(ssize: int, dsize: int) -> bool:
    scale = ssize / float(dsize)
    return abs(scale - np.rint(scale)) < DBL_EPSILON


def resize_path(src_hw, dsize) -> str:
    """Which of OpenCV's paths cv2.resize(src, dsize=(w, h), INTER_AREA) takes: 'copy', 'fast' or 'generic'."""
    (h, w), (dw, dh) = src_hw, dsize
    if (dw, dh) == (w, h):
        return "copy"
    return "fast" if _integer_scale(w, dw) and _integer_scale(h, dh) else "generic"


def _round_byte(x32):
    """saturate_cast<uchar>(float): cvRound (half to even), saturated."""
    return np.clip(np.rint(np.asarray(x32, F32)), 0, 255).astype(np.uint8)


def resize_area(src, dsize):
    """cv2.resize(src uint8 [h, w, C], (dst_w, dst_h), interpolation=cv2.INTER_AREA) -> uint8 [dst_h, dst_w, C].  A destination
    side below 1 or above the source side is a ValueError (cv2 raises on the former; the latter would need INTER_LINEAR)."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3:
        raise ValueError(f"resize_area: need uint8 [h, w, C], got {src.dtype} {src.shape}")
    h, w, C = src.shape
    dw, dh = int(dsize[0]), int(dsize[1])
    if not (1 <= dw <= w and 1 <= dh <= h):
        raise ValueError(f"resize_area: {w} x {h} to {dw} x {dh}: each side must be in 1..source")
    path = resize_path((h, w), (dw, dh))
    if path == "copy":
        return src.copy()
    if path == "fast":
        bx, by = w // dw, h // dh
        s = src.astype(np.int64).reshape(dh, by, dw, bx, C).sum(axis=(1, 3))
        if bx == 2 and by == 2:
            return ((s + 2) >> 2).astype(np.uint8)
        return _round_byte(s.astype(F32) * (F32(1.0) / F32(bx * by)))
    xtab, ytab = area_tab(w, dw), area_tab(h, dh)
    S = src.astype(F32)
    # per source row: buf[dx] = 0, then buf[dx] += S[sx] * alpha in table order
    buf = np.zeros((h, dw, C), F32)
    for dx, ent in enumerate(xtab):
        for sx, a in ent:
            buf[:, dx] = buf[:, dx] + S[:, sx] * a
    out = np.zeros((dh, dw, C), F32)
    for dy, ent in enumerate(ytab):
        for k, (sy, b) in enumerate(ent):
            out[dy] = b * buf[sy] if k == 0 else out[dy] + b * buf[sy]
    assert buf.dtype == F32 and out.dtype == F32
    return _round_byte(out)


# ---- paste_over ------------------------------------------------------------------------------------------------------------------
def paste_over_np(im_src, im_dst, center):
    """paste_over (occlusion.py:247-279), in place on the float32 im_dst [H, W, 3]; returns the mask [H, W] of the pixels that a
    pasted texel with alpha > 0 touched."""
    assert im_dst.dtype == F32 and im_src.dtype == np.uint8
    wh_src = np.asarray([im_src.shape[1], im_src.shape[0]])
    wh_dst = np.asarray([im_dst.shape[1], im_dst.shape[0]])
    center = np.round(center).astype(np.int32)
    raw_start = center - wh_src // 2
    raw_end = raw_start + wh_src
    start, end = np.clip(raw_start, 0, wh_dst), np.clip(raw_end, 0, wh_dst)
    region_dst = im_dst[start[1]:end[1], start[0]:end[0]]
    s0 = start - raw_start
    s1 = wh_src + (end - raw_end)
    region_src = im_src[s0[1]:s1[1], s0[0]:s1[0]]
    color = region_src[..., 0:3].astype(F32)
    alpha = region_src[..., 3:].astype(F32) / F32(255)
    im_dst[start[1]:end[1], start[0]:end[0]] = alpha * color + (F32(1) - alpha) * region_dst
    touched = np.zeros(im_dst.shape[:2], bool)
    touched[start[1]:end[1], start[0]:end[0]] = region_src[..., 3] > 0
    return touched


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def occlusion_draws_np(kp24, scale, occluder_hw, res):
    """occlude_with_pascal_objects_kp up to resize_by_factor / paste_over, on the global np.random and random generators.
    kp24 float32 [24, 3]: the ground-truth keypoints after j2d_processing (normalised); scale = sc * scale; occluder_hw: (h, w) per
    cut-out.  Returns dict(count = the count drawn, objects = [(id, dst_w, dst_h, cx, cy)] of the objects kept, skipped, no_visible)."""
    im_w = im_h = int(res)
    im_scale_factor = min(im_w, im_h) / 256
    count = np.random.randint(1, 8)
    kp = np.array(kp24, F32)
    kp[:, :-1] = F32(0.5 * 224) * (kp[:, :-1] + F32(1))
    visible = kp[kp[..., -1] > 0.3]
    if len(visible) == 0:
        return dict(count=int(count), objects=[], skipped=0, no_visible=True)
    objects, skipped = [], 0
    for _ in range(count):
        oid = random.choice(range(len(occluder_hw)))
        x, y = visible[np.random.choice(range(len(visible)), 1)[0]][:2]
        delta_x = np.float64((np.random.randn() * 0.1) * scale)
        delta_y = np.float64((np.random.randn() * 0.1) * scale)
        cx = int(np.clip(np.float64(x) + delta_x, 0, im_w))
        cy = int(np.clip(np.float64(y) + delta_y, 0, im_h))
        factor = np.random.uniform(0.2, 1.0) * im_scale_factor + 1e-8
        h, w = occluder_hw[oid]
        new = np.round(np.array([w, h]) * factor).astype(int)
        if new[0] < 1 or new[1] < 1:
            skipped += 1
            continue
        objects.append((int(oid), int(new[0]), int(new[1]), cx, cy))
    return dict(count=int(count), objects=objects, skipped=skipped, no_visible=False)


def apply_objects_np(crop, occluders, objects):
    """The objects [(id, dst_w, dst_h, cx, cy)] pasted in order onto a copy of the float32 crop [res, res, 3]: (result, touched mask)."""
    out = np.array(crop, F32)
    touched = np.zeros(out.shape[:2], bool)
    for oid, dw, dh, cx, cy in objects:
        touched |= paste_over_np(resize_area(occluders[oid], (dw, dh)), out, np.array([cx, cy]))
    return out, touched


def synthetic_crop(res: int, k: int) -> np.ndarray:
    """A float32 [res, res, 3] crop with values in [0, 255] and fractions in 1/1024ths, as the dataset crop makes them: a smooth
    pattern (it compresses well in the fixture) that differs per k."""
    y, x, c = np.meshgrid(np.arange(res), np.arange(res), np.arange(3), indexing="ij")
    v = ((x * (3 + k) + y * (5 + 2 * k) + c * 61) % 256) * 1024 - ((x + 2 * y + k) % 7) * 97
    return (np.clip(v, 0, 255 * 1024).astype(np.int64).astype(F32) / F32(1024)).astype(F32)


# ---- the whole crop --------------------------------------------------------------------------------------------------------------
def rgb_processing_occ_np(img_u8, center, scale, rot, flip, pn, occluders, objects, res=224, normalize=True):
    """rgb_processing (base_dataset.py:201-221) with the occluder step, then normalize_img: (float32 [3, res, res], pixels touched).
    `objects` are the sample's drawn objects (occlusion_draws_np / datacrop.occlusion_params)."""
    x = datacrop_np.crop_cv2_np(img_u8, center, scale, res, rot)
    if flip:
        x = np.fliplr(x)
    x, touched = apply_objects_np(x, occluders, objects)
    for c in range(3):
        x[:, :, c] = np.minimum(F32(255.0), np.maximum(F32(0.0), x[:, :, c] * F32(pn[c])))
    if normalize:
        x = (((x / F32(255.0)) - datacrop_np.crop_np.MEAN) / datacrop_np.crop_np.STD).astype(F32)
    return np.ascontiguousarray(x.transpose(2, 0, 1)), int(touched.sum())


def dataset_crop_occ_np(images, img_index, centers, scales, rots, flips, pns, occluders, objects, res=224, normalize=True):
    """The batch: (float32 [N, 3, res, res], cover int64 [N])."""
    outs = [rgb_processing_occ_np(images[int(img_index[n])], centers[n], scales[n], rots[n], flips[n], pns[n], occluders, objects[n], res,
                                  normalize) for n in range(len(img_index))]
    return np.stack([o for o, _ in outs]), np.asarray([c for _, c in outs], np.int64)
