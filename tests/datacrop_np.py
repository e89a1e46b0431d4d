"""Numpy restatement of the reference's DATASET crop and of the ground-truth transforms that go with it - the yardstick of
tests/test_datacrop_*.py.  Built on oracle/crop_np.py for cv2.getAffineTransform, warpAffine's inversion and
its fixed-point coordinates; added here:

  source points   gen_trans_from_patch_cv(c_x, c_y, bb, bb, res, res, scale=1.0, rot) up to `src` / `dst`
                  (pocolib/utils/vibe_image_utils.py:49-91) with the dtype chain of the reference's numpy 1.18: rotate_2d multiplies a
                  float32 scalar by the float64 sin / cos -> float64, stored as float32; src_center (float64) + that -> float64,
                  stored into the float32 `src`.  Every dtype is spelled out, so the result does not depend on the numpy installed.
  float blend     cv2.warpAffine on a FLOAT32 image (crop_cv2, image_utils.py:189-206; base_dataset.py:277 converts the image):
                  same coordinates as the uint8 path, but remapBilinear<float> with the float table (1-fy|fy)*(1-fx|fx), fx, fy in
                  32nds, and no rounding of the result.
  flip / noise    np.fliplr after the warp, min(255, max(0, v * pn[c])) on the float32 array (numpy 1.x: the float64 scalar is
                  cast to float32), / 255, Normalize (base_dataset.py:201-221,309).
  ground truth    pose_processing / rot_aa / flip_pose, j3d_processing / flip_kp, j2d_processing / transform, calculate_bbox_info
                  (base_dataset.py:223-262, image_utils.py:21-45,111-118,174-187,236-278).
cv2 itself is absent here: crop_cv2 and rot_aa (cv2.Rodrigues) are restated from OpenCV's published algorithm, not run;
tools/validate_assets.py --dataset-crop compares with the real cv2 where it is importable."""
import numpy as np

from oracle import crop_np

SMPL_JOINTS_FLIP_PERM = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]      # constants.py:104
SMPL_POSE_FLIP_PERM = [3 * i + k for i in SMPL_JOINTS_FLIP_PERM for k in range(3)]                                 # constants.py:105-109
J24_FLIP_PERM = [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22]              # constants.py:111


def py_round(v) -> int:
    """int(round(v)) of crop_cv2: Python's round, half to even, on the value as a float64."""
    return int(round(float(v)))


def rotate_2d(x32, y32, rot_rad):
    """vibe_image_utils.py:49-55 on a float32 point: float64 products, float32 result."""
    sn, cs = np.float64(np.sin(rot_rad)), np.float64(np.cos(rot_rad))
    x, y = np.float64(np.float32(x32)), np.float64(np.float32(y32))
    return np.float32(x * cs - y * sn), np.float32(x * sn + y * cs)


def patch_points(c_x: int, c_y: int, bb: int, res: int, rot: float):
    """`src`, `dst` [3,2] float32 of gen_trans_from_patch_cv(c_x, c_y, bb, bb, res, res, scale=1.0, rot)."""
    src_w = src_h = float(bb) * 1.0
    rot_rad = np.pi * float(rot) / 180
    down = rotate_2d(np.float32(0), np.float32(src_h * 0.5), rot_rad)
    right = rotate_2d(np.float32(src_w * 0.5), np.float32(0), rot_rad)
    cx, cy = np.float64(c_x), np.float64(c_y)
    src = np.zeros((3, 2), np.float32)
    src[0] = (cx, cy)
    src[1] = (cx + np.float64(down[0]), cy + np.float64(down[1]))
    src[2] = (cx + np.float64(right[0]), cy + np.float64(right[1]))
    half = np.float32(res * 0.5)
    dst = np.array([[half, half], [half, half + half], [half + half, half]], np.float32)
    return src, dst


def warp_affine_f32(img, M, res):
    """cv2.warpAffine(img float32 [H,W,C] holding byte values, M 2x3 float64, (res,res), INTER_LINEAR, BORDER_CONSTANT 0) ->
    float32 [res,res,C]: the coordinates of crop_np.warp_affine_u8, remapBilinear<float> for the blend."""
    H, W = img.shape[:2]
    Mi = crop_np.invert_affine_cv(M)
    AB = float(1 << crop_np.AB_BITS)
    TAB = crop_np.TAB
    xs = np.arange(res, dtype=np.float64)
    adelta = np.rint(Mi[0] * xs * AB).astype(np.int64)
    bdelta = np.rint(Mi[3] * xs * AB).astype(np.int64)
    rd = (1 << crop_np.AB_BITS) // TAB // 2
    X0 = np.rint((Mi[1] * xs + Mi[2]) * AB).astype(np.int64) + rd
    Y0 = np.rint((Mi[4] * xs + Mi[5]) * AB).astype(np.int64) + rd
    X = (X0[:, None] + adelta[None, :]) >> (crop_np.AB_BITS - crop_np.INTER_BITS)
    Y = (Y0[:, None] + bdelta[None, :]) >> (crop_np.AB_BITS - crop_np.INTER_BITS)
    sx = np.clip(X >> crop_np.INTER_BITS, -32768, 32767)
    sy = np.clip(Y >> crop_np.INTER_BITS, -32768, 32767)
    # initInterTab1D(INTER_LINEAR): tab[i] = (1 - i/32, i/32) in float32; the 2-D table is their float32 product
    t = np.arange(TAB, dtype=np.float32) * np.float32(1.0 / TAB)
    t1 = np.stack([np.float32(1.0) - t, t], 1)
    fx, fy = X & (TAB - 1), Y & (TAB - 1)
    w = [(t1[fy, a] * t1[fx, b]).astype(np.float32)[..., None] for a in (0, 1) for b in (0, 1)]     # y0x0, y0x1, y1x0, y1x1
    f = img.astype(np.float32)

    def px(xx, yy):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = f[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(ok[..., None], v, np.float32(0))

    out = px(sx, sy) * w[0] + px(sx + 1, sy) * w[1] + px(sx, sy + 1) * w[2] + px(sx + 1, sy + 1) * w[3]
    assert out.dtype == np.float32
    return out


def crop_cv2_np(img_u8, center, scale, res, rot=0.0):
    """crop_cv2(img.astype(float32), center, scale, [res, res], rot) (image_utils.py:189-206): float32 [res,res,3]."""
    c_x, c_y = py_round(center[0]), py_round(center[1])
    bb = py_round(float(scale) * 200.0)
    src, dst = patch_points(c_x, c_y, bb, res, rot)
    return warp_affine_f32(img_u8, crop_np.get_affine_transform_cv(src, dst), res)


def rgb_processing_np(img_u8, center, scale, rot, flip, pn, res=224, normalize=True):
    """rgb_processing (base_dataset.py:201-221) without occluders, then normalize_img: float32 [3,res,res].  `scale` is already
    sc * scale.  normalize=False: the raw float crop after noise and clamp (what the kernel hands out with normalize = 0)."""
    x = crop_cv2_np(img_u8, center, scale, res, rot)
    if flip:
        x = np.fliplr(x)
    x = np.array(x, np.float32)
    for c in range(3):
        x[:, :, c] = np.minimum(np.float32(255.0), np.maximum(np.float32(0.0), x[:, :, c] * np.float32(pn[c])))
    if not normalize:
        return np.ascontiguousarray(x.transpose(2, 0, 1))
    x = x / np.float32(255.0)
    return np.ascontiguousarray(((x - crop_np.MEAN) / crop_np.STD).astype(np.float32).transpose(2, 0, 1))


def dataset_crop_np(images, img_index, centers, scales, rots, flips, pns, res=224, normalize=True):
    """The batch: crop n is cut from images[img_index[n]] with scale `scales[n]` (= sc * scale).  float32 [N,3,res,res]."""
    return np.stack([rgb_processing_np(images[int(img_index[n])], centers[n], scales[n], rots[n], flips[n], pns[n], res, normalize)
                     for n in range(len(img_index))])


# ---- ground truth ----------------------------------------------------------------------------------------------------------------
def rot_aa_np(aa, rot):
    """rot_aa (image_utils.py:236-247): Rodrigues -> Rz(-rot) . R -> axis-angle, with scipy's Rotation standing in for cv2.Rodrigues."""
    from scipy.spatial.transform import Rotation
    a = np.deg2rad(-float(rot))
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    per = Rotation.from_rotvec(np.asarray(aa, np.float64)).as_matrix()
    return Rotation.from_matrix(R @ per).as_rotvec()


def flip_pose_np(pose):
    p = np.asarray(pose)[SMPL_POSE_FLIP_PERM].copy()
    p[1::3] = -p[1::3]
    p[2::3] = -p[2::3]
    return p


def flip_kp_np(kp):
    k = np.asarray(kp)[J24_FLIP_PERM].copy()
    k[:, 0] = -k[:, 0]
    return k


def pose_processing_np(pose, r, f):
    p = np.array(pose, np.float64)
    p[:3] = rot_aa_np(p[:3], r)
    if f:
        p = flip_pose_np(p)
    return p.astype(np.float32)


def j3d_processing_np(S, r, f):
    S = np.array(S, np.float64)
    rot_mat = np.eye(3)
    if not r == 0:
        rot_rad = -r * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
    S[:, :3] = np.einsum("ij,kj->ki", rot_mat, S[:, :3])
    if f:
        S = flip_kp_np(S)
    return S.astype(np.float32)


def get_transform_np(center, scale, res, rot=0):
    h = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0] = float(res[1]) / h
    t[1, 1] = float(res[0]) / h
    t[0, 2] = res[1] * (-float(center[0]) / h + .5)
    t[1, 2] = res[0] * (-float(center[1]) / h + .5)
    t[2, 2] = 1
    if not rot == 0:
        rot = -rot
        rot_mat = np.zeros((3, 3))
        rot_rad = rot * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
        rot_mat[2, 2] = 1
        t_mat = np.eye(3)
        t_mat[0, 2] = -res[1] / 2
        t_mat[1, 2] = -res[0] / 2
        t_inv = t_mat.copy()
        t_inv[:2, 2] *= -1
        t = np.dot(t_inv, np.dot(rot_mat, np.dot(t_mat, t)))
    return t


def transform_np(pt, center, scale, res, rot=0):
    t = get_transform_np(center, scale, res, rot)
    new_pt = np.dot(t, np.array([pt[0] - 1, pt[1] - 1, 1.]).T)
    return new_pt[:2].astype(int) + 1


def j2d_processing_np(kp, center, scale, r, f, res=224):
    """base_dataset.py:223-235 on `part` [24,3] (x, y, confidence): float32 [24,3] in normalised crop coordinates."""
    kp = np.array(kp, np.float64)
    for i in range(kp.shape[0]):
        kp[i, 0:2] = transform_np(kp[i, 0:2] + 1, center, scale, [res, res], rot=r)
    kp[:, :-1] = 2. * kp[:, :-1] / res - 1.
    if f:
        kp = flip_kp_np(kp)
    return kp.astype(np.float32)


def bbox_info_np(center, scale, orig_shape):
    """calculate_bbox_info (image_utils.py:174-187) with scale = sc * scale."""
    img_h, img_w = orig_shape[0], orig_shape[1]
    focal = float((img_w ** 2 + img_h ** 2) ** 0.5)
    b = np.array([center[0] - img_w / 2., center[1] - img_h / 2., scale * 200])
    b[:2] = b[:2] / focal * 2.8
    b[2] = (b[2] - 0.24 * focal) / (0.06 * focal)
    return b.astype(np.float32)


def augm_params_np(cfg, is_train):
    """augm_params (base_dataset.py:172-199) on numpy's global generator; cfg = dict(FLIP, NOISE_FACTOR, ROT_FACTOR, SCALE_FACTOR)."""
    flip, pn, rot, sc = 0, np.ones(3), 0, 1
    if is_train:
        if np.random.uniform() <= 0.5 and cfg["FLIP"]:
            flip = 1
        pn = np.random.uniform(1 - cfg["NOISE_FACTOR"], 1 + cfg["NOISE_FACTOR"], 3)
        rot = min(2 * cfg["ROT_FACTOR"], max(-2 * cfg["ROT_FACTOR"], np.random.randn() * cfg["ROT_FACTOR"]))
        sc = min(1 + cfg["SCALE_FACTOR"], max(1 - cfg["SCALE_FACTOR"], np.random.randn() * cfg["SCALE_FACTOR"] + 1))
        if np.random.uniform() <= 0.6:
            rot = 0
    return flip, pn, rot, sc
