"""The pseudo-labeler's contract of include/poco_hip.h ("pseudo-labeler") restated in numpy: the yardstick of
tests/test_pseudo_*.py and tests/test_demo_dataset_gpu.py and the host path tools/bench_pseudo.py times.  dtype = np.float32 mirrors
the reference (torch float32 there), np.float64 is the yardstick.  Each function cites the reference lines it restates; none of
their text is copied.

    rotmat_to_aa       geometry.py:264-429 (rotation_matrix_to_angle_axis through rotation_matrix_to_quaternion and
                       quaternion_to_angle_axis)
    trailing_mean      poco_utils.py:67-70 (what postproc.prepare_uncert computes, without the accumulation)
    kinematic          poco_utils.py:21-25
    confident_frames   train_utils.py:31-45
    crop_to_image      demo_utils.py:268-281
    step               tester.py:194-196,232-233 + the record layout and the stable compaction of csrc/pseudo_gt.hip
"""
import numpy as np

from poco_amd.synth import SMPL_PARENTS
from tests.eval_np import rodrigues  # noqa: F401  (the round trip's other half)

RECORD_FLOATS = 384
# record offsets (include/poco_hip.h)
P_SRC, P_CENTER, P_SCALE, P_POSE, P_SHAPE, P_VAR, P_OPENPOSE, P_PART, P_S, P_PAD = 0, 1, 3, 4, 76, 86, 110, 185, 257, 353
UNWRITTEN = 0xFFFFFFFF


def rotmat_to_aa(R, dtype=np.float64):
    """R [N,3,3] float32 -> axis-angle [N,3] float32.  The three branch comparisons are made on the float32 inputs with
    eps = float32(1e-6) whatever dtype carries the arithmetic; the four candidates are multiplied by their masks and added, so a NaN
    reaches every component; k = 2 where sin^2 is not positive; NaN results become 0."""
    Rf = np.asarray(R, np.float32).reshape(-1, 3, 3)
    d2 = Rf[:, 2, 2] < np.float32(1e-6)
    d0_d1 = Rf[:, 0, 0] > Rf[:, 1, 1]
    d0_nd1 = Rf[:, 0, 0] < -Rf[:, 1, 1]
    m = [(d2 & d0_d1), (d2 & ~d0_d1), (~d2 & d0_nd1), (~d2 & ~d0_nd1)]
    m = [x.astype(dtype)[:, None] for x in m]
    A = Rf.astype(dtype)
    one = dtype(1)
    r = lambda i, j: A[:, i, j]   # noqa: E731
    # rmat_t[i][j] = R[j][i]
    t0 = one + r(0, 0) - r(1, 1) - r(2, 2)
    t1 = one - r(0, 0) + r(1, 1) - r(2, 2)
    t2 = one - r(0, 0) - r(1, 1) + r(2, 2)
    t3 = one + r(0, 0) + r(1, 1) + r(2, 2)
    q0 = np.stack([r(2, 1) - r(1, 2), t0, r(1, 0) + r(0, 1), r(0, 2) + r(2, 0)], -1)
    q1 = np.stack([r(0, 2) - r(2, 0), r(1, 0) + r(0, 1), t1, r(2, 1) + r(1, 2)], -1)
    q2 = np.stack([r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(2, 1) + r(1, 2), t2], -1)
    q3 = np.stack([t3, r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)], -1)
    with np.errstate(all="ignore"):
        q = q0 * m[0] + q1 * m[1] + q2 * m[2] + q3 * m[3]
        q = q / np.sqrt(t0[:, None] * m[0] + t1[:, None] * m[1] + t2[:, None] * m[2] + t3[:, None] * m[3])
        q = q * dtype(0.5)
        s2 = q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
        s = np.sqrt(s2)
        c = q[:, 0]
        two_theta = dtype(2) * np.where(c < 0, np.arctan2(-s, -c), np.arctan2(s, c))
        k = np.where(s2 > 0, two_theta / s, dtype(2))
        aa = q[:, 1:] * k[:, None]
    aa = np.asarray(aa, dtype)
    aa[np.isnan(aa)] = 0
    return aa.astype(np.float32)


def quaternion_branch(R):
    """Which of the four candidates rotation_matrix_to_quaternion takes, per matrix (0..3)."""
    Rf = np.asarray(R, np.float32).reshape(-1, 3, 3)
    d2 = Rf[:, 2, 2] < np.float32(1e-6)
    return np.where(d2, np.where(Rf[:, 0, 0] > Rf[:, 1, 1], 0, 1), np.where(Rf[:, 0, 0] < -Rf[:, 1, 1], 2, 3))


def trailing_mean(var_pose):
    """[B,24] as it is, [B,24,T] averaged over T: float32, numpy's own order."""
    v = np.asarray(var_pose, np.float32)
    return v.mean(-1) if v.ndim == 3 else v.copy()


def kinematic(var):
    var = np.array(var, copy=True)
    for i in range(1, 24):
        var[:, i] += var[:, SMPL_PARENTS[i]]
    return var


def confident_frames(var, threshold):
    """Indices of the rows get_confident_frames keeps: accumulate, then column 0 < threshold (a NaN compares false)."""
    v = kinematic(np.asarray(var, np.float32))
    with np.errstate(invalid="ignore"):
        return np.nonzero(v[:, 0] < np.float32(threshold))[0]


def crop_to_image(boxes, kp, crop_res):
    """convert_crop_coords_to_orig_img in float32: the box side is its width."""
    boxes, kp = np.asarray(boxes, np.float32), np.asarray(kp, np.float32)
    cx, cy, h = boxes[:, 0], boxes[:, 1], boxes[:, 2]
    out = np.float32(0.5 * crop_res) * (kp + np.float32(1.0))
    out = out * (h[:, None, None] / np.float32(crop_res))
    out[:, :, 0] = (cx - h / np.float32(2))[:, None] + out[:, :, 0]
    out[:, :, 1] = (cy - h / np.float32(2))[:, None] + out[:, :, 1]
    return out


def step(pred_pose, pred_shape, var_pose, joints2d, joints3d, boxes, source_id, threshold=None, joints_in_crop=False, crop_res=224,
         dtype=np.float64):
    """The records [n_kept, RECORD_FLOATS] float32 of one call (or of the concatenation of several), kept crops in source order,
    and the flags [B].  threshold None, NaN or <= 0: every crop."""
    B = len(pred_pose)
    boxes = np.asarray(boxes, np.float32).reshape(B, 4)
    var = trailing_mean(var_pose)
    keep = np.ones(B, bool)
    if threshold is not None and threshold > 0:
        keep = np.zeros(B, bool)
        keep[confident_frames(var, threshold)] = True
    rec = np.zeros((B, RECORD_FLOATS), np.float32)
    rec[:, P_SRC] = np.asarray(source_id, np.int32).view(np.float32)
    rec[:, P_CENTER:P_CENTER + 2] = boxes[:, :2]
    rec[:, P_SCALE] = np.maximum(boxes[:, 2], boxes[:, 3]) / np.float32(200.0)
    rec[:, P_POSE:P_POSE + 72] = rotmat_to_aa(np.asarray(pred_pose, np.float32).reshape(-1, 3, 3), dtype).reshape(B, 72)
    rec[:, P_SHAPE:P_SHAPE + 10] = np.asarray(pred_shape, np.float32)
    rec[:, P_VAR:P_VAR + 24] = var
    j2 = np.asarray(joints2d, np.float32).reshape(B, 49, 2)
    if joints_in_crop:
        j2 = crop_to_image(boxes, j2, crop_res)
    kp = np.concatenate([j2, np.ones((B, 49, 1), np.float32)], -1)
    rec[:, P_OPENPOSE:P_PART] = kp[:, :25].reshape(B, 75)
    rec[:, P_PART:P_S] = kp[:, 25:].reshape(B, 72)
    rec[:, P_S:P_PAD] = np.concatenate([np.asarray(joints3d, np.float32).reshape(B, 49, 3)[:, 25:], np.ones((B, 24, 1), np.float32)],
                                       -1).reshape(B, 96)
    return rec[keep], keep                  # boolean indexing keeps the order: the stable compaction


def split(rec):
    """Records -> the named arrays of the dataset file (without imgname / person_id, which the caller maps from source_id)."""
    rec = np.asarray(rec, np.float32).reshape(-1, RECORD_FLOATS)
    n = len(rec)
    return {"source_id": rec[:, P_SRC].copy().view(np.int32), "center": rec[:, P_CENTER:P_CENTER + 2].copy(), "scale": rec[:, P_SCALE].copy(),
            "pose": rec[:, P_POSE:P_POSE + 72].copy(), "shape": rec[:, P_SHAPE:P_SHAPE + 10].copy(), "var": rec[:, P_VAR:P_VAR + 24].copy(),
            "has_smpl": np.ones(n, np.float32), "openpose": rec[:, P_OPENPOSE:P_PART].reshape(n, 25, 3).copy(),
            "part": rec[:, P_PART:P_S].reshape(n, 24, 3).copy(), "S": rec[:, P_S:P_PAD].reshape(n, 24, 4).copy()}


# ---- the seeded inputs of tests/golden/pseudo.npz (tools/gen_pseudo_golden.py) -----------------------------------------------------
CLASSES = ("rot6d", "uniform", "angle_1e-3", "angle_1e-5", "pi-1e-3", "pi-1e-5", "pi", "pi_coordinate", "identity", "branch", "zero",
           "nan")
SPECIAL = ("pi", "pi_coordinate", "identity", "zero", "nan")       # rows whose device values must equal the restatement's exactly
FIXTURE_THRESHOLD = 0.3


def _axis_angle_matrix(axis, angle):
    """exp of angle * [axis]x in float64 (Rodrigues' formula; only to make inputs)."""
    n = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    K = np.zeros(n.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -n[..., 2], n[..., 1], n[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -n[..., 0], -n[..., 1], n[..., 0]
    a = np.asarray(angle, np.float64)[..., None, None]
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def fixture_matrices(seed=20):
    """(R float32 [N,3,3], cls int32 [N] into CLASSES): every input class of the fixture, N >= 257."""
    r = np.random.default_rng(seed)
    parts = []

    def add(name, R):
        R = np.asarray(R, np.float64).reshape(-1, 3, 3).astype(np.float32)
        parts.append((R, np.full(len(R), CLASSES.index(name), np.int32)))

    x = r.standard_normal((96, 3, 2)).astype(np.float32)             # rot6d_to_rotmat's Gram-Schmidt (geometry.py:247-261), float32
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / np.maximum(np.linalg.norm(a1, axis=1, keepdims=True), np.float32(1e-12))
    u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    b2 = u / np.maximum(np.linalg.norm(u, axis=1, keepdims=True), np.float32(1e-12))
    add("rot6d", np.stack([b1, b2, np.cross(b1, b2)], -1))
    q = r.standard_normal((96, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, xq, y, z = q.T
    add("uniform", np.stack([1 - 2 * (y * y + z * z), 2 * (xq * y - w * z), 2 * (xq * z + w * y),
                             2 * (xq * y + w * z), 1 - 2 * (xq * xq + z * z), 2 * (y * z - w * xq),
                             2 * (xq * z - w * y), 2 * (y * z + w * xq), 1 - 2 * (xq * xq + y * y)], -1))
    for name, ang in (("angle_1e-3", 1e-3), ("angle_1e-5", 1e-5), ("pi-1e-3", np.pi - 1e-3), ("pi-1e-5", np.pi - 1e-5)):
        add(name, _axis_angle_matrix(r.standard_normal((16, 3)), np.full(16, ang)))
    n = r.standard_normal((16, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    add("pi", 2.0 * n[:, :, None] * n[:, None, :] - np.eye(3))       # exactly pi: symmetric to the bit
    add("pi_coordinate", [np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])])
    add("identity", np.eye(3))
    add("branch", _axis_angle_matrix(np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 1.0]]), np.array([2.5, 2.5, 2.5, 0.3])))
    add("zero", np.zeros((3, 3)))
    bad = np.eye(3)
    bad[1, 2] = np.nan
    add("nan", bad)
    R = np.concatenate([p[0] for p in parts])
    cls = np.concatenate([p[1] for p in parts])
    assert len(R) >= 257
    return R, cls


def fixture_var(seed=21, rows=64, threshold=FIXTURE_THRESHOLD):
    """var [rows,24] float32 around the threshold in column 0, one row with a NaN there and one exactly at the threshold."""
    r = np.random.default_rng(seed)
    var = r.uniform(0.05, 0.6, (rows, 24)).astype(np.float32)
    var[5, 0] = np.nan
    var[9, 0] = np.float32(threshold)
    var[11, 7] = np.nan                       # a NaN elsewhere does not decide
    return var


def step_inputs(B, T=1, seed=0):
    """Seeded inputs of one poco_pseudo_step call (numpy, float32): rotations from fixture_matrices' classes, boxes, keypoints."""
    r = np.random.default_rng(1000 + seed)
    R, _ = fixture_matrices()
    pose = R[r.integers(0, len(R), (B, 24))]
    var = r.uniform(0.05, 0.6, (B, 24) if T == 1 else (B, 24, T)).astype(np.float32)
    return {"pred_pose": np.ascontiguousarray(pose), "pred_shape": r.standard_normal((B, 10)).astype(np.float32), "var_pose": var,
            "joints2d": r.uniform(-1.2, 1.2, (B, 49, 2)).astype(np.float32), "joints3d": r.standard_normal((B, 49, 3)).astype(np.float32),
            "boxes": np.stack([r.uniform(0, 640, B), r.uniform(0, 480, B), r.uniform(20, 400, B), r.uniform(20, 400, B)], 1).astype(np.float32),
            "source_id": r.integers(-5, 1 << 30, B).astype(np.int32)}
