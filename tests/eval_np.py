"""The evaluation contract of include/poco_hip.h ("evaluator") restated in numpy: the yardstick of tests/test_eval_*.py and the
host path tools/bench_eval.py times.  dtype = np.float32 mirrors the reference (its numpy / torch path is float32 there),
np.float64 is the yardstick.  Each function cites the reference lines it restates; none of their text is copied.

    joints_from_mesh   eval_utils.py:62-75, base_dataset.py:359-365
    mpjpe              eval_utils.py:99-102
    procrustes, pampjpe  eval_utils.py:11-59, 77-97
    v2v                eval_utils.py:104-118
    rodrigues          geometry.py:207-244
    pose_distance      eval_utils.py:154-160
    processed_uncert   poco_utils.py:21-25, 62-94
    pearson            eval_utils.py:162-165 (scipy.stats.pearsonr), centred
"""
import numpy as np

from poco_amd.synth import SMPL_PARENTS

H36M_TO_J17 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10, 0, 7, 9]      # constants.py:95
H36M_TO_J14 = H36M_TO_J17[:14]                                               # constants.py:96
MAX_JOINTS = 32
RECORD_FLOATS = 416
# record offsets (include/poco_hip.h)
R_MPJPE, R_PA, R_V2V, R_MPJPE_J, R_PA_J, R_POSE, R_UNC, R_PRED, R_GT, R_NONREL = 0, 1, 2, 4, 36, 68, 92, 116, 212, 308


def joint_map(dataset_name: str):
    """eval_utils.py:65: 17 joints for mpi-inf-3dhp, 14 otherwise."""
    return H36M_TO_J17 if dataset_name == "mpi-inf-3dhp" else H36M_TO_J14


def joints_from_mesh(verts, J_regressor, jmap, pelvis=0, dtype=np.float64):
    """verts [B,V,3], J_regressor [J,V] -> (pelvis-relative [B,M,3], not relative [B,M,3])."""
    j = np.matmul(np.asarray(J_regressor, dtype)[None], np.asarray(verts, dtype))
    pel = j[:, [pelvis], :].copy()
    nonrel = j[:, list(jmap), :]
    return nonrel - pel, nonrel.copy()


def mpjpe(pred, gt, dtype=np.float64):
    """-> (per joint [B,M], mean [B])."""
    e = np.sqrt(((np.asarray(pred, dtype) - np.asarray(gt, dtype)) ** 2).sum(-1))
    return e, e.mean(-1)


def procrustes_parts(S1, S2, dtype=np.float64):
    """One crop, S1 / S2 [M,3]: (mu1, mu2, var1, K = X1 X2^T, U, s, Vh) of eval_utils.py:25-40."""
    A, G = np.asarray(S1, dtype).T, np.asarray(S2, dtype).T                  # 3 x M
    mu1, mu2 = A.mean(1, keepdims=True), G.mean(1, keepdims=True)
    X1, X2 = A - mu1, G - mu2
    var1 = np.sum(X1 ** 2)
    K = X1.dot(X2.T)
    U, s, Vh = np.linalg.svd(K)
    return A, mu1, mu2, var1, K, U, s, Vh


def procrustes(S1, S2, dtype=np.float64, sign_fix=True):
    """S1 aligned onto S2 by the best similarity transform, one crop [M,3].  sign_fix=False leaves out the Z correction (a
    reflection is then allowed): only for the non-vacuity test."""
    A, mu1, mu2, var1, K, U, s, Vh = procrustes_parts(S1, S2, dtype)
    V = Vh.T
    Z = np.eye(3, dtype=dtype)
    if sign_fix:
        Z[2, 2] *= np.sign(np.linalg.det(U.dot(V.T)))
    R = V.dot(Z.dot(U.T))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.trace(R.dot(K)) / var1
        t = mu2 - scale * R.dot(mu1)
        return (scale * R.dot(A) + t).T


def conditioning(S1, S2):
    """(smallest (sigma2 +- sigma3) / sigma1 of K, det(U V^T)) in float64: how far the crop is from the ill-conditioned case, and
    whether the Z fix fires (det < 0)."""
    _, _, _, _, K, U, s, Vh = procrustes_parts(S1, S2, np.float64)
    return float((s[1] - s[2]) / s[0]), float(np.linalg.det(U.dot(Vh)))


def pampjpe(pred, gt, dtype=np.float64, sign_fix=True):
    """-> (per joint [B,M], mean [B])."""
    pred, gt = np.asarray(pred, dtype), np.asarray(gt, dtype)
    hat = np.stack([procrustes(pred[i], gt[i], dtype, sign_fix) for i in range(pred.shape[0])])
    e = np.sqrt(((hat - gt) ** 2).sum(-1))
    return e, e.mean(-1)


def v2v(pred_verts, gt_verts=None, dtype=np.float64):
    if gt_verts is None:
        return np.zeros(len(pred_verts), dtype)
    return np.sqrt(((np.asarray(gt_verts, dtype) - np.asarray(pred_verts, dtype)) ** 2).sum(-1)).mean(-1)


def rodrigues(aa, dtype=np.float64):
    """aa [N,3] -> [N,3,3]: norm of theta + 1e-8, quaternion (cos(a/2), sin(a/2) theta / a), renormalised, expanded."""
    th = np.asarray(aa, dtype).reshape(-1, 3)
    angle = np.sqrt(((th + dtype(1e-8)) ** 2).sum(1, keepdims=True))
    n = th / angle
    half = angle * dtype(0.5)
    q = np.concatenate([np.cos(half), np.sin(half) * n], 1)
    q = q / np.sqrt((q ** 2).sum(1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    R = np.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                  2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                  2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], 1)
    return R.reshape(-1, 3, 3).astype(dtype)


def pose_distance(pred_pose, gt_pose_aa, dtype=np.float64):
    """pred_pose [B,24,3,3], gt_pose_aa [B,72] -> [B,24]."""
    g = rodrigues(np.asarray(gt_pose_aa).reshape(-1, 3), dtype).reshape(-1, 24, 3, 3)
    return ((np.asarray(pred_pose, dtype) - g) ** 2).mean(-1).mean(-1)


def processed_uncert(var, kinematic=True, dtype=np.float32):
    """var [B,24] / [B,24,a] / [B,24,a,b] -> [B,24]."""
    v = np.asarray(var, dtype)
    if v.ndim == 4:
        v = v.mean(-1).mean(-1)
    elif v.ndim == 3:
        v = v.mean(-1)
    v = v.copy()
    if kinematic:
        for i in range(1, 24):
            v[:, i] += v[:, SMPL_PARENTS[i]]
    return v


def pearson(x, y):
    """float64, centred: means first, then the three centred sums; clipped to [-1, 1] as scipy does."""
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    xm, ym = x - x.mean(), y - y.mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (xm * ym).sum() / (np.sqrt((xm * xm).sum()) * np.sqrt((ym * ym).sum()))
    return float(np.clip(r, -1.0, 1.0)) if np.isfinite(r) else float(r)


def evaluate(pred_vertices, pred_pose, var_pose, gt_pose, J_regressor, jmap, gt_vertices=None, gt_joints=None, pelvis=0,
             kinematic=True, dtype=np.float64, sign_fix=True):
    """Everything a step computes for B crops, as a dict of arrays (names of SaveResults.evaluation_results where it has one)."""
    assert (gt_vertices is None) != (gt_joints is None)
    pj, pj_nonrel = joints_from_mesh(pred_vertices, J_regressor, jmap, pelvis, dtype)
    gj = joints_from_mesh(gt_vertices, J_regressor, jmap, pelvis, dtype)[0] if gt_vertices is not None else np.asarray(gt_joints, dtype)
    e, em = mpjpe(pj, gj, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        r, rm = pampjpe(pj, gj, dtype, sign_fix)
    return {"mpjpe": e, "mpjpe_mean": em, "pampjpe": r, "pampjpe_mean": rm, "v2v": v2v(pred_vertices, gt_vertices, dtype),
            "corr_x": pose_distance(pred_pose, gt_pose, dtype), "corr_y": processed_uncert(var_pose, kinematic, np.float32 if dtype == np.float32 else np.float64),
            "pred_jnts3D": pj, "gt_jnts3D": gj, "pred_jnts3D_nonrel": pj_nonrel}


FIXTURE_CROPS = 16
FIXTURE_MIRRORED = (2, 5, 9, 14)            # crops whose prediction is a mirror image: det(U V^T) < 0, the Z fix fires
FIXTURE_COMBOS = [("verts", "3dpw"), ("verts", "mpi-inf-3dhp"), ("joints", "3dpw"), ("joints", "mpi-inf-3dhp")]


def _rand_rot(r, max_angle):
    ax = r.standard_normal(3)
    ax /= np.linalg.norm(ax)
    return rodrigues((ax * r.uniform(0.1, max_angle))[None], np.float64)[0]


def fixture_inputs(seed: int = 2024):
    """The inputs tests/golden/eval.npz was made from, re-derived from seeds (the file stores only expected outputs):
    ground-truth meshes = synth_smpl's template + per-vertex noise; predictions = a rigid + scale + noise perturbation of them
    (a mirror image first for FIXTURE_MIRRORED); axis-angle poses with angles up to pi; var_pose.  float32, as the engine's."""
    from poco_amd import synth
    r = np.random.default_rng(seed)
    B = FIXTURE_CROPS
    tmpl = synth.synth_smpl(7)["v_template"].astype(np.float64)
    J = synth.synth_j_regressor_h36m(11, tmpl.shape[0])
    gt_v = tmpl[None] + 0.03 * r.standard_normal((B,) + tmpl.shape)
    pred_v = np.empty_like(gt_v)
    for b in range(B):
        src = gt_v[b] * np.array([-1.0, 1.0, 1.0]) if b in FIXTURE_MIRRORED else gt_v[b]
        pred_v[b] = r.uniform(0.9, 1.1) * src @ _rand_rot(r, 0.6).T + r.uniform(-0.05, 0.05, 3) + 0.01 * r.standard_normal(tmpl.shape)
    gt_v32, pred_v32 = gt_v.astype(np.float32), pred_v.astype(np.float32)
    gt_j = {}
    for name in ("3dpw", "mpi-inf-3dhp"):
        jm = joint_map(name)
        j = joints_from_mesh(gt_v32, J, jm, 0, np.float64)[0]
        gt_j[name] = (j + 0.01 * r.standard_normal(j.shape)).astype(np.float32)
    ax = r.standard_normal((B, 24, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    gt_pose = (ax * r.uniform(0.0, np.pi, (B, 24, 1))).reshape(B, 72).astype(np.float32)
    pert = gt_pose.astype(np.float64) + 0.2 * r.standard_normal((B, 72))
    pred_pose = rodrigues(pert.reshape(-1, 3), np.float64).reshape(B, 24, 3, 3).astype(np.float32)
    var_pose = r.uniform(0.01, 0.3, (B, 24)).astype(np.float32)
    # poco_op_rodrigues: generic vectors, the zero vector, tiny angles and angles within 1e-3 .. 1e-6 of pi
    rod = r.standard_normal((64, 3))
    rod /= np.linalg.norm(rod, axis=-1, keepdims=True)
    ang = r.uniform(0.0, np.pi, 64)
    ang[:8] = [0.0, 1e-6, 1e-3, np.pi - 1e-3, np.pi - 1e-4, np.pi - 1e-5, np.pi - 1e-6, np.pi]
    rod_aa = (rod * ang[:, None]).astype(np.float32)
    return {"J_regressor": J, "gt_vertices": gt_v32, "pred_vertices": pred_v32, "gt_joints": gt_j, "gt_pose": gt_pose,
            "pred_pose": pred_pose, "var_pose": var_pose, "rod_aa": rod_aa}


def fixture_case(inp, form, dataset_name):
    """keyword arguments of evaluate() for one (ground-truth form, joint map) combination of the fixture."""
    kw = dict(pred_vertices=inp["pred_vertices"], pred_pose=inp["pred_pose"], var_pose=inp["var_pose"], gt_pose=inp["gt_pose"],
              J_regressor=inp["J_regressor"], jmap=joint_map(dataset_name))
    if form == "verts":
        kw["gt_vertices"] = inp["gt_vertices"]
    else:
        kw["gt_joints"] = inp["gt_joints"][dataset_name]
    return kw


FIELDS = {"mpjpe_mean": (R_MPJPE, 1), "pampjpe_mean": (R_PA, 1), "v2v": (R_V2V, 1), "mpjpe": (R_MPJPE_J, 1), "pampjpe": (R_PA_J, 1),
          "corr_x": (R_POSE, 1), "corr_y": (R_UNC, 1), "pred_jnts3D": (R_PRED, 3), "gt_jnts3D": (R_GT, 3),
          "pred_jnts3D_nonrel": (R_NONREL, 3)}


def unpack(records, M):
    """[N,416] records -> the dict of evaluate()."""
    rec = np.asarray(records)
    out = {}
    for k, (o, w) in FIELDS.items():
        if k in ("mpjpe_mean", "pampjpe_mean", "v2v"):
            out[k] = rec[:, o]
        elif k in ("corr_x", "corr_y"):
            out[k] = rec[:, o:o + 24]
        elif w == 1:
            out[k] = rec[:, o:o + M]
        else:
            out[k] = rec[:, o:o + 3 * MAX_JOINTS].reshape(-1, MAX_JOINTS, 3)[:, :M]
    return out


def summary(records, sel=None):
    """The five numbers of finish over [N,416] records, float64: (N, mpjpe mm, pampjpe mm, v2v mm, corr)."""
    rec = np.asarray(records, np.float64)
    sel = list(range(24)) if sel is None else list(sel)
    x = rec[:, R_POSE:R_POSE + 24][:, sel]
    y = rec[:, R_UNC:R_UNC + 24][:, sel]
    return (rec.shape[0], 1000.0 * rec[:, R_MPJPE].mean(), 1000.0 * rec[:, R_PA].mean(), 1000.0 * rec[:, R_V2V].mean(),
            pearson(x, y))
