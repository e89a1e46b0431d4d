"""Choosing between two regressors by their own per-joint uncertainty (demo.py / eval.py --cfg2 --ckpt2 --select,
poco_op_select_regressor) restated in float64 numpy with plain loops.  This file IS the contract (include/poco_hip.h, DESIGN.md
section 25) and imports nothing of the project.  Everything the operator does is a decision plus copies, so every comparison with
it is bit for bit."""
import numpy as np

PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)       # SMPL's kinematic tree
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def processed(var_row, kinematic):
    """u[j] = var[j]; with kinematic u[child] = var[child] + u[parent] in child order 1..23, fp32 additions (poco_utils.py:21-25)."""
    u = [np.float32(v) for v in var_row]
    if kinematic:
        with np.errstate(all="ignore"):
            for c in range(1, 24):
                u[c] = np.float32(u[c] + u[PARENTS[c]])
    return u


def crop_score(u, kind, thr):
    """poco_utils.py:50-60 on one row, float64 from the fp32 u: kind 1 the root against 2 thr, kind 0 the mean in joint order
    against thr; a row over its threshold scores exactly 1."""
    root = float(u[0])
    if kind == 1:
        return 1.0 if root > 2.0 * thr else root
    if root > thr:
        return 1.0
    s = 0.0
    for j in range(24):
        s = s + float(u[j])
    return s / 24.0


def _f32(s):
    """A score rounded once; a NaN is the one quiet NaN 0x7fc00000."""
    with np.errstate(all="ignore"):
        return QNAN if s != s else np.float32(s)


def select(pose0, var0, kind0, pose1, var1, kind1, kinematic, thr, scale, mode, payloads=()):
    """pose_m [B,24,3,3], var_m [B,24] float32; payloads = [(src0, src1), ...] of [B, ...] float32 arrays; mode 0 crop | 1 joint.
    -> dict(pose, var, choice uint8 [B,24], score float32 [B,2], mixed uint8 [B], rows = the mixed rows in order (int32),
    payloads = [dst, ...], u = the two processed uncertainties [2,B,24] float32)."""
    B = len(pose0)
    thr, scale = float(thr), float(scale)
    pose, var = np.empty((B, 24, 3, 3), np.float32), np.empty((B, 24), np.float32)
    choice, score, mixed = np.zeros((B, 24), np.uint8), np.empty((B, 2), np.float32), np.zeros(B, np.uint8)
    uu = np.empty((2, B, 24), np.float32)
    dst = [np.empty_like(a) for a, _ in payloads]
    rows = []
    for t in range(B):
        u0, u1 = processed(var0[t], kinematic), processed(var1[t], kinematic)
        uu[0, t], uu[1, t] = u0, u1
        s0 = crop_score(u0, kind0, thr)
        s1 = scale * crop_score(u1, kind1, thr)
        score[t, 0], score[t, 1] = _f32(s0), _f32(s1)
        for j in range(24):
            if mode == 0:
                one = s1 < s0                                    # false for a tie and for a NaN on either side: model 0
            else:
                one = scale * float(u1[j]) < float(u0[j])
            choice[t, j] = 1 if one else 0
            src_p, src_v = (pose1, var1) if one else (pose0, var0)
            pose[t, j].view(np.uint32)[...] = src_p[t, j].view(np.uint32)
            var[t:t + 1, j].view(np.uint32)[...] = src_v[t:t + 1, j].view(np.uint32)
        if len(set(int(c) for c in choice[t])) > 1:
            mixed[t] = 1
            rows.append(t)
        for k, (a, b) in enumerate(payloads):                    # every payload row follows the root
            src = b if choice[t, 0] else a
            dst[k][t:t + 1].view(np.uint32)[...] = src[t:t + 1].view(np.uint32)
    return {"pose": pose, "var": var, "choice": choice, "score": score, "mixed": mixed, "rows": np.asarray(rows, np.int32),
            "payloads": dst, "u": uu}
