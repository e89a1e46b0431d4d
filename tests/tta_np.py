"""The contract of poco_op_tta_fuse (include/poco_hip.h) in float64 numpy, in plain loops: the yardstick of
tests/test_tta_*.py.  Nothing here is shared with the code under test except the joint permutation (data)."""
import math

import numpy as np

FLIP_PERM = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]
SWEEPS = 10
M3 = (1.0, -1.0, -1.0)


def view_cs(rot):
    """cos and sin of +rot degrees in float64, exact at the quarter turns.  Deliberately restated, not shared with ops.tta_view_cs: that
    the two agree says little (same logic); the independent check is the cos / sin of pi / 12 comparison in tests/test_tta_cpu.py."""
    rot = float(rot)
    if rot % 90.0 == 0.0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(rot // 90.0) % 4]
    return math.cos(math.radians(rot)), math.sin(math.radians(rot))


def unflip(R):
    """flip_pose on a rotation matrix (an involution): R[i][c] * m_i * m_c with m = (1, -1, -1)."""
    out = np.empty((3, 3))
    for i in range(3):
        for c in range(3):
            out[i, c] = R[i][c] * (M3[i] * M3[c])
    return out


def unrotate(R, c, s):
    """Rz(+rot) R: the inverse of rot_aa on the root's rotation matrix."""
    out = np.empty((3, 3))
    for col in range(3):
        out[0, col] = c * R[0][col] - s * R[1][col]
        out[1, col] = s * R[0][col] + c * R[1][col]
        out[2, col] = R[2][col]
    return out


def untransform(R, j, flip, c, s):
    """The rotation of joint j (read from the source joint by the caller) of a view back in the base frame: un-flip, then for the
    root of a rotated view un-rotate."""
    R = np.asarray(R, np.float64)
    if flip:
        R = unflip(R)
    if j == 0 and not (c == 1.0 and s == 0.0):
        R = unrotate(R, c, s)
    return R


def _rotate(a, v, p, q):
    apq = a[p][q]
    if not apq != 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    for k in range(4):
        akp, akq = a[k][p], a[k][q]
        a[k][p], a[k][q] = c * akp - s * akq, s * akp + c * akq
    for k in range(4):
        apk, aqk = a[p][k], a[q][k]
        a[p][k], a[q][k] = c * apk - s * aqk, s * apk + c * aqk
    for k in range(4):
        vkp, vkq = v[k][p], v[k][q]
        v[k][p], v[k][q] = c * vkp - s * vkq, s * vkp + c * vkq


def project(M):
    """argmax over SO(3) of tr(R^T M): the unit quaternion that maximises q^T N q (Horn 1987), N's largest eigenvector by cyclic
    Jacobi with a fixed number of sweeps."""
    M = np.asarray(M, np.float64)
    k = [[float(M[c][r]) for c in range(3)] for r in range(3)]                # K = M^T (Python floats: IEEE overflow to inf, no warning)
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = k[0][0] + k[1][1] + k[2][2]
    N[1][1] = k[0][0] - k[1][1] - k[2][2]
    N[2][2] = -k[0][0] + k[1][1] - k[2][2]
    N[3][3] = -k[0][0] - k[1][1] + k[2][2]
    N[0][1] = N[1][0] = k[1][2] - k[2][1]
    N[0][2] = N[2][0] = k[2][0] - k[0][2]
    N[0][3] = N[3][0] = k[0][1] - k[1][0]
    N[1][2] = N[2][1] = k[0][1] + k[1][0]
    N[1][3] = N[3][1] = k[2][0] + k[0][2]
    N[2][3] = N[3][2] = k[1][2] + k[2][1]
    E = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rotate(N, E, p, q)
    best, col = N[0][0], 0
    for i in range(1, 4):
        if N[i][i] > best:
            best, col = N[i][i], i
    qw, qx, qy, qz = E[0][col], E[1][col], E[2][col], E[3][col]
    qn = math.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
    return np.array([[qw * qw + qx * qx - qy * qy - qz * qz, 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
                     [2.0 * (qx * qy + qw * qz), qw * qw - qx * qx + qy * qy - qz * qz, 2.0 * (qy * qz - qw * qx)],
                     [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), qw * qw - qx * qx - qy * qy + qz * qz]])


def project_svd(M):
    """The same projection through the SVD: U diag(1, 1, det(U V^T)) V^T."""
    U, _, Vt = np.linalg.svd(np.asarray(M, np.float64))
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def fuse(pose, var, betas, views, weight):
    """pose [K*B,24,3,3], var [K*B,24], betas [K*B,10] (float32 as the device holds them), views = [(flip, rot degrees), ...],
    weight 0 = uniform | 1 = uncertainty -> dict of float64 arrays pose [B,24,3,3], var [B,24], spread [B,24], betas [B,10] before
    their one rounding to fp32, W [B,24] and dropped [K,B,24]."""
    K = len(views)
    pose = np.asarray(pose).reshape(K, -1, 24, 3, 3)
    B = pose.shape[1]
    var, betas = np.asarray(var).reshape(K, B, 24), np.asarray(betas).reshape(K, B, 10)
    cs = [view_cs(r) for _, r in views]
    out = dict(pose=np.zeros((B, 24, 3, 3)), var=np.zeros((B, 24)), spread=np.zeros((B, 24)), betas=np.zeros((B, 10)), W=np.zeros((B, 24)),
               dropped=np.zeros((K, B, 24), bool))
    for b in range(B):
        for j in range(24):
            Rs, vs, ws = [], [], []
            for k in range(K):
                flip = int(views[k][0])
                js = FLIP_PERM[j] if flip else j
                raw = pose[k, b, js].astype(np.float64)
                v = float(var[k, b, js])
                ok = math.isfinite(v) and v >= 0.0 and bool(np.isfinite(raw).all())
                w = 0.0
                if ok:
                    w = 1.0 / (v + 1e-9) if weight else 1.0
                out["dropped"][k, b, j] = not ok
                Rs.append(untransform(raw, j, flip, *cs[k]) if ok else None)
                vs.append(v)
                ws.append(w)
            M, W, SV = np.zeros((3, 3)), 0.0, 0.0
            for k in range(K):
                if ws[k] > 0.0:
                    M = M + ws[k] * Rs[k]
                    W = W + ws[k]
                    SV = SV + ws[k] * vs[k]
            out["W"][b, j] = W
            if not W > 0.0:
                out["pose"][b, j], out["var"][b, j], out["spread"][b, j] = pose[0, b, j], var[0, b, j], np.nan
                if j == 0:
                    out["betas"][b] = betas[0, b]
                continue
            Rp = project(M)
            acc = 0.0
            for k in range(K):
                if ws[k] > 0.0:
                    d = 0.0
                    for i in range(3):
                        for c in range(3):
                            df = Rs[k][i, c] - Rp[i, c]
                            d = d + df * df
                    acc = acc + ws[k] * (d / 9.0)
            out["pose"][b, j], out["var"][b, j], out["spread"][b, j] = Rp, SV / W, acc / W
            if j == 0:
                for i in range(10):
                    s = 0.0
                    for k in range(K):
                        if ws[k] > 0.0:
                            s = s + ws[k] * float(betas[k, b, i])
                    out["betas"][b, i] = s / W
    return out
