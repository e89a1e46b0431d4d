"""The uncertainty-weighted track smoother (demo.py --mode video --smooth_uncert, poco_op_track_smooth) restated in float64 numpy:
the contract of DESIGN.md section 28 in executable form and the yardstick of tests/test_usmooth_*.py.  There is no counterpart in
the reference's code.

The route differs from the kernel's on purpose: D and A = diag(w) + lam D^T Omega D are built as DENSE T x T matrices and solved
with np.linalg.solve (LU with pivoting), where the kernel forms the five bands and factors them as L D L^T.  The projection onto
SO(3) is tests/tta_np.py's `project` (Horn's quaternion, cyclic Jacobi, 10 sweeps), stated here once more over a batch of matrices
with the same operations in the same order (tests/test_usmooth_cpu.py holds the two equal bit for bit).

Inputs, concatenated over the P tracks of a clip (N rows): offsets int32 [P+1], frames int32 [N] (strictly increasing within a
track, holes allowed), pose fp32 [N,24,3,3], u fp32 [N,24], lin fp32 [N,L], lam, u_ref, max_gap >= 1."""
import numpy as np

from tests import infill_np, tta_np

NJ = 24
W_MIN, W_MAX, U_MIN = 1e-6, 1e6, 1e-6
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 130)                 # the tracks of the GPU test, one ragged buffer
GAPS = (1, 1, 1, 2, 3, 40)
MAX_GAP = 30


def weights(u, u_ref) -> np.ndarray:
    """clamp((u_ref / max(u, 1e-6))^2, 1e-6, 1e6); a NaN or an infinity of either sign gives 1e-6."""
    u = np.asarray(u, np.float32).astype(np.float64)
    fin = np.isfinite(u)
    r = np.float64(u_ref) / np.maximum(np.where(fin, u, 1.0), U_MIN)
    return np.where(fin, np.clip(r * r, W_MIN, W_MAX), W_MIN)


def penalty(frames, max_gap):
    """D [T,T] (rows 0 and T-1 and every row next to a hole wider than max_gap are zero) and omega [T]."""
    f = np.asarray(frames).astype(np.int64)
    T = len(f)
    D, om = np.zeros((T, T)), np.zeros(T)
    for t in range(1, T - 1):
        h1, h2 = int(f[t] - f[t - 1]), int(f[t + 1] - f[t])
        if 1 <= h1 <= max_gap and 1 <= h2 <= max_gap:
            h1, h2 = float(h1), float(h2)
            D[t, t - 1], D[t, t], D[t, t + 1] = 2.0 / (h1 * (h1 + h2)), -2.0 / (h1 * h2), 2.0 / (h2 * (h1 + h2))
            om[t] = (h1 + h2) / 2.0
    return D, om


def system(w, D, om, lam) -> np.ndarray:
    """A = diag(w) + lam D^T Omega D, dense."""
    return np.diag(w) + float(lam) * (D.T @ (om[:, None] * D))


def solve_banded_ldl(w, D, om, lam, Y) -> np.ndarray:
    """The same system by the plain banded route: the three bands of A, L D L^T without pivoting, forward and backward
    substitution.  Y [T,C].  (The CPU test holds this against the dense solve; the benchmark times it as the host form.)"""
    A = system(w, D, om, lam)
    T = len(w)
    Y = np.asarray(Y, np.float64)
    d, l1, l2 = np.zeros(T), np.zeros(T), np.zeros(T)
    z = np.zeros_like(Y)
    for i in range(T):
        d[i] = A[i, i] - (l1[i - 1] ** 2 * d[i - 1] if i >= 1 else 0.0) - (l2[i - 2] ** 2 * d[i - 2] if i >= 2 else 0.0)
        if i + 1 < T:
            l1[i] = (A[i + 1, i] - (l1[i - 1] * l2[i - 1] * d[i - 1] if i >= 1 else 0.0)) / d[i]
        if i + 2 < T:
            l2[i] = A[i + 2, i] / d[i]
        z[i] = w[i] * Y[i] - (l1[i - 1] * z[i - 1] if i >= 1 else 0.0) - (l2[i - 2] * z[i - 2] if i >= 2 else 0.0)
    x = np.zeros_like(Y)
    for i in range(T - 1, -1, -1):
        x[i] = z[i] / d[i] - (l1[i] * x[i + 1] if i + 1 < T else 0.0) - (l2[i] * x[i + 2] if i + 2 < T else 0.0)
    return x


def _rotate(a, v, p, q):
    """tta_np._rotate over a batch: a, v [n,4,4]."""
    apq = a[:, p, q].copy()
    go = apq != 0.0                                        # False for zero and NaN: the entry is left alone
    with np.errstate(all="ignore"):
        theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
    c, s = np.where(go, c, 1.0), np.where(go, s, 0.0)      # the identity rotation: c * x - 0 * y = x exactly
    for k in range(4):
        akp, akq = a[:, k, p].copy(), a[:, k, q].copy()
        a[:, k, p], a[:, k, q] = c * akp - s * akq, s * akp + c * akq
    for k in range(4):
        apk, aqk = a[:, p, k].copy(), a[:, q, k].copy()
        a[:, p, k], a[:, q, k] = c * apk - s * aqk, s * apk + c * aqk
    for k in range(4):
        vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
        v[:, k, p], v[:, k, q] = c * vkp - s * vkq, s * vkp + c * vkq


def project_batch(M) -> np.ndarray:
    """tta_np.project over M [n,3,3]."""
    M = np.asarray(M, np.float64)
    n = M.shape[0]
    k = M.transpose(0, 2, 1)                               # K = M^T
    N = np.zeros((n, 4, 4))
    N[:, 0, 0] = k[:, 0, 0] + k[:, 1, 1] + k[:, 2, 2]
    N[:, 1, 1] = k[:, 0, 0] - k[:, 1, 1] - k[:, 2, 2]
    N[:, 2, 2] = -k[:, 0, 0] + k[:, 1, 1] - k[:, 2, 2]
    N[:, 3, 3] = -k[:, 0, 0] - k[:, 1, 1] + k[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = k[:, 1, 2] - k[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = k[:, 2, 0] - k[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = k[:, 0, 1] - k[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = k[:, 0, 1] + k[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = k[:, 2, 0] + k[:, 0, 2]
    N[:, 2, 3] = N[:, 3, 2] = k[:, 1, 2] + k[:, 2, 1]
    E = np.tile(np.eye(4), (n, 1, 1))
    for _ in range(tta_np.SWEEPS):
        for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            _rotate(N, E, p, q)
    best, col = N[:, 0, 0].copy(), np.zeros(n, np.int64)
    for i in range(1, 4):
        better = N[:, i, i] > best
        best, col = np.where(better, N[:, i, i], best), np.where(better, i, col)
    q = E[np.arange(n), :, col]
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    qn = np.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
    qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
    R = np.empty((n, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = qw * qw + qx * qx - qy * qy - qz * qz, 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2.0 * (qx * qy + qw * qz), qw * qw - qx * qx + qy * qy - qz * qz, 2.0 * (qy * qz - qw * qx)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), qw * qw - qx * qx - qy * qy + qz * qz
    return R


def shift_deg(A, R) -> np.ndarray:
    """The angle of Q = A^T R in degrees over a batch [n,3,3]: atan2(|skew(Q)| / 2, (trace(Q) - 1) / 2)."""
    Q = np.asarray(A, np.float64).transpose(0, 2, 1) @ np.asarray(R, np.float64)
    sx, sy, sz = Q[:, 2, 1] - Q[:, 1, 2], Q[:, 0, 2] - Q[:, 2, 0], Q[:, 1, 0] - Q[:, 0, 1]
    sn = 0.5 * np.sqrt(sx * sx + sy * sy + sz * sz)
    cs = 0.5 * (Q[:, 0, 0] + Q[:, 1, 1] + Q[:, 2, 2] - 1.0)
    return np.degrees(np.arctan2(sn, cs))


def smooth(pose, u, frames, offsets, lin, lam, u_ref, max_gap, solver=None) -> dict:
    """-> float64 arrays before their one rounding: pose64 [N,24,3,3], lin64 [N,L], shift64 [N,24], solved64 [N,24,3,3] (before
    the projection), and pose / lin / shift, their float32 roundings.  solver(w, D, om, lam, Y): another route to A X = diag(w) Y."""
    pose, u, lin = np.asarray(pose, np.float32), np.asarray(u, np.float32), np.asarray(lin, np.float32)
    N, L = pose.shape[0], lin.shape[1]
    solved, lin64 = np.zeros((N, NJ, 3, 3)), np.zeros((N, L))
    for p in range(len(offsets) - 1):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        D, om = penalty(frames[lo:hi], max_gap)
        for j in range(NJ):
            w = weights(u[lo:hi, j], u_ref)
            Y = pose[lo:hi, j].reshape(hi - lo, 9).astype(np.float64)
            if j == 0 and L:
                Y = np.concatenate([Y, lin[lo:hi].astype(np.float64)], 1)
            X = solver(w, D, om, lam, Y) if solver else np.linalg.solve(system(w, D, om, lam), w[:, None] * Y)
            solved[lo:hi, j] = X[:, :9].reshape(hi - lo, 3, 3)
            if j == 0 and L:
                lin64[lo:hi] = X[:, 9:]
    pose64 = project_batch(solved.reshape(-1, 3, 3)).reshape(N, NJ, 3, 3)
    shift64 = shift_deg(pose.reshape(-1, 3, 3), pose64.reshape(-1, 3, 3)).reshape(N, NJ)
    return dict(pose64=pose64, lin64=lin64, shift64=shift64, solved64=solved, pose=pose64.astype(np.float32),
                lin=lin64.astype(np.float32), shift=shift64.astype(np.float32))


def gpu_case(seed=28, L=14) -> dict:
    """The material of tests/test_usmooth_gpu.py: tracks of LENGTHS rows in one buffer; slowly turning joints with a degree or two
    of jitter on top; u in [0.05, 3] with a few NaN and +Inf; frame gaps drawn from GAPS (40 exceeds MAX_GAP: a hole)."""
    r = np.random.default_rng(seed)
    poses, us, frs, lins = [], [], [], []
    for T in LENGTHS:
        base = infill_np.smooth_rotations(r, T, 3.0).astype(np.float64)
        jit = np.stack([infill_np.rot_axis(r.standard_normal(3), np.deg2rad(r.uniform(0.0, 4.0))) for _ in range(T * NJ)])
        poses.append((base.reshape(-1, 3, 3) @ jit).reshape(T, NJ, 3, 3).astype(np.float32))
        u = r.uniform(0.05, 3.0, (T, NJ)).astype(np.float32)
        bad = r.random((T, NJ))
        u[bad < 0.02] = np.nan
        u[bad > 0.98] = np.inf
        us.append(u)
        frs.append(int(r.integers(0, 1000)) + np.cumsum(r.choice(GAPS, T)))
        lins.append(r.standard_normal((T, L)).astype(np.float32))
    return dict(pose=np.concatenate(poses), u=np.concatenate(us), frames=np.concatenate(frs).astype(np.int32),
                offsets=np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32), lin=np.concatenate(lins))
