"""The keypoint refit (demo.py --mode video --kp_refit, eval.py --kp_refit, poco_op_kp_refit) restated in numpy with plain loops:
the contract of DESIGN.md section 31 in executable form and the yardstick of tests/test_refit_*.py.  There is no counterpart in the
reference's code (its smplify_runner is VIBE's TemporalSMPLify, which is not in its tree).

It is written from the contract, not from the kernel, and the route differs where the contract leaves it open: the Jacobian is a
dense [2K,75] matrix, the normal matrix is the dense J^T W J, and the system is solved with numpy.linalg.cholesky and two
triangular solves (the kernel keeps a packed triangle and factors it root-free).  `ft` chooses the arithmetic: numpy.float64 is
the yardstick, numpy.longdouble (with a plain-loop Cholesky, numpy.linalg has none for it) measures the yardstick's own rounding -
the tolerance of tests/test_refit_gpu.py.

Per row: pose fp32 [24,3,3], u fp32 [24], jrest fp32 [24,3], kp fp32 [K,3] (x, y, confidence), cam fp32 [5] = (a, tx, ty, px, py),
norm fp32; kp_joint int [K] (-1 = not observed), parents int [24]."""
import numpy as np

NJ = 24
NU = 75                                                    # 24 x 3 rotation unknowns, then kappa, dtx, dty
W_MIN, W_MAX, U_MIN = 1e-6, 1e6, 1e-6
MU0, MU_MIN, MU_MAX = 1e-3, 1e-12, 1e12
SMPL_PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], np.int32)
# BODY_25: Nose Neck RShoulder RElbow RWrist LShoulder LElbow LWrist MidHip RHip RKnee RAnkle LHip LKnee LAnkle, then eyes, ears, feet
BODY25_TO_SMPL = np.array([-1, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7] + [-1] * 10, np.int32)
DEFAULTS = dict(lam=0.1, u_ref=0.3, rho=0.1, cam_prior=1.0, conf_thresh=0.3, min_kp=4, iters=10)


def hat(v, ft=np.float64):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], ft)


def exp_so3(d, ft=np.float64):
    """Rodrigues: I + A K + B K^2, A = sin(t) / t, B = (1 - cos(t)) / t^2; below t = 1e-8 their series 1 - t^2/6 and 1/2 - t^2/24."""
    d = np.asarray(d, ft)
    t2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    t = np.sqrt(t2)
    if t < 1e-8:
        A, B = ft(1) - t2 / ft(6), ft(0.5) - t2 / ft(24)
    else:
        A, B = np.sin(t) / t, (ft(1) - np.cos(t)) / t2
    K = hat(d, ft)
    return np.eye(3, dtype=ft) + A * K + B * (K @ K)


def log_so3(Q, ft=np.float64):
    """The rotation vector of Q: s = skew(Q) / 2 = (Q21 - Q12, Q02 - Q20, Q10 - Q01) / 2, angle atan2(|s|, (trace - 1) / 2), vector
    s * angle / |s|; |s| < 1e-8 gives s itself (near the identity that is the series' first term; a half turn has no unique
    vector and the refit, which starts at the identity of this map, does not get there)."""
    s = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]], ft) * ft(0.5)
    sn = np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    cs = ft(0.5) * (Q[0, 0] + Q[1, 1] + Q[2, 2] - ft(1))
    if sn < 1e-8:
        return s
    return s * (np.arctan2(sn, cs) / sn)


def angle_deg(A, R, ft=np.float64):
    """poco_op_track_smooth's shift: the angle of A^T R in degrees."""
    Q = A.T @ R
    s = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]], ft)
    sn = ft(0.5) * np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
    cs = ft(0.5) * (Q[0, 0] + Q[1, 1] + Q[2, 2] - ft(1))
    return np.arctan2(sn, cs) * (ft(180) / ft(np.pi) if ft is np.float64 else ft(180) / np.arctan2(ft(0), ft(-1)))


def weights(u, lam, u_ref, ft=np.float64):
    """w_j = lam * clamp((u_ref / max(u_j, 1e-6))^2, 1e-6, 1e6); a NaN or an infinity of either sign gives lam * 1e-6."""
    w = np.empty(NJ, ft)
    for j in range(NJ):
        uj = np.float32(u[j])
        if not np.isfinite(uj):
            w[j] = ft(lam) * ft(W_MIN)
        else:
            r = ft(u_ref) / max(ft(uj), ft(U_MIN))
            w[j] = ft(lam) * min(max(r * r, ft(W_MIN)), ft(W_MAX))
    return w


def ancestors(parents, j):
    """The proper ancestors of joint j, nearest first: the joints whose rotation moves p_j."""
    out = []
    j = int(parents[j])
    while j >= 0:
        out.append(j)
        j = int(parents[j]) if j > 0 else -1
    return out


def forward_kinematics(R, jrest, parents, ft=np.float64):
    """G_0 = R_0, p_0 = J_0; G_j = G_parent R_j, p_j = p_parent + G_parent (J_j - J_parent)."""
    G, p = np.empty((NJ, 3, 3), ft), np.empty((NJ, 3), ft)
    G[0], p[0] = R[0], jrest[0]
    for j in range(1, NJ):
        a = int(parents[j])
        G[j] = G[a] @ R[j]
        p[j] = p[a] + G[a] @ (jrest[j] - jrest[a])
    return G, p


def gm(s, rho, ft=np.float64):
    if rho <= 0:
        return s
    r2 = ft(rho) * ft(rho)
    return r2 * s / (r2 + s)


class Row:
    """One row's constants in the arithmetic `ft`."""

    def __init__(self, pose, u, jrest, kp, cam, norm, kp_joint, parents, lam, u_ref, rho, cam_prior, conf_thresh, ft):
        self.ft = ft
        self.Rnet = np.asarray(pose, np.float32).astype(ft).reshape(NJ, 3, 3)
        self.jrest = np.asarray(jrest, np.float32).astype(ft).reshape(NJ, 3)
        # float64 keypoints are taken as they are (tests: an unrounded projection); everything else is the operator's fp32
        self.kp = (np.asarray(kp) if np.asarray(kp).dtype == np.float64 else np.asarray(kp, np.float32)).astype(ft).reshape(-1, 3)
        self.cam0 = np.asarray(cam, np.float32).astype(ft).reshape(5)
        self.norm = ft(np.float32(norm))
        self.kp_joint, self.parents = np.asarray(kp_joint, np.int64), np.asarray(parents, np.int64)
        self.K = self.kp.shape[0]
        self.w = weights(u, lam, u_ref, ft)
        self.rho, self.cam_prior = float(rho), ft(cam_prior)
        self.c = np.array([self.kp[k, 2] if (self.kp_joint[k] >= 0 and self.kp[k, 2] > ft(conf_thresh)) else ft(0)
                           for k in range(self.K)], ft)

    def camera(self, x):
        """x = (kappa, dtx, dty) totals -> (a, tx, ty)."""
        return self.cam0[0] * np.exp(x[0]), self.cam0[1] + x[1], self.cam0[2] + x[2]

    def evaluate(self, R, x):
        """-> dict(G, p, r [K,2], s [K], q [24,3], F) at rotations R and camera totals x."""
        ft = self.ft
        G, p = forward_kinematics(R, self.jrest, self.parents, ft)
        a, tx, ty = self.camera(x)
        r, s = np.zeros((self.K, 2), ft), np.zeros(self.K, ft)
        F = ft(0)
        for k in range(self.K):
            if self.c[k] == 0:
                continue
            P = p[self.kp_joint[k]]
            r[k, 0] = (a * (P[0] + tx) + self.cam0[3] - self.kp[k, 0]) / self.norm
            r[k, 1] = (a * (P[1] + ty) + self.cam0[4] - self.kp[k, 1]) / self.norm
            s[k] = self.c[k] * (r[k, 0] * r[k, 0] + r[k, 1] * r[k, 1])
            F = F + gm(s[k], self.rho, ft)
        q = np.zeros((NJ, 3), ft)
        for j in range(NJ):
            q[j] = log_so3(self.Rnet[j].T @ R[j], ft)
            F = F + self.w[j] * (q[j, 0] * q[j, 0] + q[j, 1] * q[j, 1] + q[j, 2] * q[j, 2])
        F = F + self.cam_prior * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
        return dict(G=G, p=p, r=r, s=s, q=q, F=F, a=a, tx=tx, ty=ty)

    def jacobian(self, ev):
        """d r / d (delta_0 .. delta_23, kappa, dtx, dty) [K,2,75] at the point of `ev` (rows of unobserved keypoints are zero)."""
        ft = self.ft
        J = np.zeros((self.K, 2, NU), ft)
        f = ev["a"] / self.norm
        for k in range(self.K):
            if self.c[k] == 0:
                continue
            jk = int(self.kp_joint[k])
            for j in ancestors(self.parents, jk):
                M = -hat(ev["p"][jk] - ev["p"][j], ft) @ ev["G"][j]
                J[k, :, 3 * j:3 * j + 3] = f * M[:2]
            J[k, 0, 72] = ev["a"] * (ev["p"][jk][0] + ev["tx"]) / self.norm
            J[k, 1, 72] = ev["a"] * (ev["p"][jk][1] + ev["ty"]) / self.norm
            J[k, 0, 73] = f
            J[k, 1, 74] = f
        return J

    def irls(self, ev):
        """The weights of the Gauss-Newton step: c_k gm'(s_k) = c_k (rho^2 / (rho^2 + s_k))^2; c_k when rho is off."""
        ft = self.ft
        if self.rho <= 0:
            return self.c.copy()
        r2 = ft(self.rho) * ft(self.rho)
        return np.array([self.c[k] * (r2 / (r2 + ev["s"][k])) ** 2 for k in range(self.K)], ft)

    def normal_equations(self, ev, x):
        """A = J^T W J + priors, g = J^T W r + prior gradients (both halved: F = |.|^2 sums).  The prior's Jacobian with respect to
        delta_j is taken as the identity."""
        ft = self.ft
        J = self.jacobian(ev).reshape(2 * self.K, NU)
        wk = np.repeat(self.irls(ev), 2)
        Jw = J * np.sqrt(wk)[:, None]
        rw = ev["r"].reshape(-1) * np.sqrt(wk)
        A, g = Jw.T @ Jw, Jw.T @ rw
        for j in range(NJ):
            for c in range(3):
                A[3 * j + c, 3 * j + c] += self.w[j]
                g[3 * j + c] += self.w[j] * ev["q"][j, c]
        for c in range(3):
            A[72 + c, 72 + c] += self.cam_prior
            g[72 + c] += self.cam_prior * x[c]
        return A, g


def cholesky_solve(A, b, ft=np.float64):
    """A x = b by Cholesky without pivoting: numpy.linalg.cholesky in float64, plain loops otherwise."""
    n = A.shape[0]
    if ft is np.float64:
        L = np.linalg.cholesky(A)
    else:
        L = np.zeros_like(A)
        for c in range(n):
            L[c, c] = np.sqrt(A[c, c] - np.dot(L[c, :c], L[c, :c]))
            for i in range(c + 1, n):
                L[i, c] = (A[i, c] - np.dot(L[i, :c], L[c, :c])) / L[c, c]
    y = np.zeros(n, ft)
    for i in range(n):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(n, ft)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def refit_row(pose, u, jrest, kp, cam, norm, kp_joint=BODY25_TO_SMPL, parents=SMPL_PARENTS, lam=0.1, u_ref=0.3, rho=0.1, cam_prior=1.0,
              conf_thresh=0.3, min_kp=4, iters=10, ft=np.float64, trace=None) -> dict:
    """-> dict(pose [24,3,3], cam [3], shift [24], cost [2] in `ft`, accepted, flag).  trace: a list that receives (F, F_trial) of
    every step."""
    pose32, cam32 = np.asarray(pose, np.float32).reshape(NJ, 3, 3), np.asarray(cam, np.float32).reshape(5)
    skipped = lambda flag: dict(pose=pose32.astype(ft), cam=cam32[:3].astype(ft), shift=np.zeros(NJ, ft), cost=np.zeros(2, ft),   # noqa: E731
                                accepted=0, flag=flag)
    fin = all(np.isfinite(np.asarray(a, np.float32)).all() for a in (pose, jrest, kp, cam, norm))
    if not fin or not np.float32(norm) > 0:
        return skipped(2)
    row = Row(pose, u, jrest, kp, cam, norm, kp_joint, parents, lam, u_ref, rho, cam_prior, conf_thresh, ft)
    if int(np.count_nonzero(row.c)) < min_kp:
        return skipped(1)
    R, x = row.Rnet.copy(), np.zeros(3, ft)
    ev = row.evaluate(R, x)
    F0, mu, accepted = ev["F"], ft(MU0), 0
    for _ in range(iters):
        A, g = row.normal_equations(ev, x)
        A[np.arange(NU), np.arange(NU)] += mu * np.diag(A)
        d = cholesky_solve(A, -g, ft)
        Rt = np.stack([R[j] @ exp_so3(d[3 * j:3 * j + 3], ft) for j in range(NJ)])
        xt = x + d[72:75]
        evt = row.evaluate(Rt, xt)
        if trace is not None:
            trace.append((ev["F"], evt["F"]))
        if evt["F"] < ev["F"]:
            R, x, ev, accepted = Rt, xt, evt, accepted + 1
            mu = max(mu / ft(3), ft(MU_MIN))
        else:
            mu = min(mu * ft(3), ft(MU_MAX))
    a, tx, ty = row.camera(x)
    return dict(pose=R, cam=np.array([a, tx, ty], ft), shift=np.array([angle_deg(row.Rnet[j], R[j], ft) for j in range(NJ)], ft),
                cost=np.array([F0, ev["F"]], ft), accepted=accepted, flag=0)


def refit(pose, u, jrest, kp, cam, norm, ft=np.float64, **kw) -> dict:
    """Rows [N,...] -> the values before their one rounding (pose64 [N,24,3,3], cam64 [N,3], shift64 [N,24], cost64 [N,2] in `ft`),
    their float32 roundings (pose, cam, shift, cost) and info int32 [N,2] = (accepted steps, flag).  A skipped row's pose and cam
    are the input's bits."""
    N = len(pose)
    rows = [refit_row(pose[i], u[i], jrest[i], kp[i], cam[i], norm[i], ft=ft, **kw) for i in range(N)]
    out = {k + "64": np.stack([r[k] for r in rows]) for k in ("pose", "cam", "shift", "cost")}
    out.update({k: out[k + "64"].astype(np.float32) for k in ("pose", "cam", "shift", "cost")})
    out["info"] = np.array([[r["accepted"], r["flag"]] for r in rows], np.int32).reshape(N, 2)
    return out


def reprojection_error(pose, jrest, kp, cam3, cam5, norm, kp_joint=BODY25_TO_SMPL, parents=SMPL_PARENTS, conf_thresh=0.3) -> np.ndarray:
    """Mean over the observed keypoints of |proj(p_k) - kp_k| / norm per row [N] (NaN where none is observed); cam3 = (a, tx, ty)
    of the pose, cam5 supplies (px, py)."""
    out = np.full(len(pose), np.nan)
    for i in range(len(pose)):
        _, p = forward_kinematics(np.asarray(pose[i], np.float64), np.asarray(jrest[i], np.float64), parents)
        e = [np.hypot(cam3[i][0] * (p[j][0] + cam3[i][1]) + cam5[i][3] - kp[i][k][0],
                      cam3[i][0] * (p[j][1] + cam3[i][2]) + cam5[i][4] - kp[i][k][1]) / norm[i]
             for k, j in enumerate(kp_joint) if j >= 0 and kp[i][k][2] > conf_thresh]
        if e:
            out[i] = float(np.mean(e))
    return out


# ---- seeded material ------------------------------------------------------------------------------------------------------------
def rot_axis(axis, angle):
    axis = np.asarray(axis, np.float64)
    return exp_so3(axis / np.linalg.norm(axis) * angle)


def rest_joints(r) -> np.ndarray:
    """A plausible rest skeleton [24,3] in metres (y up as SMPL's): every joint a bone of 0.1 .. 0.45 m from its parent."""
    J = np.zeros((NJ, 3))
    for j in range(1, NJ):
        d = r.standard_normal(3)
        J[j] = J[SMPL_PARENTS[j]] + d / np.linalg.norm(d) * r.uniform(0.1, 0.45)
    return J


def project(pose, jrest, cam, kp_joint=BODY25_TO_SMPL, parents=SMPL_PARENTS) -> np.ndarray:
    """The exact keypoints [K,2] of a pose under cam [5] (zeros where unobserved)."""
    _, p = forward_kinematics(np.asarray(pose, np.float64), np.asarray(jrest, np.float64), parents)
    out = np.zeros((len(kp_joint), 2))
    for k, j in enumerate(kp_joint):
        if j >= 0:
            out[k] = cam[0] * (p[j][0] + cam[1]) + cam[3], cam[0] * (p[j][1] + cam[2]) + cam[4]
    return out


U_VALUES = (1e-8, 0.3, 1e4, np.inf)


def gpu_case(N=65, seed=31, K=25) -> dict:
    """The material of tests/test_refit_gpu.py: N rows; poses of up to 40 degrees per joint; keypoints = the projection of the pose
    turned by up to 12 degrees per joint, plus 2 % of the box of noise, confidences in [0, 1] (a third below the threshold); u from
    [0.05, 3] with U_VALUES sprinkled in; row 3 and every 16th row after it keeps two keypoints (under min_kp), row 5 carries a NaN
    in its pose and row 37 an infinity in its keypoints."""
    r = np.random.default_rng(seed)
    pose, u, jrest, kp, cam, norm = [], [], [], [], [], []
    for i in range(N):
        J = rest_joints(r)
        R = np.stack([rot_axis(r.standard_normal(3), np.deg2rad(r.uniform(0, 40))) for _ in range(NJ)])
        Rt = np.stack([R[j] @ rot_axis(r.standard_normal(3), np.deg2rad(r.uniform(0, 12))) for j in range(NJ)])
        h = r.uniform(120, 300)
        c5 = np.array([r.uniform(0.7, 1.1) * h / 2, r.uniform(-0.1, 0.1), r.uniform(-0.1, 0.1), r.uniform(200, 400), r.uniform(200, 400)])
        c5 = c5.astype(np.float32).astype(np.float64)
        xy = project(Rt.astype(np.float32), J.astype(np.float32), c5) + r.standard_normal((K, 2)) * 0.02 * h
        conf = r.uniform(0, 1, K)
        conf[r.random(K) < 0.33] *= 0.29
        if i % 16 == 3:
            conf[:] = 0.0
            conf[[1, 8]] = 0.9
        ui = r.uniform(0.05, 3.0, NJ)
        sel = r.random(NJ)
        for n, v in enumerate(U_VALUES):
            ui[(sel >= 0.06 * n) & (sel < 0.06 * (n + 1))] = v
        pose.append(R); u.append(ui); jrest.append(J); kp.append(np.concatenate([xy, conf[:, None]], 1)); cam.append(c5); norm.append(h)  # noqa: E702
    out = {k: np.ascontiguousarray(np.stack(v), np.float32) for k, v in
           (("pose", pose), ("u", u), ("jrest", jrest), ("kp", kp), ("cam", cam), ("norm", norm))}
    if N > 5:
        out["pose"][5, 7, 1, 2] = np.nan
    if N > 37:
        out["kp"][37, 3, 0] = np.inf
    return out


TURNED = (4, 5, 18, 19)                                    # knees and elbows


def recovery_case(N=6, seed=32) -> dict:
    """The recovery scene: a seeded true pose, keypoints that are its exact projection with confidence 1 on the 14 mapped
    keypoints, and a network pose that is the true one with the knees and elbows turned by 25 degrees about the camera axis (z, in
    the world frame: the local rotation is conjugated by the parent's global one) and given var 3.0; every other joint is exact with
    var 0.05."""
    r = np.random.default_rng(seed)
    out = {k: [] for k in ("pose", "u", "jrest", "kp", "cam", "norm", "truth")}
    for _ in range(N):
        J = rest_joints(r).astype(np.float32).astype(np.float64)
        R = np.stack([rot_axis(r.standard_normal(3), np.deg2rad(r.uniform(0, 30))) for _ in range(NJ)])
        h = r.uniform(150, 300)
        c5 = np.array([0.9 * h / 2, r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05), 320.0, 240.0]).astype(np.float32).astype(np.float64)
        G, _ = forward_kinematics(R, J, SMPL_PARENTS)
        net = R.copy()
        for j in TURNED:                                   # G_j' = Rz G_j: R_j' = G_parent^T Rz G_parent R_j
            Gp = G[SMPL_PARENTS[j]]
            net[j] = Gp.T @ rot_axis([0, 0, 1], np.deg2rad(25.0)) @ Gp @ R[j]
        # the joints BELOW a turned joint keep their true GLOBAL orientation only if their local rotation absorbs the turn; the
        # network's error is in the turned joint alone, so its descendants' local rotations stay the true ones
        xy = project(R, J, c5)
        conf = (BODY25_TO_SMPL >= 0).astype(np.float64)
        ui = np.full(NJ, 0.05)
        ui[list(TURNED)] = 3.0
        for k, v in (("pose", net), ("u", ui), ("jrest", J), ("kp", np.concatenate([xy, conf[:, None]], 1)), ("cam", c5), ("norm", h),
                     ("truth", R)):
            out[k].append(v)
    return {k: np.ascontiguousarray(np.stack(v), np.float64 if k == "truth" else np.float32) for k, v in out.items()}
