"""The in-fill of unreliable joint rotations (demo.py --mode video --infill, poco_op_track_infill) restated in float64 numpy with
plain loops: the contract of DESIGN.md section 24 in executable form, and the yardstick of tests/test_infill_gpu.py.  There is no
counterpart in the reference's code.

Inputs, concatenated over the P tracks of a clip (N rows): offsets int32 [P+1], frames int32 [N] (strictly increasing within a
track, holes allowed), pose fp32 [N,24,3,3] (proper rotations), u fp32 [N,24], lin fp32 [N,L], thresh, max_gap >= 1.
Every sum below is written in the order the kernel adds in; nothing is contracted."""
import numpy as np

NJ = 24
MAX_LIN = 16


def quat_of(R) -> np.ndarray:
    """Row-major 3x3 -> unit quaternion (w, x, y, z), float64: the largest of (trace, m00, m11, m22), the first of equals
    (Shepperd), then normalised."""
    m = np.asarray(R, np.float64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (np.float64(v) for v in m.reshape(9))
    tr = (m00 + m11) + m22
    k = int(np.argmax([tr, m00, m11, m22]))           # argmax: the first maximum
    one, two, quarter = np.float64(1.0), np.float64(2.0), np.float64(0.25)
    if k == 0:
        s = np.sqrt(one + tr) * two
        q = [quarter * s, (m21 - m12) / s, (m02 - m20) / s, (m10 - m01) / s]
    elif k == 1:
        s = np.sqrt(((one + m00) - m11) - m22) * two
        q = [(m21 - m12) / s, quarter * s, (m01 + m10) / s, (m02 + m20) / s]
    elif k == 2:
        s = np.sqrt(((one + m11) - m00) - m22) * two
        q = [(m02 - m20) / s, (m01 + m10) / s, quarter * s, (m12 + m21) / s]
    else:
        s = np.sqrt(((one + m22) - m00) - m11) * two
        q = [(m10 - m01) / s, (m02 + m20) / s, (m12 + m21) / s, quarter * s]
    q = np.array(q, np.float64)
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def slerp(qa, qb, s) -> np.ndarray:
    """Shortest arc: qb is negated when qa.qb < 0; |qa.qb| > 1 - 1e-12: the normalised linear blend; else acos and sin."""
    qa, qb, s = np.asarray(qa, np.float64), np.asarray(qb, np.float64), np.float64(s)
    d = ((qa[0] * qb[0] + qa[1] * qb[1]) + qa[2] * qb[2]) + qa[3] * qb[3]
    if d < 0.0:
        qb, d = -qb, -d
    if d > 1.0 - 1e-12:
        q = qa + s * (qb - qa)
        n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        return q / n
    th = np.arccos(d)
    st = np.sin(th)
    wa, wb = np.sin((np.float64(1.0) - s) * th) / st, np.sin(s * th) / st
    return wa * qa + wb * qb


def rotmat_of(q) -> np.ndarray:
    """Unit quaternion -> rotation matrix, the standard form, float64."""
    w, x, y, z = (np.float64(v) for v in q)
    one, two = np.float64(1.0), np.float64(2.0)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], np.float64)


def decide(frames, reliable, t, lo, hi, max_gap):
    """The rule for the unreliable entry at row t of a column whose track is rows [lo, hi): -> (flag, a, b, c, s); rows that play no
    part are -1, s is None unless flag = 1."""
    a = b = -1
    for r in range(t - 1, lo - 1, -1):
        if reliable[r]:
            a = r
            break
    for r in range(t + 1, hi):
        if reliable[r]:
            b = r
            break
    ft = int(frames[t])
    if a >= 0 and b >= 0 and int(frames[b]) - int(frames[a]) <= max_gap:
        s = np.float64(ft - int(frames[a])) / np.float64(int(frames[b]) - int(frames[a]))
        return 1, a, b, -1, s
    if a < 0 and b < 0:
        return 3, a, b, -1, None
    if b < 0 or (a >= 0 and ft - int(frames[a]) <= int(frames[b]) - ft):          # a tie goes to a
        c = a
    else:
        c = b
    if abs(ft - int(frames[c])) <= max_gap // 2:
        return 2, a, b, c, None
    return 3, a, b, c, None


def infill(pose, u, frames, offsets, lin, thresh, max_gap):
    """-> dict(pose [N,24,3,3] fp32, lin [N,L] fp32, flags uint8 [N,24], touched uint8 [N], pose64 [N,24,3,3] float64 = the
    interpolated matrices before the final rounding (the input's values elsewhere))."""
    pose = np.ascontiguousarray(pose, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    lin = np.ascontiguousarray(lin, np.float32)
    frames, offsets = np.asarray(frames), np.asarray(offsets)
    N = pose.shape[0]
    assert pose.shape == (N, NJ, 3, 3) and u.shape == (N, NJ) and frames.shape == (N,) and lin.shape[0] == N and lin.shape[1] <= MAX_LIN
    assert max_gap >= 1 and offsets[0] == 0 and offsets[-1] == N and np.all(np.diff(offsets) > 0)
    thresh = np.float32(thresh)
    with np.errstate(invalid="ignore"):
        reliable = u <= thresh                                               # a NaN compares false
    out, out64, lin_out = pose.copy(), pose.astype(np.float64), lin.copy()
    flags = np.zeros((N, NJ), np.uint8)
    for p in range(len(offsets) - 1):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        for j in range(NJ):
            for t in range(lo, hi):
                if reliable[t, j]:
                    continue
                flag, a, b, c, s = decide(frames, reliable[:, j], t, lo, hi, max_gap)
                flags[t, j] = flag
                if flag == 1:
                    R = rotmat_of(slerp(quat_of(pose[a, j]), quat_of(pose[b, j]), s))
                    out64[t, j] = R
                    out[t, j] = R.astype(np.float32)
                    if j == 0:
                        la, lb = lin[a].astype(np.float64), lin[b].astype(np.float64)
                        lin_out[t] = (la + s * (lb - la)).astype(np.float32)
                elif flag == 2:
                    out[t, j] = pose[c, j]
                    out64[t, j] = pose[c, j]
                    if j == 0:
                        lin_out[t] = lin[c]
    touched = ((flags == 1) | (flags == 2)).any(1).astype(np.uint8)
    return {"pose": out, "lin": lin_out, "flags": flags, "touched": touched, "pose64": out64}


# ---- test material --------------------------------------------------------------------------------------------------------
def rot_axis(axis, angle) -> np.ndarray:
    """Rodrigues' formula in float64: the rotation by `angle` about `axis`."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], np.float64)
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def smooth_rotations(rng, T, max_step_deg=12.0) -> np.ndarray:
    """[T,24,3,3] fp32 proper rotations: a random start per joint, then steps of at most max_step_deg about random axes.  With runs
    of at most 170 / max_step_deg rows between anchors the anchors' relative angle stays below 170 degrees."""
    out = np.empty((T, NJ, 3, 3), np.float64)
    for j in range(NJ):
        R = rot_axis(rng.standard_normal(3), rng.uniform(0, np.pi))
        for t in range(T):
            out[t, j] = R
            R = R @ rot_axis(rng.standard_normal(3), np.deg2rad(rng.uniform(0.0, max_step_deg)))
    return out.astype(np.float32)


def relative_angle_deg(Ra, Rb) -> float:
    c = (np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
