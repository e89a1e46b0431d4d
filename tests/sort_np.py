"""SORT on per-frame detections (poco_op_sort_tracks) restated in numpy with plain loops: one tracker object
at a time, one frame at a time, the contract's sequence of operations written out (each product sum over c = 0..3 in ascending c).
Nothing here is imported by the package.  `dtype` is numpy.float64 (the contract) or numpy.longdouble (tests: the rounding floor of
the arithmetic itself).  The assignment is NOT the operator's method: it is scipy.optimize.linear_sum_assignment on the gated
matrix, or an exhaustive search for small matrices (brute_assign).

Besides the five outputs it reports per frame two decision margins: `margin_assign`, the gap between the best total and the best
total with any one chosen pair forbidden, and `margin_gate`, the smallest |IoU - iou_thresh| over all pairs.  Where both exceed the
rounding of fp64 by orders of magnitude, two fp64 implementations of the contract must take the same discrete decisions."""
import itertools

import numpy as np

R_DIAG = (1.0, 1.0, 10.0, 10.0)
Q_DIAG = (1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.0001)
P0_DIAG = (10.0, 10.0, 10.0, 10.0, 10000.0, 10000.0, 10000.0)


def dense_matrices(dtype=np.float64):
    """F, H, Q, R and the initial P of the published sort.py (KalmanBoxTracker.__init__) as dense matrices."""
    F = np.eye(7, dtype=dtype)
    F[0, 4] = F[1, 5] = F[2, 6] = 1
    H = np.eye(4, 7, dtype=dtype)
    return F, H, np.diag(np.asarray(Q_DIAG, dtype)), np.diag(np.asarray(R_DIAG, dtype)), np.diag(np.asarray(P0_DIAG, dtype))


def lower_mirrored(P):
    """The contract keeps the covariance symmetric: the elements r >= c are the computed ones, the upper triangle is their copy."""
    return np.tril(P) + np.tril(P, -1).T


class Tracker:
    def __init__(self, det, ident, dtype):
        self.dtype = dtype
        cx, cy, w, h = (dtype(v) for v in det)
        self.x = np.array([cx, cy, w * h, w / h, 0, 0, 0], dtype)
        self.P = np.diag(np.asarray(P0_DIAG, dtype))
        self.id = ident
        self.time_since_update = 0
        self.hits = 0
        self.hit_streak = 0
        self.age = 0

    def predict(self):
        F, _, Q, _, _ = dense_matrices(self.dtype)
        self.shrink_rule = bool(self.x[2] + self.x[6] <= 0)
        if self.shrink_rule:
            self.x[6] = 0
        self.x = F @ self.x                         # every element is a sum of at most two terms: no order to state
        self.P = lower_mirrored(F @ self.P @ F.T + Q)
        self.age += 1
        if self.time_since_update > 0:
            self.hit_streak = 0
        self.time_since_update += 1

    def update(self, det):
        dt = self.dtype
        cx, cy, w, h = (dt(v) for v in det)
        z = np.array([cx, cy, w * h, w / h], dt)
        x, P = self.x, self.P
        R = np.asarray(R_DIAG, dt)
        y = z - x[:4]
        S = P[:4, :4].copy()
        for i in range(4):
            S[i, i] = S[i, i] + R[i]
        # S = L D L^T, the lower triangle of S, no pivoting
        L, D = np.eye(4, dtype=dt), np.zeros(4, dt)
        for j in range(4):
            v = S[j, j]
            for k in range(j):
                v = v - L[j, k] * (L[j, k] * D[k])
            D[j] = v
            for i in range(j + 1, 4):
                v = S[i, j]
                for k in range(j):
                    v = v - L[i, k] * (L[j, k] * D[k])
                L[i, j] = v / D[j]
        # K = P[:, :4] S^-1, row by row: L w = b, w / D, L^T k = w
        K = np.zeros((7, 4), dt)
        for r in range(7):
            w_ = np.zeros(4, dt)
            for i in range(4):
                v = P[r, i]
                for k in range(i):
                    v = v - L[i, k] * w_[k]
                w_[i] = v
            for i in range(4):
                w_[i] = w_[i] / D[i]
            for i in range(3, -1, -1):
                v = w_[i]
                for k in range(i + 1, 4):
                    v = v - L[k, i] * K[r, k]
                K[r, i] = v
        # x += K y
        acc = K[:, 0] * y[0]
        for c in range(1, 4):
            acc = acc + K[:, c] * y[c]
        self.x = x + acc
        # Joseph form with A = I - K H: AP = P - K P[:4, :], then (AP - AP[:, :4] K^T) + (K R) K^T
        T = K[:, [0]] * P[[0], :]
        for c in range(1, 4):
            T = T + K[:, [c]] * P[[c], :]
        AP = P - T
        T1 = AP[:, [0]] * K[:, 0][None, :]
        T2 = (K[:, [0]] * R[0]) * K[:, 0][None, :]
        for c in range(1, 4):
            T1 = T1 + AP[:, [c]] * K[:, c][None, :]
            T2 = T2 + (K[:, [c]] * R[c]) * K[:, c][None, :]
        self.P = lower_mirrored((AP - T1) + T2)
        self.time_since_update = 0
        self.hits += 1
        self.hit_streak += 1

    def size(self):
        """(w, h) of the state: w = sqrt(s r), h = s / w (NaN where s r < 0)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.sqrt(self.x[2] * self.x[3])
            return w, self.x[2] / w

    def box(self):
        w, h = self.size()
        return np.array([self.x[0], self.x[1], w, h], self.dtype)


def corners(cx, cy, w, h):
    return cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2


def iou(a, b):
    """a, b: x1y1x2y2."""
    xx1, yy1, xx2, yy2 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    zero = type(xx1)(0)
    w, h = max(zero, xx2 - xx1), max(zero, yy2 - yy1)
    wh = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return wh / (((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - wh)


def brute_assign(g):
    """The best total of a gated matrix by exhaustive search, and one matching that reaches it: [(row, col), ...] of pairs with g > 0."""
    g = np.asarray(g, np.float64)
    n, m = g.shape
    if n == 0 or m == 0:
        return 0.0, []
    best, pairs = -1.0, []
    if n <= m:
        for cols in itertools.permutations(range(m), n):
            t = sum(g[i, c] for i, c in enumerate(cols))
            if t > best:
                best, pairs = t, [(i, c) for i, c in enumerate(cols) if g[i, c] > 0]
    else:
        for rows in itertools.permutations(range(n), m):
            t = sum(g[r, j] for j, r in enumerate(rows))
            if t > best:
                best, pairs = t, [(r, j) for j, r in enumerate(rows) if g[r, j] > 0]
    return float(best), pairs


def assign(g, brute_below=5):
    """(total, pairs) of a matching that maximises the sum of g; pairs with g = 0 are no matches."""
    g = np.asarray(g, np.float64)
    if g.size == 0:
        return 0.0, []
    if max(g.shape) < brute_below:
        return brute_assign(g)
    from scipy.optimize import linear_sum_assignment
    r, c = linear_sum_assignment(g, maximize=True)
    pairs = [(int(i), int(j)) for i, j in zip(r, c) if g[i, j] > 0]
    return float(sum(g[i, j] for i, j in pairs)), pairs


def sort_tracks(dets, frame_offsets, clip_offsets=None, iou_thresh=0.3, max_age=1, min_hits=3, max_trackers=64, dtype=np.float64):
    """dets [N,>=4] (cx, cy, w, h), frame_offsets [F+1], clip_offsets [C+1] (None: one clip) -> dict(tracker [N], id [N], box [N,4],
    count [C], status [C], margin_assign [F], margin_gate [F], total [F], shrink_rule = how often the s + s' <= 0 rule applied); margins are +inf where a frame takes no such decision."""
    dets = np.asarray(dets, dtype).reshape(-1, np.shape(dets)[-1] if np.ndim(dets) == 2 else 4)[:, :4]
    fo = np.asarray(frame_offsets, np.int64)
    F, N = len(fo) - 1, len(dets)
    co = np.array([0, F], np.int64) if clip_offsets is None else np.asarray(clip_offsets, np.int64)
    Cn = len(co) - 1
    thr = dtype(iou_thresh)
    out = {"tracker": np.full(N, -1, np.int32), "id": np.full(N, -1, np.int32), "box": np.full((N, 4), np.nan, dtype),
           "count": np.zeros(Cn, np.int32), "status": np.zeros(Cn, np.int32), "margin_assign": np.full(F, np.inf),
           "margin_gate": np.full(F, np.inf), "total": np.zeros(F), "shrink_rule": 0}
    for c in range(Cn):
        trackers, next_id = [], 0
        for f in range(co[c], co[c + 1]):
            fc = f - co[c] + 1
            lo, hi = fo[f], fo[f + 1]
            D = hi - lo
            for t in trackers:
                t.predict()
                out["shrink_rule"] += int(t.shrink_rule)
            g = np.zeros((D, len(trackers)))
            for k, t in enumerate(trackers):
                w, h = t.size()
                ok = bool(np.isfinite(w) and np.isfinite(h) and np.isfinite(t.x[0]) and np.isfinite(t.x[1]) and w > 0 and h > 0)
                tb = corners(t.x[0], t.x[1], w, h)
                for d in range(D):
                    o = iou(corners(*dets[lo + d]), tb) if ok else dtype(0)
                    if ok and np.isfinite(o):
                        out["margin_gate"][f] = min(out["margin_gate"][f], abs(float(o - thr)))
                    g[d, k] = float(o) if (ok and o >= thr) else 0.0
            total, pairs = assign(g)
            out["total"][f] = total
            for (d, k) in pairs:                                         # the best total with one chosen pair forbidden
                g2 = g.copy()
                g2[d, k] = 0.0
                out["margin_assign"][f] = min(out["margin_assign"][f], total - assign(g2)[0])
            det_of = {k: d for d, k in pairs}
            matched = {d for d, _ in pairs}
            births = [d for d in range(D) if d not in matched]
            if len(trackers) + len(births) > max_trackers:
                out["status"][c] = 1
                break
            slot = {}
            for k, t in enumerate(trackers):
                if k in det_of:
                    t.update(dets[lo + det_of[k]])
                    slot[det_of[k]] = t
            for d in births:
                t = Tracker(dets[lo + d], next_id, dtype)
                next_id += 1
                trackers.append(t)
                slot[d] = t
            for d in range(D):
                t = slot[d]
                out["tracker"][lo + d] = t.id
                out["box"][lo + d] = t.box()
                if t.time_since_update == 0 and (t.hit_streak >= min_hits or fc <= min_hits):
                    out["id"][lo + d] = t.id
            trackers = [t for t in trackers if t.time_since_update <= max_age]
        out["count"][c] = next_id
    return out
