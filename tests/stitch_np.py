"""Track stitching (poco_op_track_stitch) restated in numpy with plain loops: one fragment at a time, one
pair at a time, the contract's sequence of operations written out.  Nothing here is imported by the package.  `dtype` is
numpy.float64 (the contract) or numpy.longdouble (tests: the rounding floor of the arithmetic itself).  The assignment is NOT the
operator's method: it is scipy.optimize.linear_sum_assignment on the gain matrix, or an exhaustive search for small matrices
(brute_assign).

Besides the six outputs it reports per clip three decision margins: `margin_assign`, the gap between the best total and the best
total with any one chosen link forbidden (inf without a link); `margin_gate`, the least |c_m - 1| and |c_s - 1| over the admissible
pairs (inf without one); `margin_gap`, the least |D - (max_gap + 1)| over all ordered pairs with D >= 1, an integer.  Where the first
two exceed the rounding of fp64 by orders of magnitude, two fp64 implementations of the contract take the same discrete decisions."""
import itertools

import numpy as np

DESC = 28
SLOTS = 64


def tree_sum(values, dtype):
    """The contract's sum over the rows of a fragment: slot l of 64 adds its rows l, l + 64, ... in ascending order to 0, then
    slot t takes slot t + o for o = 32, 16, .., 1."""
    slots = [dtype(0)] * SLOTS
    for i, v in enumerate(values):
        slots[i % SLOTS] = slots[i % SLOTS] + v
    o = SLOTS // 2
    while o > 0:
        for t in range(o):
            slots[t] = slots[t] + slots[t + o]
        o //= 2
    return slots[0]


def line_fit(t, q, dtype):
    """(state at t = 0, velocity) of the least-squares line of q against t, the normal equations written with centred t."""
    m = len(t)
    tsum, qsum = dtype(0), dtype(0)
    for j in range(m):
        tsum = tsum + dtype(t[j])
        qsum = qsum + q[j]
    tbar, qbar = tsum / dtype(m), qsum / dtype(m)
    stt, stq = dtype(0), dtype(0)
    for j in range(m):
        dt = dtype(t[j]) - tbar
        dq = q[j] - qbar
        stt = stt + dt * dt
        stq = stq + dt * dq
    if m > 1 and stt > 0:
        vel = stq / stt
        return qbar - vel * tbar, vel
    return qbar, dtype(0)


def describe(frames, boxes, betas, var, fit_len, u_ref, dtype):
    """The 28 numbers of one fragment."""
    T = len(frames)
    s, e = int(frames[0]), int(frames[-1])
    w = []
    for i in range(T):
        u = dtype(var[i][0])
        for j in range(1, 24):
            u = u + dtype(var[i][j])
        u = u / dtype(24)
        r = dtype(u_ref) / (u if u > dtype(1e-6) else dtype(1e-6))
        w.append(r * r)
    W = tree_sum(w, dtype)
    W2 = tree_sum([wi * wi for wi in w], dtype)
    bbar = [tree_sum([w[i] * dtype(betas[i][k]) for i in range(T)], dtype) / W for k in range(10)]
    spread = []
    for i in range(T):
        d0 = dtype(betas[i][0]) - bbar[0]
        d = d0 * d0
        for k in range(1, 10):
            dk = dtype(betas[i][k]) - bbar[k]
            d = d + dk * dk
        spread.append(w[i] * d)
    sig2 = tree_sum(spread, dtype) / W / dtype(10)
    m = min(int(fit_len), T)
    out = [*bbar, sig2, W, W2, dtype(T)]
    for rows, ref in ((range(T - m, T), e), (range(m), s)):
        t = [int(frames[i]) - ref for i in rows]
        fits = [line_fit(t, [dtype(boxes[i][0]) for i in rows], dtype), line_fit(t, [dtype(boxes[i][1]) for i in rows], dtype),
                line_fit(t, [np.log(dtype(boxes[i][3])) for i in rows], dtype)]
        out += [f[0] for f in fits] + [f[1] for f in fits]
    return np.asarray(out + [dtype(s), dtype(e)], dtype)


def pair_gain(da, db, max_gap, motion_tol, shape_tol, shape_floor, shape_w, dtype):
    """(gain, c_m, c_s, D) of the ordered pair a -> b of one clip, a != b; c_m = c_s = None where the pair is not admissible."""
    D = int(db[26]) - int(da[27])
    if D < 1 or D > int(max_gap) + 1:
        return dtype(0), None, None, D
    h = dtype(D) / dtype(2)
    pa = [da[14 + k] + da[17 + k] * h for k in range(3)]
    pb = [db[20 + k] - db[23 + k] * h for k in range(3)]
    dx, dy, dl = pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]
    with np.errstate(all="ignore"):
        cm = np.sqrt((dx * dx + dy * dy) / (np.exp(pa[2]) * np.exp(pb[2])) + dl * dl) / (dtype(motion_tol) * np.sqrt(dtype(D)))
        e0 = da[0] - db[0]
        ss = e0 * e0
        for k in range(1, 10):
            ek = da[k] - db[k]
            ss = ss + ek * ek
        cs = np.sqrt(ss / dtype(10)) / np.sqrt((da[10] + db[10]) + dtype(shape_floor) * dtype(shape_floor)) / dtype(shape_tol)
    if not np.isfinite(cm) or not np.isfinite(cs) or cm > 1 or (shape_w > 0 and cs > 1):
        return dtype(0), cm, cs, D
    g = dtype(1) - (cm * cm + dtype(shape_w) * (cs * cs)) / (dtype(1) + dtype(shape_w))
    return (g if g > 0 else dtype(0)), cm, cs, D


def brute_assign(G):
    """(total, column of every row or -1) of a best matching of the square G >= 0, by trying every permutation (n <= 6)."""
    n = len(G)
    best, arg = -1.0, None
    for perm in itertools.permutations(range(n)):
        tot = sum(float(G[i][perm[i]]) for i in range(n))
        if tot > best:
            best, arg = tot, perm
    return best, [arg[i] if G[i][arg[i]] > 0 else -1 for i in range(n)]


def assign(G):
    """(total, column of every row or -1): scipy's optimum of the square G >= 0; pairs of gain 0 are no links."""
    from scipy.optimize import linear_sum_assignment
    n = len(G)
    if n == 0:
        return 0.0, []
    A = np.asarray(G, np.float64)
    rows, cols = linear_sum_assignment(-A)
    col = [-1] * n
    for r, c in zip(rows, cols):
        if A[r, c] > 0:
            col[r] = int(c)
    return float(sum(A[r, col[r]] for r in range(n) if col[r] >= 0)), col


def chains_of(succ, pred):
    """Chain numbers from 0 in the order of the chains' first fragments' indices."""
    n = len(succ)
    chain, number = [-1] * n, 0
    for f in range(n):
        if pred[f] < 0:
            g = f
            while g >= 0:
                chain[g] = number
                g = succ[g]
            number += 1
    return chain


def track_stitch(clip_offsets, frag_offsets, frames, boxes, betas, var, max_gap=30, fit_len=8, u_ref=0.3, motion_tol=0.5, shape_tol=1.0,
                 shape_floor=0.05, shape_w=1.0, dtype=np.float64, solver=assign):
    fo = np.asarray(frag_offsets)
    P = len(fo) - 1
    co = np.asarray([0, P] if clip_offsets is None else clip_offsets)
    Cn = len(co) - 1
    desc = np.zeros((P, DESC), dtype)
    for p in range(P):
        lo, hi = int(fo[p]), int(fo[p + 1])
        desc[p] = describe(frames[lo:hi], boxes[lo:hi], betas[lo:hi], var[lo:hi], fit_len, u_ref, dtype)
    succ, pred, chain = np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.zeros(P, np.int32)
    gain, total = np.zeros(P, dtype), np.zeros(Cn, np.float64)
    m_assign, m_gate, m_gap = np.full(Cn, np.inf), np.full(Cn, np.inf), np.full(Cn, np.iinfo(np.int64).max, np.int64)
    matrices = []
    for c in range(Cn):
        lo, n = int(co[c]), int(co[c + 1] - co[c])
        G = np.zeros((n, n), dtype)
        for a in range(n):
            for b in range(n):
                if a == b:
                    continue
                g, cm, cs, D = pair_gain(desc[lo + a], desc[lo + b], max_gap, motion_tol, shape_tol, shape_floor, shape_w, dtype)
                G[a, b] = g
                if D >= 1:
                    m_gap[c] = min(m_gap[c], abs(D - (int(max_gap) + 1)))
                if cm is not None:
                    for v in (cm,) + ((cs,) if shape_w > 0 else ()):
                        if np.isfinite(v):
                            m_gate[c] = min(m_gate[c], abs(float(v) - 1.0))
        matrices.append(G)
        total[c], col = solver(G)
        for a in range(n):
            if col[a] >= 0:
                succ[lo + a], pred[lo + col[a]], gain[lo + a] = lo + col[a], lo + a, G[a, col[a]]
                H = np.array(G, np.float64)
                H[a, col[a]] = -1e9                                                # this link forbidden
                m_assign[c] = min(m_assign[c], total[c] - assign(np.maximum(H, -1e9))[0] if n > 1 else np.inf)
        ch = chains_of([s - lo if s >= 0 else -1 for s in succ[lo:lo + n]], [q - lo if q >= 0 else -1 for q in pred[lo:lo + n]])
        chain[lo:lo + n] = ch
    return {"succ": succ, "pred": pred, "chain": chain, "gain": gain, "desc": desc, "status": np.zeros(Cn, np.int32), "total": total,
            "margin_assign": m_assign, "margin_gate": m_gate, "margin_gap": m_gap, "G": matrices}
