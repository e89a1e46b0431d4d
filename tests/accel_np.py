"""The temporal metric of eval.py --sequences (poco_op_track_accel) restated in float64 with plain loops: no
code shared with poco_amd.  Row i of a ragged buffer of tracks is valid when rows i-1, i, i+1 lie in one track and their frame ids
are consecutive; accel = mean over the joints of |p[i-1] - 2 p[i] + p[i+1]|, accel_err = the same of the difference between the
prediction's and the ground truth's second difference (compute_error_accel of the VIBE line of work, per frame^2)."""
import math

import numpy as np


def track_accel(pred, gt, frames, offsets):
    """pred, gt [N,M,3] (gt may be None), frames [N], offsets [P+1] -> dict(accel64 / accel_err64 float64 [N] with NaN in the
    invalid rows, valid bool [N], terms [N,3] = what the sums add (0 in invalid rows), track_sums float64 [P,3], total [3],
    abs_track [P,3] / abs_total [3] = the sums of the absolute terms, for the bound of the sums)."""
    pred = np.asarray(pred, np.float64)
    gt = None if gt is None else np.asarray(gt, np.float64)
    frames = [int(f) for f in np.asarray(frames).reshape(-1)]
    offsets = [int(o) for o in np.asarray(offsets).reshape(-1)]
    N, M = pred.shape[0], pred.shape[1]
    P = len(offsets) - 1
    accel = [float("nan")] * N
    err = [float("nan")] * N
    valid = [False] * N
    terms = np.zeros((N, 3), np.float64)
    track_sums = np.zeros((P, 3), np.float64)
    abs_track = np.zeros((P, 3), np.float64)
    for p in range(P):
        lo, hi = offsets[p], offsets[p + 1]
        for i in range(lo + 1, hi - 1):
            if not (frames[i - 1] + 1 == frames[i] and frames[i] + 1 == frames[i + 1]):
                continue
            sa, se = 0.0, 0.0
            for m in range(M):
                a = [(pred[i - 1, m, c] - 2.0 * pred[i, m, c]) + pred[i + 1, m, c] for c in range(3)]
                sa += math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) if all(map(math.isfinite, a)) else float("nan")
                if gt is not None:
                    g = [(gt[i - 1, m, c] - 2.0 * gt[i, m, c]) + gt[i + 1, m, c] for c in range(3)]
                    e = [a[c] - g[c] for c in range(3)]
                    se += math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) if all(map(math.isfinite, e)) else float("nan")
            valid[i] = True
            accel[i], err[i] = sa / M, se / M
            terms[i] = (err[i], accel[i], 1.0)
        track_sums[p] = [math.fsum(terms[lo:hi, c]) for c in range(3)]
        abs_track[p] = [math.fsum(np.abs(terms[lo:hi, c])) for c in range(3)]
    total = np.array([math.fsum(terms[:, c]) for c in range(3)])
    abs_total = np.array([math.fsum(np.abs(terms[:, c])) for c in range(3)])
    out = {"accel64": np.array(accel), "valid": np.array(valid), "terms": terms, "track_sums": track_sums, "total": total,
           "abs_track": abs_track, "abs_total": abs_total}
    out["accel_err64"] = np.array(err) if gt is not None else np.full(N, np.nan)
    if gt is None:
        out["terms"][:, 0] = 0.0
        out["track_sums"][:, 0] = 0.0
        out["total"][0] = 0.0
    return out


def ulp_distance(a32, b64):
    """How many float32 steps lie between a32 (float32) and the float64 values b64 rounded to float32; NaN where either is NaN."""
    a = np.asarray(a32, np.float32)
    b = np.asarray(b64, np.float64).astype(np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.where(np.isnan(a) | np.isnan(b), -1, np.abs(ia - ib))
