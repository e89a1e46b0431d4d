"""The yardstick of the cluster bootstrap (include/poco_hip.h poco_op_bootstrap, poco_amd/bootstrap.py), restated
with plain loops: Philox4x32-10, the index map, the unit moments and the resample sums with math.fsum, and the statistics.  It shares
no code with csrc/bootstrap.hip or poco_amd/bootstrap.py."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(counter, key):
    """Philox4x32-10 of Salmon et al. (Random123): four 32-bit counter words and two key words -> four output words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def draws(seed, b, U):
    """The U unit indices of replicate b >= 1: word i of philox((q, 0, b, 0), (seed low, seed high)) is draw 4 q + i."""
    key = (seed & MASK, (seed >> 32) & MASK)
    idx = []
    for q in range((U + 3) // 4):
        idx += [(w * U) >> 32 for w in philox((q, 0, b, 0), key)]
    return np.asarray(idx[:U], np.int64)


def draws_np(seed, b, U):
    """draws() with the counters q = 0 .. ceil(U / 4) - 1 carried through the ten rounds side by side in uint64 arrays (a product of two
    32-bit words fits); tests/test_boot_cpu.py holds it against draws()."""
    u64 = np.uint64
    q = np.arange((U + 3) // 4, dtype=np.uint64)
    c = [q, np.zeros_like(q), np.full_like(q, b), np.zeros_like(q)]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = u64(M0) * c[0], u64(M1) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ u64(k0), p1 & u64(MASK), (p0 >> u64(32)) ^ c[3] ^ u64(k1), p0 & u64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return ((np.stack(c, axis=1).reshape(-1)[:U] * u64(U)) >> u64(32)).astype(np.int64)


def fsum(values):
    """math.fsum that follows IEEE where it raises: NaN with a NaN or with infinities of both signs, else the infinity, else fsum."""
    v = [float(x) for x in values]
    if any(x != x for x in v):
        return math.nan
    pos, neg = any(x == math.inf for x in v), any(x == -math.inf for x in v)
    if pos or neg:
        return math.nan if pos and neg else (math.inf if pos else -math.inf)
    return math.fsum(v)


def mag(values):
    """The sum of |terms| over the finite terms (the scale of a sum's rounding bound)."""
    return math.fsum(abs(float(x)) for x in values if math.isfinite(float(x)))


def offsets_of(n, unit_offsets):
    return np.arange(n + 1, dtype=np.int64) if unit_offsets is None else np.asarray(unit_offsets, np.int64)


def centers(planes):
    """-> (center [E], sum |v| / n [E])."""
    planes = np.asarray(planes, np.float32)
    n = planes.shape[1]
    return np.asarray([fsum(p) / n for p in planes]), np.asarray([mag(p) / n for p in planes])


def unit_moments(planes, pairs, unit_offsets, center):
    """-> (unit_mom [U, M], sum |terms| [U, M]) with the given centres (float64 [E]): the products are formed as the header states
    them, each factor and the product rounded to float64, and added with fsum."""
    planes = np.asarray(planes, np.float32)
    E, n = planes.shape
    off = offsets_of(n, unit_offsets)
    U, M = len(off) - 1, 1 + E + len(pairs)
    mom, mags = np.zeros((U, M)), np.zeros((U, M))
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(U):
            lo, hi = int(off[u]), int(off[u + 1])
            mom[u, 0] = hi - lo
            for e in range(E):
                terms = [float(v) for v in planes[e, lo:hi]]
                mom[u, 1 + e], mags[u, 1 + e] = fsum(terms), mag(terms)
            for k, (a, b) in enumerate(pairs):
                terms = [float((np.float64(x) - center[a]) * (np.float64(y) - center[b])) for x, y in zip(planes[a, lo:hi], planes[b, lo:hi])]
                mom[u, 1 + E + k], mags[u, 1 + E + k] = fsum(terms), mag(terms)
    return mom, mags


def resample(unit_mom, B, seed):
    """-> (out [B + 1, M], sum |terms| [B + 1, M], draw_counts [B, U]) from the given unit moments: row 0 every unit once."""
    unit_mom = np.asarray(unit_mom, np.float64)
    U, M = unit_mom.shape
    out, mags, counts = np.zeros((B + 1, M)), np.zeros((B + 1, M)), np.zeros((B, U), np.int64)
    for b in range(B + 1):
        idx = np.arange(U) if b == 0 else draws_np(seed, b, U)
        if b:
            counts[b - 1] = np.bincount(idx, minlength=U)
        rows = unit_mom[idx]
        for m in range(M):
            out[b, m], mags[b, m] = fsum(rows[:, m]), mag(rows[:, m])
    return out, mags, counts


def bootstrap(planes, pairs, unit_offsets, B, seed):
    """The whole operator by its own arithmetic -> dict(center, unit_mom, out, draw_counts)."""
    center, _ = centers(planes)
    mom, _ = unit_moments(planes, pairs, unit_offsets, center)
    out, _, counts = resample(mom, B, seed)
    return {"center": center, "unit_mom": mom, "out": out, "draw_counts": counts}


# ---- the statistics of poco_amd/bootstrap.py -----------------------------------------------------------------------------------------
def mean_of(out, col, scale=1.0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray([scale * row[col] / row[0] for row in out])


def pearson_of(out, center, E, a, b, kaa, kbb, kab):
    """Pearson's r of planes a and b per row of `out`, from the count, the raw sums and the centred product columns kaa, kbb, kab
    (pair indices).  NaN where a variance is not positive or the row count is zero."""
    r = []
    for row in out:
        cnt = row[0]
        if not cnt > 0:
            r.append(math.nan)
            continue
        sa, sb = row[1 + a] - cnt * center[a], row[1 + b] - cnt * center[b]
        vaa, vbb, vab = row[1 + E + kaa] - sa * sa / cnt, row[1 + E + kbb] - sb * sb / cnt, row[1 + E + kab] - sa * sb / cnt
        r.append(vab / math.sqrt(vaa * vbb) if vaa > 0 and vbb > 0 else math.nan)
    return np.asarray(r)


def summarize(stat, level):
    """One statistic [B + 1] (entry 0 = the full sample) -> (point, se, lo, hi, valid)."""
    reps = np.asarray(stat[1:], np.float64)
    ok = reps[np.isfinite(reps)]
    se = float(np.std(ok, ddof=1)) if len(ok) >= 2 else math.nan
    lo, hi = math.nan, math.nan
    if len(ok) and 2 * len(ok) >= len(reps):
        lo, hi = (float(v) for v in np.quantile(ok, [(1 - level) / 2, (1 + level) / 2], method="linear"))
    return float(stat[0]), se, lo, hi, float(len(ok))


def evaluator_summary(crop_planes, joint_planes, crop_offsets, S, B, seed, level):
    """boot_summary of poco_amd/bootstrap.py for L labels: crop_planes [4 L, N] (per label the mean uncertainty, MPJPE, PA-MPJPE, V2V),
    joint_planes [2 L, N S] (per label the processed uncertainty and the pose distance), crop_offsets = the units over the N crop
    rows (None: every crop) -> [S, 5] in bootstrap.py's order."""
    crop_planes, joint_planes = np.asarray(crop_planes, np.float32), np.asarray(joint_planes, np.float32)
    L, N = crop_planes.shape[0] // 4, crop_planes.shape[1]
    off = offsets_of(N, crop_offsets)
    cp = [p for l in range(L) for p in ((4 * l, 4 * l), (4 * l + 1, 4 * l + 1), (4 * l, 4 * l + 1))]
    jp = [p for l in range(L) for p in ((2 * l, 2 * l), (2 * l + 1, 2 * l + 1), (2 * l, 2 * l + 1))]
    c = bootstrap(crop_planes, cp, off, B, seed)
    j = bootstrap(joint_planes, jp, off * S, B, seed)
    per = []
    for l in range(L):
        per.append([mean_of(c["out"], 1 + 4 * l + 1, 1000.0), mean_of(c["out"], 1 + 4 * l + 2, 1000.0), mean_of(c["out"], 1 + 4 * l + 3, 1000.0),
                    pearson_of(j["out"], j["center"], 2 * L, 2 * l + 1, 2 * l, 3 * l + 1, 3 * l, 3 * l + 2),
                    pearson_of(c["out"], c["center"], 4 * L, 4 * l, 4 * l + 1, 3 * l, 3 * l + 1, 3 * l + 2)])
    stats = list(per[0])
    for l in range(1, L):
        stats += per[l] + [x - y for x, y in zip(per[l], per[0])]
    return np.asarray([summarize(s, level) for s in stats])
