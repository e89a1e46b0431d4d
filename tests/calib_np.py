"""The yardstick of the calibration operators (include/poco_hip.h poco_op_isotonic / poco_op_calib_apply),
restated with plain loops, a stack and math.fsum.  It shares no code with csrc/isotonic.hip or poco_amd/calibrate.py, which only call the operators.

A segment is given as its rows in ascending order of canonical key (-0.0 = +0.0).  Units are the maximal runs of equal keys; the fit
pools neighbours whose means satisfy mean_left >= mean_right, decided exactly (integers on a common power-of-two scale); the values
are math.fsum of the block's rows over its rows."""
import math
from fractions import Fraction

import numpy as np


def canonical(key):
    k = np.asarray(key, np.float32).copy()
    k[k == 0] = 0.0
    return k


def units_of(keys):
    """[(first position, rows)] of the maximal runs of equal keys."""
    out, i, n = [], 0, len(keys)
    while i < n:
        j = i + 1
        while j < n and keys[j] == keys[i]:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def exact_ints(y):
    """The float32 values as Python integers on one common power-of-two scale: sums and comparisons of means on them are exact."""
    fr = [Fraction(float(v)) for v in y]
    scale = max([f.denominator for f in fr], default=1)                   # every denominator is a power of two
    return [int(f * scale) for f in fr]


def pava(keys, y):
    """Blocks [(first position, rows)] of the fit of one segment; keys ascending, y in the same order.  A stack of (start, rows,
    exact sum); two neighbours pool when mean_left >= mean_right, decided exactly by cross-multiplication of integers."""
    keys, iy = canonical(keys), exact_ints(np.asarray(y))
    stack = []
    for start, rows in units_of(keys):
        stack.append((start, rows, sum(iy[start:start + rows])))
        while len(stack) > 1:
            (s0, c0, a), (s1, c1, b) = stack[-2], stack[-1]
            if a * c1 >= b * c0:
                stack[-2:] = [(s0, c0 + c1, a + b)]
            else:
                break
    return [(s, c) for s, c, _ in stack]


def isotonic_segment(keys, y):
    """(block [n] = the first position of each position's block, fit [n] float64, knots [B,4] = lo key, hi key, value, rows,
    mag [n] = the block's sum of |y|)."""
    keys, y = canonical(keys), np.asarray(y)
    n = len(keys)
    block, fit, mag, knots = np.zeros(n, np.int64), np.zeros(n, np.float64), np.zeros(n, np.float64), []
    for start, rows in pava(keys, y):
        mine = [float(t) for t in y[start:start + rows]]
        v = math.fsum(mine) / rows
        block[start:start + rows] = start
        fit[start:start + rows] = v
        mag[start:start + rows] = math.fsum(abs(t) for t in mine)
        knots.append((float(keys[start]), float(keys[start + rows - 1]), v, float(rows)))
    return block, fit, np.asarray(knots, np.float64).reshape(-1, 4), mag


def isotonic(key, y, order, seg_offsets):
    """The whole operator: dict(block, fit, seg_blocks, knots, mag) with mag [N] = the block's sum of |y| (the value bound's scale)."""
    key, y, order = np.asarray(key, np.float32), np.asarray(y, np.float32), np.asarray(order, np.int64)
    N, S = len(order), len(seg_offsets) - 1
    block, fit, mag = np.zeros(N, np.int32), np.zeros(N, np.float64), np.zeros(N, np.float64)
    seg_blocks, knots = [0], []
    for s in range(S):
        a, b = int(seg_offsets[s]), int(seg_offsets[s + 1])
        rows = order[a:b]
        blk, f, kn, mg = isotonic_segment(key[rows], y[rows])
        block[a:b], fit[a:b], mag[a:b] = blk + a, f, mg
        knots.append(kn)
        seg_blocks.append(seg_blocks[-1] + len(kn))
    return dict(block=block, fit=fit, seg_blocks=np.asarray(seg_blocks, np.int32),
                knots=np.concatenate(knots, axis=0) if knots else np.zeros((0, 4)), mag=mag)


def exact_fit(keys, y):
    """Brute force over every partition of the units into consecutive blocks, on Fractions: the one whose block means increase
    strictly and none of whose blocks splits into a left part with a mean strictly below the right part's.  Returns [(start, rows)]."""
    keys, y = canonical(keys), np.asarray(y)
    units = units_of(keys)
    U = len(units)
    if U == 0:
        return []
    fr = [Fraction(float(v)) for v in y]
    found = []
    for mask in range(1 << (U - 1)):                                      # bit i set: a block boundary after unit i
        blocks, first = [], 0
        for i in range(U):
            if i == U - 1 or (mask >> i) & 1:
                blocks.append((first, i))
                first = i + 1
        ok, prev = True, None
        for u0, u1 in blocks:
            p0, p1 = units[u0][0], units[u1][0] + units[u1][1]
            mean = sum(fr[p0:p1], Fraction(0)) / (p1 - p0)
            if prev is not None and not prev < mean:
                ok = False
            prev = mean
            for cut in range(u0 + 1, u1 + 1):                             # a split in front of unit `cut`
                pc = units[cut][0]
                if sum(fr[p0:pc], Fraction(0)) / (pc - p0) < sum(fr[pc:p1], Fraction(0)) / (p1 - pc):
                    ok = False
        if ok:
            found.append([(units[u0][0], units[u1][0] + units[u1][1] - units[u0][0]) for u0, u1 in blocks])
    assert len(found) == 1, found
    return found[0]


def margins(keys, y):
    """(gap, split) of one segment's fit, exactly: the smallest difference of adjacent block means and the smallest POSITIVE
    left-minus-right mean difference over every split of every block at a unit boundary, each relative to the larger of the two
    means in magnitude; inf where there is none."""
    keys, iy = canonical(keys), exact_ints(np.asarray(y))
    pre = [0]
    for v in iy:
        pre.append(pre[-1] + v)
    heads = [u[0] for u in units_of(keys)]
    gap = split = math.inf
    prev, hi = None, 0
    for start, rows in pava(keys, y):
        end = start + rows
        mean = Fraction(pre[end] - pre[start], rows)
        if prev is not None:
            gap = min(gap, float((mean - prev) / max(abs(mean), abs(prev))))
        prev = mean
        while hi < len(heads) and heads[hi] <= start:
            hi += 1
        while hi < len(heads) and heads[hi] < end:
            c = heads[hi]
            left, right = Fraction(pre[c] - pre[start], c - start), Fraction(pre[end] - pre[c], end - c)
            if left > right:
                split = min(split, float((left - right) / max(abs(left), abs(right))))
            hi += 1
    return gap, split


def apply_map(knots, x):
    """f(x) of one map (knots [B,4]) at one float32 x, as a float32."""
    x = np.float32(x)
    B = len(knots)
    if B == 0 or np.isnan(x):
        return np.float32(np.nan)
    xd = float(x)
    if xd <= knots[0][0]:
        return np.float32(knots[0][2])
    if xd >= knots[B - 1][1]:
        return np.float32(knots[B - 1][2])
    first, last = 0, B - 1                                                # the last block whose lowest key is <= x
    while first < last:
        mid = (first + last + 1) // 2
        if float(knots[mid][0]) <= xd:
            first = mid
        else:
            last = mid - 1
    b = first
    lo, hi, v = float(knots[b][0]), float(knots[b][1]), float(knots[b][2])
    if lo <= xd <= hi:
        return np.float32(v)
    assert b + 1 < B and hi < xd < float(knots[b + 1][0]), "the knots do not cover x"
    lo_n, v_n = float(knots[b + 1][0]), float(knots[b + 1][2])
    return np.float32(v + (v_n - v) * ((xd - hi) / (lo_n - hi)))


def calib_apply(x, map_ids, map_offsets, knots):
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape, np.float32)
    for r in range(x.shape[0]):
        for c in range(x.shape[1]):
            m = int(map_ids[c])
            out[r, c] = apply_map(knots[int(map_offsets[m]):int(map_offsets[m + 1])], x[r, c])
    return out


# ---- the patterns of the tests: (key, y) of one segment of n rows, rows already in ascending key order ---------------------------------
PATTERNS = ("increasing", "decreasing", "all_equal", "one_unit", "ties_straddle", "saw_T", "saw_Tp1", "saw_Tm1", "staircase", "huge_front",
            "huge_back", "halves", "small_ints", "eval_like")
FLOAT_PATTERNS = ("staircase", "eval_like")                               # the others are integer-valued: their sums are exact


def pattern(name, n, T, seed=0):
    """Seeded inputs of one segment.  Every pattern but the two FLOAT_PATTERNS takes small integer values in float32, whose sums
    are exact in float64, so that exact ties pool by the convention on every machine."""
    r = np.random.default_rng([seed, n, PATTERNS.index(name)])
    i = np.arange(n)
    key = (i * 0.25).astype(np.float32)                                   # distinct, ascending, exact
    if name == "increasing":
        y = i % 4096 + 4096 * (i // 4096)
    elif name == "decreasing":
        y = n - i
    elif name == "all_equal":
        y = np.full(n, 3)
    elif name == "one_unit":
        key, y = np.full(n, 1.5, np.float32), r.integers(0, 8, n)
    elif name == "ties_straddle":                                         # tie groups over every multiple of 64 and of the tile
        grp = np.zeros(n, np.int64)
        cuts = np.unique(np.concatenate([np.arange(0, n, 64), np.arange(0, n, T)]))
        bounds = sorted(set(np.clip(np.concatenate([cuts - 3, cuts + 5]), 0, n).tolist() + [0, n]))
        for g, (a, b) in enumerate(zip(bounds, bounds[1:])):
            grp[a:b] = g
        key, y = (grp * 0.5).astype(np.float32), r.integers(0, 8, n) + grp // 3
    elif name in ("saw_T", "saw_Tp1", "saw_Tm1"):
        period = T + {"saw_T": 0, "saw_Tp1": 1, "saw_Tm1": -1}[name]
        y = i % period
    elif name == "staircase":
        y = (i // 37) * 0.5 + r.uniform(0.0, 1.0, n) + 1.0
    elif name == "huge_front":
        y = i % 5 + 1
        if n:
            y[0] = 1 << 22
    elif name == "huge_back":
        y = i.copy()
        if n:
            y[-1] = 1 << 22
    elif name == "halves":
        y = np.where(i < n // 2, i + n, i - n // 2)
    elif name == "small_ints":
        y = r.integers(0, 8, n)
    elif name == "eval_like":                                             # an error that rises with the key under heavy noise
        key = np.sort(r.gamma(2.0, 0.1, n)).astype(np.float32)
        y = (50.0 + 200.0 * key) * r.gamma(2.0, 0.5, n) + 1.0
    else:
        raise KeyError(name)
    return key, np.asarray(y, np.float64).astype(np.float32)
