"""The yardstick of tests/test_rank_*.py: poco_op_rank_curve, poco_op_pearson64 and poco_amd/ranking.py restated with plain loops
in float64 (include/poco_hip.h).  Nothing here is imported from the package on purpose."""
from __future__ import annotations

import math
import struct

import numpy as np


def canonical(key) -> np.ndarray:
    """float32 keys with -0.0 -> +0.0 and every NaN -> the one positive quiet NaN 0x7fc00000."""
    bits = np.ascontiguousarray(key, np.float32).view(np.uint32).copy()
    for i in range(bits.shape[0]):
        b = int(bits[i])
        if (b & 0x7fffffff) > 0x7f800000:
            b = 0x7fc00000
        if b == 0x80000000:
            b = 0
        bits[i] = b
    return bits.view(np.float32)


def sort_image(key) -> np.ndarray:
    """The order-preserving uint32 image of the canonical keys: ~bits for a negative key, bits | 0x80000000 otherwise."""
    bits = canonical(key).view(np.uint32).astype(np.uint64)
    return np.asarray([(~int(b)) & 0xffffffff if int(b) & 0x80000000 else int(b) | 0x80000000 for b in bits], np.uint64)


def stable_order(key) -> np.ndarray:
    """Ascending by the image, equal images in row order: what numpy.argsort(kind="stable") gives on the keys (NaN last)."""
    img = sort_image(key)
    return np.asarray(sorted(range(len(img)), key=lambda i: (int(img[i]), i)), np.int32)


def midranks(key, order=None) -> np.ndarray:
    """1-based ranks, rows with equal canonical keys share the mean of their sorted positions.  order = stable_order(key), if the
    caller has it already."""
    img = sort_image(key)
    order = stable_order(key) if order is None else order
    n = len(order)
    rank = np.zeros(n, np.float64)
    lo = 0
    while lo < n:
        hi = lo
        while hi + 1 < n and img[order[hi + 1]] == img[order[lo]]:
            hi += 1
        for p in range(lo, hi + 1):
            rank[order[p]] = 0.5 * (lo + hi) + 1.0
        lo = hi + 1
    return rank


def fsum(x) -> float:
    """math.fsum, with the answers IEEE addition gives where it refuses: NaN for a NaN term or infinities of both signs."""
    x = np.asarray(x, np.float64)
    if np.isnan(x).any() or (np.isposinf(x).any() and np.isneginf(x).any()):
        return float("nan")
    return math.fsum(x)


def cut_counts(n: int, K: int):
    return [(k * n) // K for k in range(K + 1)]


def cut_sums(key, vals, K: int, order=None):
    """(cuts [E+1][K+1] exact to one rounding (math.fsum), abs [E+1][K+1] = the same sums of absolute values, cut_keys [K+1]).
    order = stable_order(key), if the caller has it already."""
    ck = canonical(key)
    order = stable_order(key) if order is None else order
    n = len(order)
    planes = [ck.astype(np.float64)] + [np.asarray(v, np.float32).astype(np.float64) for v in ([] if vals is None else vals)]
    c = cut_counts(n, K)
    cuts = np.zeros((len(planes), K + 1), np.float64)
    mags = np.zeros_like(cuts)
    for e, pl in enumerate(planes):
        s = pl[order]
        for k in range(K + 1):
            cuts[e, k] = fsum(s[:c[k]])
            mags[e, k] = fsum(np.abs(s[:c[k]]))
    cut_keys = np.asarray([ck[order[max(c[k], 1) - 1]] for k in range(K + 1)], np.float32)
    return cuts, mags, cut_keys


def bits32(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def pearson(x, y) -> float:
    """Pearson's r in float64 with exactly rounded sums, clipped to [-1, 1]; NaN where either side is constant."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if np.all(x == x[0]) or np.all(y == y[0]):
        return float("nan")
    mx, my = math.fsum(x) / len(x), math.fsum(y) / len(y)
    dx, dy = x - mx, y - my
    r = math.fsum(dx * dy) / (math.sqrt(math.fsum(dx * dx)) * math.sqrt(math.fsum(dy * dy)))
    return max(-1.0, min(1.0, r))


def spearman(a, b) -> float:
    return pearson(midranks(a), midranks(b))


# ---- the host side (poco_amd/ranking.py) with plain loops --------------------------------------------------------------------------
def sparsification(cuts_e, n: int):
    K = len(cuts_e) - 1
    c = cut_counts(n, K)
    return np.asarray([cuts_e[K - k] / c[K - k] if c[K - k] else float("nan") for k in range(K)], np.float64)


def area(diff) -> float:
    K = len(diff)
    total = 0.0
    for k in range(K - 1):
        seg = 0.5 * (diff[k] + diff[k + 1])
        if math.isfinite(seg):
            total += seg
    return total / K


def ause(curve, oracle) -> float:
    return area([(a - b) / curve[0] for a, b in zip(curve, oracle)])


def aurg(curve) -> float:
    return area([(curve[0] - a) / curve[0] for a in curve])


def reliability(cuts, n: int):
    cuts = np.asarray(cuts, np.float64)
    K = cuts.shape[1] - 1
    c = cut_counts(n, K)
    out = np.full((K, 1 + cuts.shape[0]), np.nan)
    for b in range(K):
        cnt = c[b + 1] - c[b]
        out[b, 0] = cnt
        for e in range(cuts.shape[0]):
            if cnt:
                out[b, 1 + e] = (cuts[e, b + 1] - cuts[e, b]) / cnt
    return out


def threshold_table(cut_keys, cuts, n: int):
    cuts = np.asarray(cuts, np.float64)
    K = cuts.shape[1] - 1
    c = cut_counts(n, K)
    out = np.full((K, 1 + cuts.shape[0]), np.nan)
    for k in range(1, K + 1):
        out[k - 1, 0] = c[k] / n
        out[k - 1, 1] = float(cut_keys[k])
        for e in range(1, cuts.shape[0]):
            if c[k]:
                out[k - 1, 1 + e] = cuts[e, k] / c[k]
    return out


def float_from_bits(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b))[0]
