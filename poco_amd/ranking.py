"""Rank-based measures of the uncertainty (eval.py --rank_metrics): sparsification curves, AUSE / AURG,
reliability and threshold tables, Spearman's rho.  The device does the sorting, the midranks and the prefix sums
(ops.rank_curve / ops.pearson64, csrc/rank_curve.hip); this module works on the (E + 1) x (K + 1) cut sums only, in float64 on the
host.  tests/rank_np.py restates every function here with plain loops.

Conventions: rows are sorted by ascending key (uncertainty); c_k = floor(k n / K) rows are kept at cut k; cuts[e][k] is the sum of
plane e over the c_k rows kept, plane 0 being the key itself.  Removing the least confident fraction k / K keeps c_{K-k} rows."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

CROP_METRICS = ("mpjpe", "pampjpe", "v2v")          # value planes of mode 0 (per crop), in record order
JOINT_METRICS = ("pose",)                           # value plane of mode 1 (per joint): the pose distance
RANK_SUMMARY_FIELDS = ("K", "spearman_pose", "spearman_mpjpe", "spearman_pampjpe", "spearman_v2v") + tuple(
    f"{a}_{m}" for m in CROP_METRICS + JOINT_METRICS for a in ("ause", "aurg"))
RANK_NPZ_KEYS = tuple(f"rank_{c}_{m}" for m in CROP_METRICS + JOINT_METRICS for c in ("spars", "oracle")) + (
    "rank_reliab_crop", "rank_reliab_joint", "rank_thresholds", "rank_summary")


def flag_error(args):
    """The one sentence that refuses --rank_metrics / --rank_bins where they cannot work, or None.  (A second model and --tta are
    refused by select.flag_error and tta.flag_error, which list the flag among those that read one model's single forward.)"""
    bins = getattr(args, "rank_bins", None)
    if not getattr(args, "rank_metrics", False):
        return "--rank_bins sets the cuts of --rank_metrics: it needs --rank_metrics" if bins is not None else None
    if bins is not None and not 1 <= bins <= 1024:
        return f"--rank_bins must be in 1..1024, got {bins}"
    for flag in ("segm", "likelihood"):
        if getattr(args, flag, False):
            return f"--rank_metrics ranks the records of the plain evaluation: it cannot be combined with --{flag}"
    return None


def cut_counts(n: int, K: int) -> np.ndarray:
    """c_k = floor(k n / K) for k = 0..K, in Python integers (no overflow), as int64."""
    return np.asarray([(k * int(n)) // int(K) for k in range(int(K) + 1)], np.int64)


def _ratio(num, den):
    """num / den elementwise in float64, NaN where den == 0."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def sparsification(cuts, n: int) -> np.ndarray:
    """cuts = one plane's K + 1 cut sums -> [K]: entry k = the mean of the plane over the c_{K-k} rows that stay when the fraction
    k / K with the largest keys is removed (entry 0 = the mean over all rows).  NaN where nothing stays (only if K > n)."""
    cuts = np.asarray(cuts, np.float64).reshape(-1)
    K = cuts.shape[0] - 1
    c = cut_counts(n, K)
    return _ratio(cuts[:0:-1], c[:0:-1])


def _area(diff) -> float:
    """Trapezoid area of `diff` [K] over the abscissae k / K; a segment with a NaN end is left out."""
    d = np.asarray(diff, np.float64)
    K = d.shape[0]
    seg = 0.5 * (d[:-1] + d[1:])
    return float(np.sum(seg[np.isfinite(seg)]) / K)


def ause(curve, oracle) -> float:
    """Area between the sparsification curve and the oracle's (rows ranked by the error itself), both divided by the all-rows mean
    curve[0].  0 for a ranking that orders the rows as the error does."""
    curve, oracle = np.asarray(curve, np.float64), np.asarray(oracle, np.float64)
    return _area((curve - oracle) / curve[0])


def aurg(curve) -> float:
    """Area between the random ranking's curve - the constant all-rows mean curve[0] - and the sparsification curve, divided by
    that mean.  Positive where the uncertainty ranks better than chance, negative where worse."""
    curve = np.asarray(curve, np.float64)
    return _area((curve[0] - curve) / curve[0])


def reliability(cuts, n: int) -> np.ndarray:
    """cuts [E+1,K+1] -> [K, 2+E]: per equal-count bin of ascending key its row count, its mean key and the mean of every value
    plane, from differences of adjacent cuts.  NaN means where a bin is empty (only if K > n)."""
    cuts = np.asarray(cuts, np.float64)
    K = cuts.shape[1] - 1
    cnt = np.diff(cut_counts(n, K)).astype(np.float64)
    return np.concatenate([cnt[:, None], _ratio(np.diff(cuts, axis=1), cnt[None, :]).T], axis=1)


def threshold_table(cut_keys, cuts, n: int) -> np.ndarray:
    """cut_keys [K+1], cuts [E+1,K+1] -> [K, 2+E]: for k = 1..K the kept fraction c_k / n, the largest key among the rows kept (the
    threshold that keeps exactly them, ties aside) and the mean of every value plane over the rows kept."""
    cuts = np.asarray(cuts, np.float64)
    K = cuts.shape[1] - 1
    c = cut_counts(n, K)[1:].astype(np.float64)
    return np.concatenate([(c / float(n))[:, None], np.asarray(cut_keys, np.float64)[1:, None], _ratio(cuts[1:, 1:], c[None, :]).T], axis=1)


class RankMetrics:
    """All rank-based measures of an Evaluator's records.

        rm = RankMetrics(evaluator, K=20)
        rm.result        # dict: the RANK_NPZ_KEYS arrays
        rm.lines()       # the report block of eval.py --rank_metrics

    Per mode one ops.rank_curve call keyed by the uncertainty (all value planes ride along) and one per value plane keyed by the
    error itself (the oracle ranking; plane 0 of that call is the error).  Spearman's rho is ops.pearson64 of the two calls' rank
    arrays, which stay on the device; only the cut sums, the cut keys and the rho scalars are read back."""

    def __init__(self, evaluator, K: int = 20):
        from . import ops
        import torch
        self.K = K = int(K)
        res: Dict[str, np.ndarray] = {}
        summ = {"K": float(K)}
        for mode, names, tag in ((0, CROP_METRICS, "crop"), (1, JOINT_METRICS, "joint")):
            key, vals = evaluator.rank_inputs(mode)
            n = int(key.shape[0])
            by_key = ops.rank_curve(key, vals, K)
            rhos = []
            cuts = by_key["cuts"].cpu().numpy()
            for e, name in enumerate(names):
                by_err = ops.rank_curve(vals[e], None, K)
                rhos.append(ops.pearson64(by_key["rank"], by_err["rank"]))
                curve, oracle = sparsification(cuts[e + 1], n), sparsification(by_err["cuts"][0].cpu().numpy(), n)
                res[f"rank_spars_{name}"], res[f"rank_oracle_{name}"] = curve, oracle
                summ[f"ause_{name}"], summ[f"aurg_{name}"] = ause(curve, oracle), aurg(curve)
            for name, rho in zip(names, torch.cat(rhos).cpu().numpy()):
                summ[f"spearman_{name}"] = float(rho)
            res[f"rank_reliab_{tag}"] = reliability(cuts, n)
            if mode == 0:
                res["rank_thresholds"] = threshold_table(by_key["cut_keys"].cpu().numpy(), cuts, n)
        res["rank_summary"] = np.asarray([summ[f] for f in RANK_SUMMARY_FIELDS], np.float64)
        self.result = res

    def lines(self) -> List[str]:
        return rank_lines(self.result)


def rank_lines(res) -> List[str]:
    """The report block: Spearman per joint and per crop, AUSE / AURG of the four errors, and the per-crop threshold table (errors
    in mm, as the headline numbers)."""
    s = dict(zip(RANK_SUMMARY_FIELDS, np.asarray(res["rank_summary"], np.float64)))
    out = [f"Uncert Error Spearman (per joint): {s['spearman_pose']}",
           f"Uncert Error Spearman (per crop, MPJPE): {s['spearman_mpjpe']}"]
    for label, m in (("MPJPE", "mpjpe"), ("PA-MPJPE", "pampjpe"), ("V2V", "v2v"), ("Pose distance", "pose")):
        out.append(f"AUSE / AURG {label}: {s['ause_' + m]} / {s['aurg_' + m]}")
    out.append(f"Keep fraction, uncertainty threshold, MPJPE, PA-MPJPE, V2V (mm) of the crops kept ({int(s['K'])} bins):")
    for frac, thr, a, p, v in np.asarray(res["rank_thresholds"], np.float64):
        out.append(f"  {frac:.4f}  {thr:.6g}  {1000.0 * a:.3f}  {1000.0 * p:.3f}  {1000.0 * v:.3f}")
    return out
