"""Confidence intervals for eval.py's numbers (eval.py --bootstrap B): a cluster bootstrap whose unit is the
crop or the track, never the row or the (crop, joint) pair - the 24 joints of a crop share the crop and the rows of 3DPW are the
consecutive frames of about 60 clips.  The resampling runs on the device (ops.bootstrap, csrc/bootstrap.hip) on the planes that
Evaluator.rank_inputs hands out without a read-back; this module forms the statistics in float64 numpy from the [B + 1, M] moment
sums, which with the planes' centres are all that is read back.  tests/boot_np.py restates operator and statistics with plain loops."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

UNITS = ("crop", "track")
NPZ_KEYS = ("boot_names", "boot_summary", "boot_spec")          # and boot_replicates with save_results
SUMMARY_FIELDS = ("point", "se", "lo", "hi", "valid")          # the columns of boot_summary
STAT_NAMES = ("MPJPE", "PA-MPJPE", "V2V (mm)", "Uncert Error Correlation", "Corr(crop uncertainty, MPJPE)")
MAX_LABELS = 4                                                  # 4 crop planes per label, ops.BOOT_MAX_PLANES = 16
MAX_SEED = 1 << 53                                              # boot_spec holds the seed as a float64


@dataclass(frozen=True)
class BootSpec:
    """B replicates; unit = "crop" or "track" (sequences.group_tracks); level of the percentile interval; seed of the draws."""
    B: int
    unit: str = "crop"
    level: float = 0.95
    seed: int = 0

    def __post_init__(self):
        from . import ops
        if not (isinstance(self.B, (int, np.integer)) and 1 <= self.B <= ops.BOOT_MAX_B):
            raise ValueError(f"--bootstrap: B must be in 1..{ops.BOOT_MAX_B}, got {self.B!r}")
        if self.unit not in UNITS:
            raise ValueError(f"--boot_unit must be one of {UNITS}, got {self.unit!r}")
        if not (isinstance(self.level, float) and 0.0 < self.level < 1.0):
            raise ValueError(f"--boot_level must be in (0, 1), got {self.level!r}")
        if not (isinstance(self.seed, (int, np.integer)) and 0 <= self.seed < MAX_SEED):
            raise ValueError(f"--boot_seed must be in 0..2^53-1, got {self.seed!r}")


def flag_error(args) -> Optional[str]:
    """eval.py: what cannot work with --bootstrap, and --boot_* without it; None when all is well."""
    B = getattr(args, "bootstrap", None)
    if B is None:
        for flag in ("boot_unit", "boot_level", "boot_seed"):
            if getattr(args, flag, None) is not None:
                return f"--{flag} needs --bootstrap"
        return None
    for flag, on in (("--segm", bool(getattr(args, "segm", False))), ("--likelihood", bool(getattr(args, "likelihood", False))),
                     ("--sequences", bool(getattr(args, "sequences", False))), ("--visibility", bool(getattr(args, "visibility", False)))):
        if on:
            return f"--bootstrap cannot be combined with {flag}"
    try:
        spec_from_args(args)
    except ValueError as e:
        return str(e)
    return None


def spec_from_args(args) -> Optional[BootSpec]:
    """The BootSpec of --bootstrap / --boot_unit / --boot_level / --boot_seed, or None without the flag (ValueError: out of range)."""
    if getattr(args, "bootstrap", None) is None:
        return None
    opt = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)   # noqa: E731
    return BootSpec(int(args.bootstrap), str(opt("boot_unit", "crop")), float(opt("boot_level", 0.95)), int(opt("boot_seed", 0)))


def crop_pairs(L: int) -> List[Tuple[int, int]]:
    """Per label l the planes 4l .. 4l+3 = mean uncertainty, MPJPE, PA-MPJPE, V2V; its pairs 3l .. 3l+2 = (u, u), (e, e), (u, e)."""
    return [p for l in range(L) for p in ((4 * l, 4 * l), (4 * l + 1, 4 * l + 1), (4 * l, 4 * l + 1))]


def joint_pairs(L: int) -> List[Tuple[int, int]]:
    """Per label l the planes 2l, 2l+1 = processed uncertainty, pose distance; its pairs 3l .. 3l+2 = (u, u), (d, d), (u, d)."""
    return [p for l in range(L) for p in ((2 * l, 2 * l), (2 * l + 1, 2 * l + 1), (2 * l, 2 * l + 1))]


def _mean(out: np.ndarray, col: int) -> np.ndarray:
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1000.0 * out[:, col] / out[:, 0]


def _pearson(out: np.ndarray, center: np.ndarray, E: int, a: int, b: int, kaa: int, kbb: int, kab: int) -> np.ndarray:
    """Pearson's r of planes a and b in every row of the moment sums: the raw sums are shifted to the centre the products were formed
    about, then r = cov / sqrt(var var).  NaN where a variance is not positive or no row was drawn."""
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = out[:, 0]
        sa, sb = out[:, 1 + a] - cnt * center[a], out[:, 1 + b] - cnt * center[b]
        vaa, vbb = out[:, 1 + E + kaa] - sa * sa / cnt, out[:, 1 + E + kbb] - sb * sb / cnt
        vab = out[:, 1 + E + kab] - sa * sb / cnt
        ok = (cnt > 0) & (vaa > 0) & (vbb > 0)
        return np.where(ok, vab / np.sqrt(np.where(ok, vaa * vbb, 1.0)), np.nan)


def statistics(labels: Sequence[str], crop_out, crop_center, joint_out, joint_center):
    """-> (names, stats [S, B + 1]) from the two calls' moment sums: per label the five STAT_NAMES, and for every label after the
    first their differences to the first label's, replicate by replicate (the calls share their draws: a paired bootstrap)."""
    L = len(labels)
    crop_out, joint_out = np.asarray(crop_out, np.float64), np.asarray(joint_out, np.float64)
    per = []
    for l in range(L):
        per.append([_mean(crop_out, 1 + 4 * l + 1), _mean(crop_out, 1 + 4 * l + 2), _mean(crop_out, 1 + 4 * l + 3),
                    _pearson(joint_out, joint_center, 2 * L, 2 * l + 1, 2 * l, 3 * l + 1, 3 * l, 3 * l + 2),
                    _pearson(crop_out, crop_center, 4 * L, 4 * l, 4 * l + 1, 3 * l, 3 * l + 1, 3 * l + 2)])
    names = [f"{labels[0]} {s}".strip() for s in STAT_NAMES]                  # a single unnamed label: the bare names
    stats = list(per[0])
    for l in range(1, L):
        names += [f"{labels[l]} {s}" for s in STAT_NAMES] + [f"{labels[l]} - {labels[0]} {s}" for s in STAT_NAMES]
        stats += per[l] + [x - y for x, y in zip(per[l], per[0])]
    return names, np.stack(stats)


def summarize(stat: np.ndarray, level: float) -> Tuple[float, float, float, float, float]:
    """One statistic [B + 1] -> (point estimate = entry 0, bootstrap standard error = std with ddof 1 of the valid replicates,
    percentile interval, number of valid replicates).  A NaN or infinite replicate is dropped and counted; with fewer than half of
    the replicates valid the interval is NaN."""
    reps = stat[1:]
    ok = reps[np.isfinite(reps)]
    se = float(np.std(ok, ddof=1)) if len(ok) >= 2 else math.nan
    lo = hi = math.nan
    if len(ok) and 2 * len(ok) >= len(reps):
        lo, hi = (float(v) for v in np.quantile(ok, [(1.0 - level) / 2.0, (1.0 + level) / 2.0], method="linear"))
    return float(stat[0]), se, lo, hi, float(len(ok))


def bootstrap_planes(labels: Sequence[str], crop_planes: torch.Tensor, joint_planes: torch.Tensor, S: int, spec: BootSpec,
                     unit_offsets=None, save_replicates: bool = False) -> Dict[str, object]:
    """The two ops.bootstrap calls and the statistics: crop_planes fp32 [4 L, N] and joint_planes fp32 [2 L, N S] on the device, rows
    already in unit-major order; unit_offsets int32 [U + 1] over the N crop rows (None: every crop is a unit).  -> the NPZ_KEYS
    arrays (and boot_replicates [B, S] with save_replicates)."""
    from . import ops
    L, N = len(labels), int(crop_planes.shape[1])
    off_c = None if unit_offsets is None else np.asarray(unit_offsets, np.int64)
    off_j = (np.arange(N + 1, dtype=np.int64) if off_c is None else off_c) * int(S)
    c = ops.bootstrap(crop_planes, crop_pairs(L), None if off_c is None else off_c.astype(np.int32), spec.B, spec.seed)
    j = ops.bootstrap(joint_planes, joint_pairs(L), off_j.astype(np.int32), spec.B, spec.seed)
    names, stats = statistics(labels, c["out"].cpu().numpy(), c["center"].cpu().numpy(), j["out"].cpu().numpy(), j["center"].cpu().numpy())
    U = N if off_c is None else len(off_c) - 1
    res = {"boot_names": np.asarray(names), "boot_summary": np.asarray([summarize(s, spec.level) for s in stats], np.float64),
           "boot_spec": np.asarray([spec.B, U, spec.level, spec.seed], np.float64)}
    if save_replicates:
        res["boot_replicates"] = np.ascontiguousarray(stats[:, 1:].T)
    return res


def bootstrap_evaluators(evaluators, spec: BootSpec, imgname=None, person_id=None, save_replicates: bool = False) -> Dict[str, object]:
    """evaluators = [(label, Evaluator), ...] after their last step, all over the same N crops and selected joints.  Stacks their
    rank_inputs(0) planes (mean uncertainty, MPJPE, PA-MPJPE, V2V) for one ops.bootstrap call and their rank_inputs(1) planes
    (processed uncertainty and pose distance per selected joint, crop-major; units = the crops' |sel| rows) for a second one with the
    same seed and unit count, hence the same draws.  spec.unit == "track": the rows are gathered track-major on the device with
    sequences.group_tracks' order (imgname is needed; ValueError from group_tracks) and the units are the tracks.  The records are
    only read."""
    evaluators = list(evaluators)
    if not 1 <= len(evaluators) <= MAX_LABELS:
        raise ValueError(f"bootstrap_evaluators takes 1..{MAX_LABELS} evaluators, got {len(evaluators)}")
    labels = [str(label) for label, _ in evaluators]
    evs = [ev for _, ev in evaluators]
    N, sel = evs[0].count, evs[0].sel
    if N < 1 or sel.size < 1:
        raise ValueError("bootstrap_evaluators needs at least one stepped crop and one selected joint")
    if any(ev.count != N or not np.array_equal(ev.sel, sel) for ev in evs):
        raise ValueError("bootstrap_evaluators: the evaluators must hold the same number of crops and the same selected joints")
    S = int(sel.size)
    crop, joint = [], []
    for ev in evs:
        key, vals = ev.rank_inputs(0)
        crop += [key[None], vals]
        key, vals = ev.rank_inputs(1)
        joint += [key[None], vals]
    crop_planes, joint_planes = torch.cat(crop).contiguous(), torch.cat(joint).contiguous()
    offsets = None
    if spec.unit == "track":
        from .sequences import group_tracks
        if imgname is None:
            raise ValueError("--boot_unit track groups the rows by their image names: imgname is needed")
        g = group_tracks(imgname, person_id)
        if len(g["order"]) != N:
            raise ValueError(f"--boot_unit track: {len(g['order'])} image names for {N} crops")
        order = torch.from_numpy(g["order"].astype(np.int64)).to(crop_planes.device)
        rows = (order[:, None] * S + torch.arange(S, device=order.device)[None]).reshape(-1)
        crop_planes = crop_planes.index_select(1, order).contiguous()
        joint_planes = joint_planes.index_select(1, rows).contiguous()
        offsets = g["offsets"]
    return bootstrap_planes(labels, crop_planes, joint_planes, S, spec, offsets, save_replicates)


def report_lines(res: Dict[str, object]) -> List[str]:
    """One line per statistic: name  point  +- se  [lo, hi]  (valid/B), under a heading that names B, the unit and the level."""
    B, U, level, seed = res["boot_spec"]
    lines = [f"Bootstrap: {int(B)} replicates of {int(U)} units, {100.0 * level:g} % percentile intervals, seed {int(seed)}"]
    for name, (point, se, lo, hi, valid) in zip(res["boot_names"], res["boot_summary"]):
        lines.append(f"{name}  {point:.4f}  +- {se:.4f}  [{lo:.4f}, {hi:.4f}]  ({int(valid)}/{int(B)})")
    return lines
