"""Calibrating the uncertainty (eval.py --calibrate OUT.npz, demo.py --calibration FILE): monotone maps from the
model's uncertainty to the error observed on a dataset with ground truth, fitted by isotonic regression on the device
(ops.isotonic, csrc/isotonic.hip) from an Evaluator's records, scored held out, written to a file and applied to the demo's `var`
(ops.calib_apply).  Nothing is read back but tables and scalars.  tests/calib_np.py restates the operators with plain loops.

The 28 maps, in this order: crop_mpjpe, crop_pampjpe, crop_v2v (key: the mean of the crop's 24 processed uncertainties, mode 0 of
Evaluator.rank_inputs; one sort, three segments), joint_all (mode 1, pooled over the selected joints), joint_0 .. joint_23 (key:
record column R_UNC + j, y: R_POSE + j).  The crop maps are in metres, as the records are; the joint maps in the unit of the
evaluator's per-joint pose distance."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np

MAP_NAMES = ("crop_mpjpe", "crop_pampjpe", "crop_v2v", "joint_all") + tuple(f"joint_{j}" for j in range(24))
MAP_UNITS = ("m", "m", "m") + ("pose distance",) * 25
SUMMARY_FIELDS = ("ence", "bias", "r2")
NPZ_KEYS = ("calib_names", "calib_offsets", "calib_knots", "calib_rows", "calib_dropped", "calib_summary", "calib_meta")
SPLITS = ("half", "parity", "none")
DEMO_MAP_IDS = tuple(range(4, 28)) + (0, 1, 2)          # the columns of demo.py's [n,27]: var's 24, then the crop key three times
NOT_WITH = ("segm", "likelihood", "cfg2", "tta", "sequences", "kp_refit", "visibility", "augment")


def flag_error(args):
    """The one sentence that refuses eval.py's --calibrate / --calib_split / --calib_bins where they cannot work, or None."""
    out, split, bins = (getattr(args, k, None) for k in ("calibrate", "calib_split", "calib_bins"))
    if not out:
        if split is not None or bins is not None:
            return "--calib_split and --calib_bins belong to --calibrate: they need --calibrate OUT.npz"
        return None
    if bins is not None and not 1 <= bins <= 1024:
        return f"--calib_bins must be in 1..1024, got {bins}"
    for flag in NOT_WITH:
        v = getattr(args, flag, None)
        if v not in (None, False):
            return f"--calibrate fits its maps to the records of the plain evaluation: it cannot be combined with --{flag}"
    for flag, v in sorted(vars(args).items()):
        if flag.startswith("aug_") and flag != "aug_seed" and v not in (None, False):
            return f"--calibrate fits its maps to the records of the plain evaluation: it cannot be combined with --{flag}"
    return None


def demo_flag_error(args):
    """The one sentence that refuses demo.py's --calibration where it cannot work, or None."""
    if not getattr(args, "calibration", None):
        return None
    if getattr(args, "cfg2", None):
        return "--calibration applies one model's maps: it cannot be combined with --cfg2 (a pair is not calibrated)"
    return None


def head_of(backbone: str) -> str:
    """'hrnet_w48_cls-cliff' -> 'cliff': the regressor head a config names behind its backbone."""
    return backbone.rsplit("-", 1)[1] if "-" in backbone else ""


def crop_key(var):
    """The crop key of a [n,24] tensor or array of processed uncertainties, bitwise what Evaluator.rank_inputs(0) yields for the same
    values: the 24 added in joint order in float64 starting from zero, divided by 24, rounded to float32 once."""
    import torch
    if torch.is_tensor(var):
        m = torch.zeros(var.shape[0], device=var.device, dtype=torch.float64)
        for j in range(24):
            m = m + var[:, j].double()
        return (m / 24.0).float()
    m = np.zeros(len(var), np.float64)
    for j in range(24):
        m = m + np.asarray(var)[:, j].astype(np.float64)
    return (m / 24.0).astype(np.float32)


def groups_of(ev, rows=None) -> list:
    """[(key [n], ys [E,n])] on the device for the 26 sorts behind the 28 maps, from the evaluator's records; rows = a device int64
    tensor of crop indices to keep (None: all)."""
    import torch
    from .evaluate import R_POSE, R_UNC
    key0, vals0 = ev.rank_inputs(0)
    key1, vals1 = ev.rank_inputs(1)
    rec = ev.copy_records()
    unc = rec[:, R_UNC:R_UNC + 24].t().contiguous()                       # contiguous planes [24,n]
    pose = rec[:, R_POSE:R_POSE + 24].t().contiguous()
    nsel = int(ev.sel.size)
    if rows is not None:
        jrows = (rows[:, None] * nsel + torch.arange(nsel, device=rows.device)[None, :]).reshape(-1)
        key0, vals0, key1, vals1, unc, pose = key0[rows], vals0[:, rows], key1[jrows], vals1[:, jrows], unc[:, rows], pose[:, rows]
    return [(key0, vals0), (key1, vals1)] + [(unc[j], pose[j][None]) for j in range(24)]


def finite_rows(key, ys):
    """(key, ys, dropped) with the rows whose key or any y is not finite taken out, and their number."""
    import torch
    ok = torch.isfinite(key) & torch.isfinite(ys).all(0)
    kept = int(ok.sum())
    if kept == key.shape[0]:
        return key.contiguous(), ys.contiguous(), 0
    return key[ok].contiguous(), ys[:, ok].contiguous(), int(key.shape[0]) - kept


class Fit:
    """The 28 maps of one set of rows: ONE ops.isotonic call over 28 segments.

        fit.offsets int32 [29], fit.knots float64 [B,4], fit.rows / fit.dropped int64 [28]     (host)
        fit.d_offsets, fit.d_knots, and the call's inputs and outputs key, y, order, seg, out    (device)"""

    def __init__(self, groups):
        import torch
        from . import ops
        keys, ys, orders, seg, rows, dropped = [], [], [], [0], [], []
        dev = groups[0][0].device
        base = 0
        for key, vals in groups:
            key, vals, gone = finite_rows(key, vals)
            n = int(key.shape[0])
            order = ops.rank_curve(key, None, 1)["order"] if n else torch.empty(0, device=dev, dtype=torch.int32)
            for e in range(vals.shape[0]):                                # E segments share the one sort
                keys.append(key); ys.append(vals[e]); orders.append(order + base)
                base += n
                seg.append(seg[-1] + n); rows.append(n); dropped.append(gone)
        assert len(rows) == len(MAP_NAMES)
        self.key, self.y, self.order = torch.cat(keys).contiguous(), torch.cat(ys).contiguous(), torch.cat(orders).contiguous()
        self.seg = np.asarray(seg, np.int64)
        self.out = ops.isotonic(self.key, self.y, self.order, self.seg)
        self.d_offsets = self.out["seg_blocks"]
        self.offsets = self.d_offsets.cpu().numpy()
        self.d_knots = self.out["knots"][:int(self.offsets[-1])].contiguous()
        self.knots = self.d_knots.cpu().numpy()
        self.rows, self.dropped = np.asarray(rows, np.int64), np.asarray(dropped, np.int64)


def score(fit: Fit, fit_groups, groups, bins: int) -> np.ndarray:
    """[28,3] float64: ENCE, bias and 1 - SSE / SSE_const of `fit`'s maps on the rows of `groups`.  Per map one ops.calib_apply, one
    ops.rank_curve keyed by the prediction with the error as its plane (the equal-count bins), and the sums of squares in float64 on
    the device; SSE_const is the SSE of the mean of the fitting rows' y."""
    import torch
    from . import ops
    from .ranking import cut_counts
    out = np.full((len(MAP_NAMES), 3), np.nan)
    dev = fit.d_knots.device
    m = 0
    for (fkey, fvals), (key, vals) in zip(fit_groups, groups):
        fkey, fvals, _ = finite_rows(fkey, fvals)
        key, vals, _ = finite_rows(key, vals)
        n = int(key.shape[0])
        for e in range(vals.shape[0]):
            if n and fit.rows[m]:
                pred = ops.calib_apply(key[:, None].contiguous(), torch.tensor([m], device=dev, dtype=torch.int32), fit.d_offsets,
                                       fit.d_knots)[:, 0].contiguous()
                err = vals[e].contiguous()
                cuts = ops.rank_curve(pred, err[None].contiguous(), bins)["cuts"]
                const = fvals[e].double().mean()
                sse = torch.stack([((err.double() - pred.double()) ** 2).sum(), ((err.double() - const) ** 2).sum()]).cpu().numpy()
                cuts = cuts.cpu().numpy()
                cnt = np.diff(cut_counts(n, bins)).astype(np.float64)
                full = cnt > 0
                mp, me = np.diff(cuts[0])[full] / cnt[full], np.diff(cuts[1])[full] / cnt[full]
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[m] = (np.mean(np.abs(mp - me) / mp), cuts[1][-1] / cuts[0][-1], 1.0 - sse[0] / sse[1])
            m += 1
    return out


def split_rows(n: int, split: str, dev):
    """The two parts of n crops as device int64 index tensors: first and second half by index, or even and odd indices."""
    import torch
    idx = torch.arange(n, device=dev)
    if split == "half":
        return idx[:n // 2], idx[n // 2:]
    if split == "parity":
        return idx[0::2], idx[1::2]
    raise ValueError(f"--calib_split must be one of {', '.join(SPLITS)}, got {split!r}")


def calibrate(ev, split: str = "half", bins: int = 20, meta: Optional[Dict[str, object]] = None) -> Dict[str, np.ndarray]:
    """The NPZ_KEYS arrays for an Evaluator that has been stepped: the table fitted on all rows, and calib_summary [28,3] = the mean
    of the two held-out directions (fit on one part, score on the other); NaN with split 'none' or fewer than two crops."""
    if split not in SPLITS:
        raise ValueError(f"--calib_split must be one of {', '.join(SPLITS)}, got {split!r}")
    fit = Fit(groups_of(ev))
    summary = np.full((len(MAP_NAMES), 3), np.nan)
    if split != "none" and ev.count >= 2:
        a, b = (groups_of(ev, r) for r in split_rows(ev.count, split, fit.d_knots.device))
        summary = 0.5 * (score(Fit(a), a, b, bins) + score(Fit(b), b, a, bins))
    meta = dict(meta or {})
    meta.update(split=split, bins=int(bins))
    lines = [f"{k}={v}" for k, v in meta.items()] + [f"unit:{n}={u}" for n, u in zip(MAP_NAMES, MAP_UNITS)]
    return {"calib_names": np.asarray(MAP_NAMES), "calib_offsets": fit.offsets.astype(np.int32), "calib_knots": fit.knots,
            "calib_rows": fit.rows, "calib_dropped": fit.dropped, "calib_summary": summary, "calib_meta": np.asarray(lines)}


def make_meta(dataset_name: str, kinematic: bool, backbone: str) -> Dict[str, object]:
    return {"dataset": dataset_name, "kinematic": int(bool(kinematic)), "backbone": backbone, "head": head_of(backbone)}


def save(path: str, res: Dict[str, np.ndarray]) -> None:
    import os
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:                                           # an open file: numpy appends no suffix to the name
        np.savez(f, **{k: res[k] for k in NPZ_KEYS})


def load(path: str) -> Dict[str, object]:
    """The arrays of a calibration file, checked, with `meta` as a dict of strings."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in NPZ_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path} is not a calibration file: it has no {', '.join(missing)}")
        res = {k: z[k] for k in NPZ_KEYS}
    if tuple(str(s) for s in res["calib_names"]) != MAP_NAMES:
        raise ValueError(f"{path}: calib_names are not the {len(MAP_NAMES)} maps this version writes")
    off, kn = res["calib_offsets"], res["calib_knots"]
    if off.shape != (len(MAP_NAMES) + 1,) or off[0] != 0 or np.any(np.diff(off) < 0) or kn.ndim != 2 or kn.shape != (int(off[-1]), 4):
        raise ValueError(f"{path}: calib_offsets and calib_knots do not describe {len(MAP_NAMES)} maps")
    res["meta"] = dict(str(s).split("=", 1) for s in res["calib_meta"])
    return res


def summary_lines(res) -> List[str]:
    """The report block of eval.py --calibrate: per map its rows, blocks and held-out scores."""
    off, summ = np.asarray(res["calib_offsets"]), np.asarray(res["calib_summary"], np.float64)
    out = ["Calibration maps: rows, dropped, blocks, held-out ENCE, bias (sum err / sum pred), 1 - SSE / SSE_const:"]
    for m, name in enumerate(MAP_NAMES):
        out.append(f"  {name}  {int(res['calib_rows'][m])}  {int(res['calib_dropped'][m])}  {int(off[m + 1] - off[m])}  "
                   f"{summ[m, 0]:.4f}  {summ[m, 1]:.4f}  {summ[m, 2]:.4f}")
    return out


def check_file(path: str, kinematic: bool, backbone: str) -> Dict[str, object]:
    """load(path), refused unless the file's kinematic flag and head are this run's."""
    res = load(path)
    meta = res["meta"]
    if meta.get("kinematic") != str(int(bool(kinematic))):
        raise ValueError(f"{path} was fitted with kinematic uncertainty {'on' if meta.get('kinematic') == '1' else 'off'}, this run has "
                         f"it {'on' if kinematic else 'off'}")
    if meta.get("head") != head_of(backbone):
        raise ValueError(f"{path} was fitted for the head {meta.get('head')!r}, this run's is {head_of(backbone)!r}")
    return res


class Calibration:
    """A calibration file on the device, for the demo: apply(var [n,24]) -> err_pose [n,24], err_mpjpe, err_pampjpe, err_v2v [n]
    (ONE ops.calib_apply call on [n,27]: the 24 columns, and the crop key three times)."""

    def __init__(self, path: str, device, kinematic: bool, backbone: str):
        import torch
        res = check_file(path, kinematic, backbone)
        self.device = device
        self.offsets = torch.from_numpy(np.ascontiguousarray(res["calib_offsets"], np.int32)).to(device)
        self.knots = torch.from_numpy(np.ascontiguousarray(res["calib_knots"], np.float64)).to(device)
        self.ids = torch.tensor(DEMO_MAP_IDS, device=device, dtype=torch.int32)

    def apply(self, var) -> Dict[str, np.ndarray]:
        import torch
        from . import ops
        v = torch.from_numpy(np.ascontiguousarray(var, np.float32)).to(self.device).reshape(-1, 24)
        if v.shape[0] == 0:
            return {"err_pose": np.zeros((0, 24), np.float32), **{k: np.zeros(0, np.float32) for k in ("err_mpjpe", "err_pampjpe", "err_v2v")}}
        key = crop_key(v)
        out = ops.calib_apply(torch.cat([v, key[:, None].expand(-1, 3)], 1).contiguous(), self.ids, self.offsets, self.knots).cpu().numpy()
        return {"err_pose": out[:, :24].copy(), "err_mpjpe": out[:, 24].copy(), "err_pampjpe": out[:, 25].copy(), "err_v2v": out[:, 26].copy()}
