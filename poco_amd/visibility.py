"""Per-joint visibility of the ground-truth body (eval.py --visibility): how much of joint j's body part can be seen in the crop, what
hides the rest, and how the model's per-joint uncertainty and error follow it - the paper's central claim, stated per joint.

Per batch, on the evaluator's stream: the ground-truth mesh is placed in the crop as eval.py --segm places it (ops.estimate_translation
on the 24 ground-truth keypoints) and ops.part_visibility (csrc/part_visibility.hip) counts, per crop and body part, the pixels of the
part in a window around the crop (total), of those inside the crop (area), of those in front of the rest of the body (front) and of
those no synthetic occluder touched (seen; the mask comes out of the dataset crop's launch, poco_dataset_crop_occ_mask).  The default
part table gives every vertex to the joint with its largest skinning weight, so part p is joint p; a licensed table (--part_mapping)
has the same 24 names.  The [N,24,4] counts stay on the device until finish(); the statistics are N x 24 numbers in float64 on the
host.  DESIGN.md section 30 has the contract; tests/visibility_np.py restates the operator and the statistics.

    vis       = seen  / total      what is visible of the part, of what the window holds
    vis_frame = area  / total      what the box does not cut off     (truncation)
    vis_self  = front / area       what the body does not hide       (self-occlusion)
    vis_obj   = seen  / front      what the occluders do not hide    (object occlusion)

vis is the product of the three where all are defined; each is NaN where its denominator is 0, and such entries are left out of every
statistic and counted."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from ._lib import PocoHipError

NUM_JOINTS = 24
COMPONENTS = ("vis", "vis_frame", "vis_self", "vis_obj")
DATASET_KEYS = ("pose", "shape", "part")
SUMMARY_NAMES = ("vis_mean", "pearson", "spearman", "pearson_frame", "spearman_frame", "pearson_self", "spearman_self", "pearson_obj",
                 "spearman_obj", "pearson_err", "spearman_err", "valid", "invalid", "margin", "bins")
NPZ_KEYS = ("vis_counts", "vis", "vis_summary", "vis_joint", "vis_bins")


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def flag_error(args) -> Optional[str]:
    """The one sentence that refuses --visibility / --vis_margin / --vis_bins where they cannot work, or None."""
    margin, bins = getattr(args, "vis_margin", None), getattr(args, "vis_bins", None)
    if not getattr(args, "visibility", False):
        for name, v in (("vis_margin", margin), ("vis_bins", bins)):
            if v is not None:
                return f"--{name} belongs to --visibility: it needs --visibility"
        return None
    if getattr(args, "cfg2", None) or getattr(args, "ckpt2", None):
        return "--visibility reads one model's outputs: it cannot be combined with --cfg2 / --ckpt2"
    if getattr(args, "tta", None) is not None:
        return "--visibility reads one forward's outputs: it cannot be combined with --tta"
    if getattr(args, "sequences", False):
        return "--sequences cannot be combined with --visibility"
    if getattr(args, "rank_metrics", False):
        return "--rank_metrics ranks the records of the plain evaluation: it cannot be combined with --visibility"
    if getattr(args, "likelihood", False):
        return "--visibility reads the records of the plain evaluation: it cannot be combined with --likelihood"
    if bins is not None and not 2 <= int(bins) <= 20:
        return f"--vis_bins must be in 2..20, got {bins}"
    if margin is not None and int(margin) < 0:
        return f"--vis_margin must be in 0..res (the crop's side), got {margin}"
    return None


def check_dataset_keys(files) -> None:
    """The dataset needs pose, shape and part (ValueError names the missing keys, as --segm does)."""
    missing = [k for k in DATASET_KEYS if k not in set(files)]
    if missing:
        raise ValueError(f"--visibility needs {missing} in the dataset (ground-truth SMPL parameters and the 24 2-D keypoints place the "
                         "mesh in the crop)")


# ---- statistics (host, float64) ------------------------------------------------------------------------------------------------------
def ratios(counts) -> Dict[str, np.ndarray]:
    """counts [N,24,4] = (total, area, front, seen) -> the four float64 [N,24] ratios, NaN where the denominator is 0."""
    c = np.asarray(counts, np.float64).reshape(-1, NUM_JOINTS, 4)

    def div(a, b):
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=b > 0)
        return out
    total, area, front, seen = (c[:, :, k] for k in range(4))
    return {"vis": div(seen, total), "vis_frame": div(area, total), "vis_self": div(front, area), "vis_obj": div(seen, front)}


def pearson(x, y) -> float:
    """Pearson's r in float64; NaN with fewer than two entries or when either side is constant."""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    if x.size < 2:
        return float("nan")
    dx, dy = x - x.mean(), y - y.mean()
    den = np.sqrt((dx * dx).sum() * (dy * dy).sum())
    return float((dx * dy).sum() / den) if den > 0 else float("nan")


def average_ranks(x) -> np.ndarray:
    """1-based ranks in float64, equal values sharing the mean of their positions."""
    x = np.asarray(x, np.float64).reshape(-1)
    _, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    last = np.cumsum(cnt).astype(np.float64)
    return (last - (cnt - 1) / 2.0)[inv]


def spearman(x, y) -> float:
    """Spearman's rho = Pearson's r of the average ranks."""
    return pearson(average_ranks(x), average_ranks(y))


def statistics(counts, uncert, err, bins: int = 5) -> Dict[str, object]:
    """counts [N,24,4], uncert and err [N,24] (the per-joint uncertainty and error of Evaluator.finish: corr_y and corr_x) -> the
    four ratio arrays and
      mean [24], mean_all       mean vis per joint and over all valid entries
      corr                      {component: (Pearson, Spearman)} of (1 - component, uncertainty), pooled over the component's valid entries
      corr_joint [24,2]         (Pearson, Spearman) of (1 - vis, uncertainty) per joint
      corr_err                  (Pearson, Spearman) of (1 - vis, error), pooled
      bins [K,3]                per equal-width bin of vis over [0, 1] (the last one closed): entries, mean uncertainty, mean error
      valid, invalid            entries with total > 0, and without
    An entry whose ratio is NaN is left out of every statistic of that ratio."""
    bins = int(bins)
    if not 2 <= bins <= 20:
        raise ValueError(f"bins must be in 2..20, got {bins}")
    r = ratios(counts)
    n = r["vis"].shape[0]
    u = np.asarray(uncert, np.float64).reshape(n, NUM_JOINTS)
    e = np.asarray(err, np.float64).reshape(n, NUM_JOINTS)
    ok = np.isfinite(r["vis"])
    out: Dict[str, object] = dict(r)
    out["valid"], out["invalid"] = int(ok.sum()), int((~ok).sum())
    mean = np.full(NUM_JOINTS, np.nan)
    cj = np.full((NUM_JOINTS, 2), np.nan)
    for j in range(NUM_JOINTS):
        m = ok[:, j]
        if m.any():
            mean[j] = r["vis"][m, j].mean()
            cj[j] = pearson(1.0 - r["vis"][m, j], u[m, j]), spearman(1.0 - r["vis"][m, j], u[m, j])
    out["mean"], out["corr_joint"] = mean, cj
    out["mean_all"] = float(r["vis"][ok].mean()) if ok.any() else float("nan")
    out["corr"] = {}
    for k in COMPONENTS:
        m = np.isfinite(r[k])
        out["corr"][k] = (pearson(1.0 - r[k][m], u[m]), spearman(1.0 - r[k][m], u[m]))
    out["corr_err"] = (pearson(1.0 - r["vis"][ok], e[ok]), spearman(1.0 - r["vis"][ok], e[ok]))
    table = np.full((bins, 3), np.nan)
    ci = np.asarray(counts, np.int64).reshape(n, NUM_JOINTS, 4)
    which = np.minimum(ci[:, :, 3][ok] * bins // ci[:, :, 0][ok], bins - 1)      # k / K <= seen / total < (k + 1) / K, in integers
    for k in range(bins):
        m = which == k
        table[k, 0] = m.sum()
        if m.any():
            table[k, 1], table[k, 2] = u[ok][m].mean(), e[ok][m].mean()
    out["bins"] = table
    return out


def summary_vector(st: Dict[str, object], margin: int) -> np.ndarray:
    """float64 [len(SUMMARY_NAMES)]: the pooled numbers of statistics() in the order of SUMMARY_NAMES."""
    c = st["corr"]
    return np.array([st["mean_all"], *c["vis"], *c["vis_frame"], *c["vis_self"], *c["vis_obj"], *st["corr_err"], st["valid"], st["invalid"],
                     margin, st["bins"].shape[0]], np.float64)


def result_arrays(counts, st: Dict[str, object], margin: int) -> Dict[str, object]:
    """What the evaluator's result (and the .npz) gains: vis_counts int32 [N,24,4], vis [N,24], vis_summary, vis_joint [24,3] = mean
    vis, Pearson, Spearman per joint, vis_bins [K,3]; `vis_stats` (the whole dict, for the report; not saved)."""
    return {"vis_counts": np.asarray(counts, np.int32).reshape(-1, NUM_JOINTS, 4), "vis": st["vis"], "vis_summary": summary_vector(st, margin),
            "vis_joint": np.concatenate([st["mean"][:, None], st["corr_joint"]], axis=1), "vis_bins": st["bins"], "vis_stats": st,
            "vis_margin": int(margin)}


def report_lines(res: Dict[str, object]):
    """eval.py --visibility: the report from the result's `vis_stats`."""
    st, K = res["vis_stats"], res["vis_bins"].shape[0]
    c = st["corr"]
    lines = [f"Visibility (window margin {res['vis_margin']} px): mean {st['mean_all']} over {st['valid']} (crop, joint) entries "
             f"({st['invalid']} without a pixel in the window)",
             "Visibility per joint: " + " ".join(f"{v:.4f}" for v in st["mean"]),
             f"Corr(1 - vis, uncertainty): Pearson {c['vis'][0]}, Spearman {c['vis'][1]}",
             "Corr(1 - vis, uncertainty) per joint (Pearson): " + " ".join(f"{v:.4f}" for v in st["corr_joint"][:, 0]),
             "Corr(1 - vis, uncertainty) per joint (Spearman): " + " ".join(f"{v:.4f}" for v in st["corr_joint"][:, 1])]
    for k, what in (("vis_frame", "truncation"), ("vis_self", "self-occlusion"), ("vis_obj", "object occlusion")):
        lines.append(f"Corr(1 - {k}, uncertainty) [{what}]: Pearson {c[k][0]}, Spearman {c[k][1]}")
    lines.append(f"Corr(1 - vis, per-joint error): Pearson {st['corr_err'][0]}, Spearman {st['corr_err'][1]}")
    lines.append("Visibility bin: entries, mean uncertainty, mean per-joint error")
    for k in range(K):
        row = res["vis_bins"][k]
        lines.append(f"  [{k / K:.2f}, {(k + 1) / K:.2f}{']' if k == K - 1 else ')'}: {int(row[0])}, {row[1]}, {row[2]}")
    return lines


# ---- the per-batch step --------------------------------------------------------------------------------------------------------------
class VisibilityEval:
    """The per-batch step of eval.py --visibility, on the current stream: ground-truth joints -> gt_cam_t (as --segm) -> counts.

        vs = VisibilityEval(mesh, part_crop, capacity=len(dataset), batch_size=64)
        vs.step(lo, hi, gt_verts, gt_joints49, occ_mask)          # per batch; nothing is read back
        res.update(vs.finish(res["corr_x"], res["corr_y"]))       # once: one copy of [N,24,4] int32, statistics on the host
    """

    def __init__(self, mesh, part_crop, capacity: int, batch_size: int, res: int = 224, margin: Optional[int] = None, bins: int = 5,
                 focal: float = 5000.0):
        self.mesh, self.res, self.focal = mesh, int(res), float(focal)
        self.margin = self.res // 2 if margin is None else int(margin)
        self.bins = int(bins)
        if not 0 <= self.margin <= self.res:
            raise ValueError(f"--vis_margin must be in 0..res (the crop's side, {self.res}), got {self.margin}")
        if not 2 <= self.bins <= 20:
            raise ValueError(f"--vis_bins must be in 2..20, got {self.bins}")
        self.part = np.asarray(part_crop, np.float32).reshape(-1, NUM_JOINTS, 3)
        self.capacity, self.count, self.batch = int(capacity), 0, max(int(batch_size), 1)
        if self.part.shape[0] != self.capacity:
            raise ValueError(f"`part` has {self.part.shape[0]} rows, the dataset {self.capacity}")
        dev = mesh.device
        self.h_face_part = mesh.face_part.cpu().numpy()
        self.counts = torch.zeros((self.capacity, NUM_JOINTS, 4), device=dev, dtype=torch.int32)
        nbytes = ops.part_visibility_scratch_bytes(min(self.batch, self.capacity), self.res, self.margin)
        if nbytes < 1:
            raise ValueError(f"--visibility: batch {self.batch}, res {self.res} and margin {self.margin} are outside the operator's range")
        self.scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        self.last_cam_t = None

    def step(self, lo: int, hi: int, gt_verts: torch.Tensor, gt_joints49: torch.Tensor, occ_mask: Optional[torch.Tensor] = None) -> None:
        """Rows [lo, hi) of the dataset: gt_verts [B,V,3] / gt_joints49 [B,49,3] from smpl_lbs of the ground truth, occ_mask uint8
        [B,res,res] or None.  The batches come in order; nothing is copied to the host."""
        B = hi - lo
        if lo != self.count or B < 1 or B > self.batch or hi > self.capacity or int(gt_verts.shape[0]) != B:
            raise PocoHipError(f"VisibilityEval.step: rows [{lo}, {hi}) do not follow the {self.count} rows stepped (batches of up to {self.batch})")
        dev = self.mesh.device
        k2d = torch.from_numpy(np.ascontiguousarray(self.part[lo:hi])).to(dev)
        with torch.cuda.device(dev):
            cam_t = ops.estimate_translation(gt_joints49[:, 25:49].contiguous(), k2d, self.focal, self.res)
            ops.part_visibility(gt_verts, cam_t, self.mesh.faces, self.mesh.face_part, self.focal, self.res, self.margin, occ_mask,
                                out=self.counts[lo:hi], scratch=self.scratch, h_face_part=self.h_face_part)
        self.last_cam_t = cam_t
        self.count = hi

    def finish(self, corr_x, corr_y) -> Dict[str, object]:
        """corr_x / corr_y: the per-joint error and uncertainty of Evaluator.finish(), [N * 24] with all 24 joints selected."""
        if self.count < 1:
            raise PocoHipError("VisibilityEval.finish: no crop has been stepped")
        counts = self.counts[:self.count].cpu().numpy()
        u, e = np.asarray(corr_y, np.float64), np.asarray(corr_x, np.float64)
        if u.size != self.count * NUM_JOINTS or e.size != u.size:
            raise ValueError(f"--visibility needs the uncertainty and error of all 24 joints of {self.count} crops, got {u.size} and {e.size} numbers")
        return result_arrays(counts, statistics(counts, u, e, self.bins), self.margin)


def prepare(model, dataset, dataset_path: str, smpl_path: str, part_mapping: Optional[str] = None, batch_size: int = 64,
            uncert_threshold: Optional[float] = None, res: int = 224, margin: Optional[int] = None, bins: int = 5) -> VisibilityEval:
    """The VisibilityEval of one evaluation run: the dataset's `part` rows in crop pixels (as segm.run_eval reads them), the part mesh
    of the body model, and dataset.want_occ_mask switched on so that an occluded batch brings its mask.  ValueError for a dataset
    without SMPL ground truth or `part`, a body model without triangles, a margin or bin count out of range."""
    from . import evaluate, segm
    if dataset.gt_form != "smpl" or dataset.shape is None:
        raise ValueError("--visibility needs SMPL ground truth (`pose` and `shape`) in the dataset")
    with np.load(dataset_path, allow_pickle=False) as z:
        check_dataset_keys(z.files)
        rows = evaluate.select_confident(z, uncert_threshold, dataset_path) if uncert_threshold is not None else z
        part = dataset.part_keypoints(rows["part"]) if getattr(dataset, "crop", "demo") == "dataset" \
            else segm.crop_keypoints24(rows["part"], dataset.center, dataset.scale, res)
    with np.load(smpl_path) as z:
        mesh = segm.PartMesh.from_smpl({k: z[k] for k in ("faces", "lbs_weights") if k in z.files}, model.device, part_mapping)
    vs = VisibilityEval(mesh, part, len(dataset), batch_size, res, margin, bins, segm.FOCAL_LENGTH)
    dataset.want_occ_mask = True
    return vs
