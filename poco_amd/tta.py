"""Test-time augmentation (eval.py / demo.py --tta VIEWS [--tta_weight uncert|uniform]): K views of every crop - the crop itself,
mirrored, rotated, rescaled - are cut in one launch of the dataset crop (poco_amd/datacrop.py), regressed in ONE forward of K * b
rows, and poco_op_tta_fuse (csrc/tta_fuse.hip) takes every view's rotations back into the base crop's frame and fuses them per joint,
weighted by the model's own uncertainty; the fused rows are re-posed with the LBS operator.  All on the current stream, nothing read
back.  The contract is stated in include/poco_hip.h and DESIGN.md section 26; tests/tta_np.py restates it.

Camera and 2-D joints are NOT fused: the fused dict carries the base view's (sections 24 and 25 leave them raw in the same way)."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import ops
from ._lib import PocoHipError

WEIGHTS = ("uncert", "uniform")
MAX_VIEWS = ops.TTA_MAX_VIEWS
FUSED_KEYS = ("pred_pose", "var_pose", "pred_shape", "smpl_vertices", "smpl_joints3d")


@dataclass(frozen=True)
class View:
    """One view of a crop: mirrored left-right or not, rotated by `rot` degrees, its box scaled by `scale` (the parameters of
    datacrop.crop_params)."""
    flip: bool = False
    rot: float = 0.0
    scale: float = 1.0

    def describe(self) -> str:
        parts = (["flip"] if self.flip else []) + ([f"rot:{self.rot:g}"] if self.rot != 0 else []) + ([f"scale:{self.scale:g}"] if self.scale != 1 else [])
        return "+".join(parts) or "identity"


def parse_views(text: str) -> List[View]:
    """"flip,rot:-15,rot:15,flip+scale:1.1" -> [identity, View(flip), View(rot=-15), View(rot=15), View(flip, scale=1.1)]: views
    separated by commas, each a '+'-joined set of flip, rot:<degrees>, scale:<factor>; the identity view is always prepended.
    ValueError: an empty or unreadable view, a component given twice, a duplicate view (the identity included), more than 8 views
    in total, scale <= 0, |rot| > 180, a number that is not finite."""
    views = [View()]
    if not isinstance(text, str) or not text.strip():
        raise ValueError("--tta needs at least one view, e.g. --tta flip")
    for item in text.split(","):
        seen, kw = set(), {}
        for part in item.strip().split("+"):
            part = part.strip()
            name, _, val = part.partition(":")
            if name not in ("flip", "rot", "scale") or name in seen or (name == "flip") != (val == "" and ":" not in part):
                raise ValueError(f"--tta: cannot read {part!r} in view {item.strip()!r}: a view is a '+'-joined set of flip, rot:<degrees>, "
                                 "scale:<factor>, each at most once")
            seen.add(name)
            if name == "flip":
                kw["flip"] = True
                continue
            try:
                x = float(val)
            except ValueError:
                x = float("nan")
            if not math.isfinite(x):
                raise ValueError(f"--tta: {part!r} needs a finite number")
            if name == "rot" and abs(x) > 180:
                raise ValueError(f"--tta: |rot| must be at most 180 degrees, got {x:g}")
            if name == "scale" and x <= 0:
                raise ValueError(f"--tta: scale must be > 0, got {x:g}")
            kw[name] = x
        v = View(**kw)
        if v in views:
            raise ValueError(f"--tta: view {item.strip()!r} ({v.describe()}) is given twice (the identity view is always there)")
        views.append(v)
        if len(views) > MAX_VIEWS:
            raise ValueError(f"--tta: at most {MAX_VIEWS} views in total, the identity included")
    return views


def views_text(views: Sequence[View]) -> str:
    return ",".join(v.describe() for v in views)


# ---- the flags of eval.py and demo.py ------------------------------------------------------------------------------------------
def flag_error(args, script: str):
    """The one sentence that refuses --tta / --tta_weight where they cannot work, or None; script = "eval" | "demo"."""
    tta = getattr(args, "tta", None)
    if tta is None:
        if getattr(args, "tta_weight", None) is not None:
            return "--tta_weight weighs the views of --tta: it needs --tta"
        return None
    try:
        parse_views(tta)
    except ValueError as e:
        return str(e)
    if getattr(args, "cfg2", None) or getattr(args, "ckpt2", None):
        return "--tta with a second model (--cfg2 / --ckpt2) is not supported: fuse the views of one model"
    if script == "eval":
        if getattr(args, "crop", "demo") != "dataset":
            return "--tta cuts its views with the dataset crop: it needs --crop dataset"
        for flag, on in (("--aug_rot", getattr(args, "aug_rot", None) is not None), ("--aug_scale", getattr(args, "aug_scale", None) is not None),
                         ("--aug_flip", bool(getattr(args, "aug_flip", False))), ("--aug_noise", getattr(args, "aug_noise", None) is not None),
                         ("--augment", bool(getattr(args, "augment", False))), ("--aug_occlude", getattr(args, "aug_occlude", None) is not None)):
            if on:
                return f"--tta makes its own views of the unperturbed crop: it cannot be combined with {flag}"
        for flag in ("segm", "likelihood", "rank_metrics"):
            if getattr(args, flag, False):
                return f"--{flag} reads one forward's outputs: it cannot be combined with --tta"
        return None
    if getattr(args, "mode", "folder") != "folder":
        return f"--tta is built for folder mode: --mode {args.mode} is not supported"
    if getattr(args, "gpus", 1) > 1:
        return "--tta with --gpus N > 1 is not supported: run with --gpus 1"
    for flag in ("occlusion_map", "save_dataset", "save_segm"):
        if getattr(args, flag, None):
            return f"--{flag} reads one forward's outputs: it cannot be combined with --tta"
    return None


# ---- making the views ----------------------------------------------------------------------------------------------------------
def view_batch(images, img_index, shapes, centers, scales, views: Sequence[View], res: int, device) -> Dict[str, torch.Tensor]:
    """The model's batch dict for K views of n crops, view-major (row k * n + i), all K * n crops from ONE launch of the dataset
    crop.  images: uint8 [H,W,3] device tensors, img_index [n] which of them crop i is cut from, shapes [n,2] their (h, w),
    centers [n,2], scales [n] (box side / 200).  scale, bbox_info and focal_length per view as EvalDataset._batch_dataset_crop
    computes them, from sc * scale; bbox_info is not mirrored for a flipped view (base_dataset.py:326 does not mirror it)."""
    from . import datacrop
    from .tester import calculate_bbox_info, calculate_focal_length
    K, n = len(views), len(img_index)
    centers = np.asarray(centers, np.float32).reshape(n, 2)
    scales = np.asarray(scales, np.float32).reshape(n)
    shapes = np.asarray(shapes, np.float32).reshape(n, 2)
    c_all, s_all, hw_all = np.tile(centers, (K, 1)), np.tile(scales, K), np.tile(shapes, (K, 1))
    rot = np.repeat([float(v.rot) for v in views], n)
    flip = np.repeat([int(v.flip) for v in views], n)
    sc = np.repeat([float(v.scale) for v in views], n)
    params = datacrop.batch_params(c_all, s_all, rot, flip, np.ones((K * n, 3)), sc, res)
    img = datacrop.dataset_crop(images, np.tile(np.asarray(img_index, np.int64), K), params, res, True)
    scale_eff = (sc * s_all.astype(np.float64)).astype(np.float32)
    info = np.stack([calculate_bbox_info(c, s, hw) for c, s, hw in zip(c_all, scale_eff, hw_all)])
    focal = np.array([calculate_focal_length(h, w) for h, w in hw_all], np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)   # noqa: E731
    return {"img": img, "bbox_info": t(info), "focal_length": t(focal), "scale": t(scale_eff), "center": t(c_all), "orig_shape": t(hw_all)}


def dataset_batch(dataset, lo: int, hi: int, views: Sequence[View], device) -> Dict[str, torch.Tensor]:
    """view_batch for samples [lo, hi) of an EvalDataset with crop='dataset' and no augmentation: every distinct image of the batch
    is read and uploaded once."""
    from PIL import Image
    from . import datacrop
    names = dataset.imgname[lo:hi]
    distinct = list(dict.fromkeys(names))
    slot = {nm: k for k, nm in enumerate(distinct)}
    frames = [np.array(Image.open(os.path.join(dataset.img_dir, nm)).convert("RGB")) for nm in distinct]
    images = [datacrop.upload_image(fr, device) for fr in frames]
    idx = [slot[nm] for nm in names]
    return view_batch(images, idx, [frames[k].shape[:2] for k in idx], dataset.center[lo:hi], dataset.scale[lo:hi], views, dataset.res, device)


def frame_batch(frame_u8: torch.Tensor, dets, views: Sequence[View], res: int) -> Dict[str, torch.Tensor]:
    """view_batch for the detections [n,4] (cx, cy, w, h) of one frame on the device: centre = (cx, cy), scale = max(w, h) / 200."""
    d = np.asarray(dets, np.float32).reshape(-1, 4)
    n = len(d)
    H, W = int(frame_u8.shape[0]), int(frame_u8.shape[1])
    return view_batch([frame_u8], np.zeros(n, np.int64), np.tile([[H, W]], (n, 1)), d[:, :2], np.maximum(d[:, 2], d[:, 3]) / 200.0, views, res,
                      frame_u8.device)


def cat_view_batches(batches, K: int) -> Dict[str, torch.Tensor]:
    """View-major batches of n_1, n_2, ... crops as one view-major batch of their sum: row k * n + i keeps its view."""
    if len(batches) == 1:
        return batches[0]
    return {key: torch.cat([b[key].reshape(K, b[key].shape[0] // K, *b[key].shape[1:]) for b in batches], 1).flatten(0, 1).contiguous()
            for key in batches[0]}


class TTAModel:
    """A finalized engine behind K views, presented as what run_eval and the folder-mode tester use of POCO: __call__(batch,
    want_segm=False), forward_all, max_batch, device, smpl_lbs, check_status, flow_context.  `batch` is the K * b-row view-major
    dict of view_batch; max_batch = the crops b one forward takes = max(1, the engine's max_batch // K)."""

    def __init__(self, model, views: Sequence[View], weight: str = "uncert"):
        views = list(views)
        if weight not in WEIGHTS:
            raise ValueError(f"tta weight must be one of {WEIGHTS}, got {weight!r}")
        if not 2 <= len(views) <= MAX_VIEWS or views[0] != View():
            raise ValueError(f"TTAModel needs 2 to {MAX_VIEWS} views, the identity first")
        if not getattr(model, "_finalized", False):
            raise PocoHipError("TTAModel needs a finalized engine")
        if model.max_batch < len(views):
            raise PocoHipError(f"TTAModel: the engine's max_batch {model.max_batch} does not hold the {len(views)} views of one crop")
        self.model, self.views, self.weight, self.K = model, views, weight, len(views)
        self.device, self.max_batch = model.device, max(1, model.max_batch // len(views))
        self.table = [(int(v.flip), float(v.rot)) for v in views]

    @torch.no_grad()
    def __call__(self, batch: Dict[str, torch.Tensor], want_segm: bool = False) -> Dict[str, object]:
        return self.forward_all(batch, want_segm)[1]

    @torch.no_grad()
    def forward_all(self, batch: Dict[str, torch.Tensor], want_segm: bool = False):
        """(the K per-view output dicts: row slices of the one forward's output; the fused dict).  The fused dict is the base
        view's rows with FUSED_KEYS replaced - pose', var', betas' from the operator, vertices and 3-D joints from smpl_lbs on all
        b rows - plus tta_spread [b,24]; camera and 2-D joints stay the base view's."""
        if want_segm:
            raise PocoHipError("TTAModel: pred_segm_mask is one view's output, not a fused one (want_segm=True)")
        rows = int(batch["img"].shape[0])
        if rows % self.K:
            raise PocoHipError(f"TTAModel: a batch of {rows} rows is not {self.K} views of whole crops")
        b = rows // self.K
        out = self.model(batch, want_segm=False)
        per_view = [{k: (v[i * b:(i + 1) * b] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == rows else v) for k, v in out.items()}
                    for i in range(self.K)]
        f = ops.tta_fuse(out["pred_pose"].contiguous(), out["var_pose"].contiguous(), out["pred_shape"].contiguous(), self.table, self.weight)
        verts, joints = self.model.smpl_lbs(f["betas"], f["pose"])
        fused = dict(per_view[0])
        fused.update(pred_pose=f["pose"], var_pose=f["var"], pred_shape=f["betas"], smpl_vertices=verts, smpl_joints3d=joints,
                     tta_spread=f["spread"])
        return per_view, fused

    forward = __call__

    def smpl_lbs(self, betas, rotmat):
        return self.model.smpl_lbs(betas, rotmat)

    def check_status(self, sync: bool = False) -> None:
        self.model.check_status(sync)

    def flow_context(self, uncert_feat):
        return self.model.flow_context(uncert_feat)

    def __getattr__(self, name):
        raise AttributeError(f"TTAModel has no {name!r}: an engine behind test-time views offers __call__, forward_all, max_batch, device, "
                             "smpl_lbs, check_status and flow_context; use tta.model for the engine's own methods")
