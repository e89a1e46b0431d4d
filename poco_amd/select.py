"""Choosing between two regressors by their own uncertainty (demo.py / eval.py --cfg2 --ckpt2 --select crop|joint): both engines regress the
same crops on one device, poco_op_select_regressor (csrc/select_regressor.hip) decides per crop or per joint from the two var_pose
and copies the chosen model's outputs, all behind the forwards on the same stream.  The contract is stated in include/poco_hip.h and
DESIGN.md section 25; tests/select_np.py restates it.

In joint mode a row may mix the two models' rotations: those rows (the operator lists them on the device) are re-posed with the LBS
operator from the mixed pose and the shape of the model chosen for the root, the pattern of infill.infill_tracks."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import ops, postproc
from ._lib import PocoHipError

MODES = ("crop", "joint")
# what follows the model chosen for the root joint, row by row: (output key, floats per row)
PAYLOAD_KEYS = ("smpl_vertices", "smpl_joints3d", "smpl_joints2d", "pred_shape", "pred_cam")


def kind_of(backbone: str) -> int:
    """The rule of get_global_uncert (poco_utils.py:50-60) a variant's score follows: 1 = root (cliff), 0 = mean (pare)."""
    return 1 if "cliff" in backbone else 0


class RegressorPair:
    """Two finalized engines presented as one: what POCOTester uses of POCO - __call__(batch, want_segm=False), max_batch, device,
    smpl_lbs, check_status, flow_context - with the selection behind the two forwards.  Model 0 is --cfg / --ckpt, model 1 is
    --cfg2 / --ckpt2; `scale` multiplies model 1's uncertainty before the comparison.

    The output dict is model 0's with pred_pose, var_pose and PAYLOAD_KEYS replaced by the selected rows, plus select uint8 [B,24]
    (0 | 1 per joint), select_score [B,2] and select_mixed uint8 [B].  Everything else - uncert_feat, pred_cam_t, record, the 6-D
    pose, body_feat2 - stays MODEL 0's and is NOT selected: nothing the tester writes reads them."""

    def __init__(self, model0, model1, *, mode: str = "crop", scale: float = 1.0, kinematic: bool = True, thr: float = 0.40):
        if mode not in MODES:
            raise ValueError(f"select mode must be one of {MODES}, got {mode!r}")
        if not (np.isfinite(scale) and scale > 0):
            raise ValueError(f"select scale must be finite and > 0, got {scale!r}")
        for m in (model0, model1):
            if not getattr(m, "_finalized", False):
                raise PocoHipError("RegressorPair needs two finalized engines")
        if model0.device != model1.device or model0.max_batch != model1.max_batch:
            raise PocoHipError(f"RegressorPair needs both engines on one device with one max_batch, got {model0.device} / "
                               f"{model0.max_batch} and {model1.device} / {model1.max_batch}")
        self.models = (model0, model1)
        self.backbones = (model0.variant, model1.variant)
        self.kinds = (kind_of(model0.variant), kind_of(model1.variant))
        self.mode, self.scale, self.kinematic, self.thr = mode, float(scale), bool(kinematic), float(thr)
        self.device, self.max_batch = model0.device, model0.max_batch

    # ---- what the tester uses of POCO ----------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, batch: Dict[str, torch.Tensor], want_segm: bool = False) -> Dict[str, object]:
        """Both forwards on the batch dict of the cliff head (the pare head reads `img` alone, model.py _pack_io), one call of the
        operator, and in joint mode the LBS of the mixed rows; all on the current stream.  Joint mode reads one int back (the
        number of mixed rows)."""
        return self.forward_all(batch, want_segm)[2]

    @torch.no_grad()
    def forward_all(self, batch: Dict[str, torch.Tensor], want_segm: bool = False):
        """(model 0's output dict, model 1's, the selected one): what __call__ computes, with the two solo outputs handed out as
        well (evaluate.run_eval_pair scores all three).  The solo dicts are the engines' own and hold until their next forward."""
        if want_segm:
            raise PocoHipError("RegressorPair: pred_segm_mask is one model's output, not a selectable one (want_segm=True)")
        o0, o1 = self.models[0](batch, want_segm=False), self.models[1](batch, want_segm=False)
        joint = self.mode == "joint"
        sel = ops.select_regressor(o0["pred_pose"], o0["var_pose"], self.kinds[0], o1["pred_pose"], o1["var_pose"], self.kinds[1],
                                   [(o0[k], o1[k]) for k in PAYLOAD_KEYS], kinematic=self.kinematic, thr=self.thr, scale=self.scale,
                                   mode=self.mode, rows=joint)
        out = dict(o0)
        out["pred_pose"], out["var_pose"] = sel["pose"], sel["var"]
        out.update(zip(PAYLOAD_KEYS, sel["payloads"]))
        out["select"], out["select_score"], out["select_mixed"] = sel["choice"], sel["score"], sel["mixed"]
        if joint:
            n = int(sel["count"].item())
            rows = sel["rows"][:n].long()
            for lo in range(0, n, max(self.max_batch, 1)):                   # LBS of the mixed rows only
                r = rows[lo:lo + self.max_batch]
                v, j = self.smpl_lbs(out["pred_shape"].index_select(0, r), out["pred_pose"].index_select(0, r))
                out["smpl_vertices"].index_copy_(0, r, v)
                out["smpl_joints3d"].index_copy_(0, r, j)
        return o0, o1, out

    forward = __call__

    def smpl_lbs(self, betas, rotmat):
        """Both engines hold the same body model (POCOTester loads one --smpl file into both): model 0's."""
        return self.models[0].smpl_lbs(betas, rotmat)

    def check_status(self, sync: bool = False) -> None:
        for m in self.models:
            m.check_status(sync)

    def flow_context(self, uncert_feat):
        """Model 0's flow, on model 0's uncert_feat (the pair's output carries that one)."""
        return self.models[0].flow_context(uncert_feat)

    def __getattr__(self, name):
        raise AttributeError(f"RegressorPair has no {name!r}: a pair of engines offers __call__, max_batch, device, smpl_lbs, "
                             "check_status and flow_context; use pair.models[i] for one engine's own methods")


# ---- the flags of demo.py and eval.py ------------------------------------------------------------------------------------------
def flag_error(args, single_model_flags=()):
    """The one sentence that refuses --cfg2 / --ckpt2 / --select / --select_scale where they cannot work, or None: one of the pair
    without the other, --select / --select_scale without them, a scale that is not a finite number > 0, --gpus N > 1, and any of
    `single_model_flags` (attribute names of flags that read one model's outputs) together with a second model."""
    cfg2, ckpt2 = getattr(args, "cfg2", None), getattr(args, "ckpt2", None)
    if bool(cfg2) != bool(ckpt2):
        return "--cfg2 and --ckpt2 describe the second model together: give both or neither"
    scale = getattr(args, "select_scale", None)
    if not cfg2:
        if getattr(args, "select", None) is not None or scale is not None:
            return "--select and --select_scale choose between two models: they need --cfg2 and --ckpt2"
        return None
    if scale is not None and not 0 < scale < float("inf"):
        return f"--select_scale must be a finite number > 0, got {scale}"
    if getattr(args, "gpus", 1) > 1:
        return ("a second model with --gpus N > 1 is not supported: the packed record the ranks exchange has no room for the "
                "choice; run with --gpus 1")
    for flag in single_model_flags:
        if getattr(args, flag, None):
            return f"--{flag} reads one model's outputs: it cannot be combined with --cfg2 / --ckpt2"
    return None


# ---- per-row post-processing on the host (postproc keeps its per-model functions) --------------------------------------------------
def root_choice(select) -> np.ndarray:
    """bool [n]: the rows whose root joint - and with it shape, camera and 2-D joints - came from model 1."""
    return np.asarray(select).reshape(-1, 24)[:, 0] != 0


def pair_uncert(var_pose, select, backbones, kinematic: bool, clip: bool):
    """(var, var_global) of selected rows: var = the processed uncertainty of the selected var_pose; var_global per row by the rule
    of the model chosen for the root (postproc.global_uncert of that backbone); clip as folder mode (True) or video mode (False)."""
    var = postproc.prepare_uncert(var_pose, kinematic)
    g0, g1 = (postproc.global_uncert(var, b, clip=clip) for b in backbones)
    return var, np.where(root_choice(select), g1, g0)


def pair_joints2d(j2d, select, backbones, dets, crop_size):
    """Folder mode's 2-D joints (tester.py:225-230 of the reference, per row): rows whose root came from a model without the cliff
    head hold crop-normalised coordinates and go through convert_crop_coords_to_orig_img; the others are original-image pixels."""
    root = root_choice(select)
    crop_rows = np.where(root, "cliff" not in backbones[1], "cliff" not in backbones[0])
    if not crop_rows.any():
        return j2d
    conv = postproc.convert_crop_coords_to_orig_img(dets, j2d, crop_size)
    return np.where(crop_rows[:, None, None], conv, j2d).astype(j2d.dtype)


def summary_line(select, mixed_rows: int, mode: str) -> str:
    """The one printed line: what was taken from model 2, the mixed rows, the totals."""
    sel = np.asarray(select).reshape(-1, 24)
    n = len(sel)
    if mode == "joint":
        return (f"select joint: {int(sel.sum())} of {sel.size} joint-entries from model 2, {int(mixed_rows)} mixed rows re-posed, "
                f"{int(root_choice(sel).sum())} of {n} crops with model 2's root")
    return f"select crop: {int(root_choice(sel).sum())} of {n} crops from model 2, {int(mixed_rows)} mixed rows"
