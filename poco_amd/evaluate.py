"""Evaluation on the GPU (eval.py): a binding of poco_evaluator_* (include/poco_hip.h, csrc/eval_metrics.hip) and the loop of
pocolib/core/trainer.py:298-336,365-391 on this engine.  Per crop nothing goes to the host between the forward and
Evaluator.finish(): the metrics are computed from the model's device outputs into device records.

The reference evaluates with numpy on the host (pocolib/utils/eval_utils.py: one np.linalg.svd per crop); tests/eval_np.py
restates that and is the yardstick of tests/test_eval_*.py."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ._lib import PocoHipError, check, lib

H36M_TO_J17 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10, 0, 7, 9]      # constants.py:95
H36M_TO_J14 = H36M_TO_J17[:14]                                               # constants.py:96
J24_TO_J17 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 18, 14, 16, 17]       # constants.py:98
J24_TO_J14 = J24_TO_J17[:14]                                                 # constants.py:99
DATASET_NAMES = ("3dpw", "h36m-p2", "mpi-inf-3dhp")
MAX_JOINTS = 32
RECORD_FLOATS = 416
# record offsets (include/poco_hip.h)
R_MPJPE, R_PA, R_V2V, R_MPJPE_J, R_PA_J, R_POSE, R_UNC, R_PRED, R_GT, R_NONREL = 0, 1, 2, 4, 36, 68, 92, 116, 212, 308


def joint_map(dataset_name: str):
    """eval_utils.py:65: 17 joints for mpi-inf-3dhp, 14 otherwise."""
    return H36M_TO_J17 if dataset_name == "mpi-inf-3dhp" else H36M_TO_J14


def _bind():
    L = lib()
    if getattr(L, "_eval_bound", False):
        return L
    L.poco_evaluator_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int64, C.POINTER(C.c_void_p)]
    L.poco_evaluator_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    L.poco_evaluator_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.poco_evaluator_uncert_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.poco_evaluator_rank_inputs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int), C.c_void_p]
    L.poco_evaluator_reset.argtypes = [C.c_void_p]
    L.poco_evaluator_destroy.argtypes = [C.c_void_p]
    L.poco_evaluator_destroy.restype = None
    L._eval_bound = True
    return L


def _dev(t: Optional[torch.Tensor], what: str, tail) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda):
        raise PocoHipError(f"Evaluator.step: {what} must be a CUDA tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    if tuple(t.shape[1:]) != tuple(tail):
        raise PocoHipError(f"Evaluator.step: {what} must be [B, {', '.join(map(str, tail))}], got {tuple(t.shape)}")
    return t


class Evaluator:
    """Device-side metric accumulator.

        ev = Evaluator(J_regressor_h36m, joint_map("3dpw"), capacity=len(dataset))
        ev.step(model(batch), gt_pose, gt_vertices=verts)        # per batch, enqueued on the current stream
        res = ev.finish()                                        # val_mpjpe, val_pampjpe, val_v2v, val_corr + per-sample arrays
    """

    def __init__(self, J_regressor, jmap: Sequence[int], capacity: int, pelvis: int = 0, sel_uncert_part: Optional[Sequence[int]] = None,
                 kinematic: bool = True, device=None):
        self.J_regressor = np.ascontiguousarray(np.asarray(J_regressor, np.float32))
        if self.J_regressor.ndim != 2:
            raise PocoHipError("Evaluator: J_regressor must be [J, V]")
        self.J, self.V = (int(x) for x in self.J_regressor.shape)
        self.map = np.ascontiguousarray(np.asarray(jmap, np.int32).reshape(-1))
        self.M = int(self.map.shape[0])
        self.sel = np.ascontiguousarray(np.asarray(list(range(24)) if sel_uncert_part is None else sel_uncert_part, np.int32).reshape(-1))
        self.capacity, self.count = int(capacity), 0
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._h = C.c_void_p()
        check(_bind().poco_evaluator_create(self.J_regressor.ctypes.data, self.J, self.V, self.map.ctypes.data, self.M, int(pelvis),
                                            self.sel.ctypes.data if self.sel.size else None, int(self.sel.size), int(bool(kinematic)),
                                            self.capacity, C.byref(self._h)), "poco_evaluator_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_evaluator_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, pred: Dict[str, torch.Tensor], gt_pose: torch.Tensor, gt_vertices: Optional[torch.Tensor] = None,
             gt_joints: Optional[torch.Tensor] = None) -> None:
        """pred = the model's output dict (smpl_vertices [B,V,3], pred_pose [B,24,3,3], var_pose [B,24] or with up to two
        trailing axes); gt_pose [B,72] axis-angle; exactly one of gt_vertices [B,V,3] and gt_joints [B,M,3].  Enqueued on the
        current stream: no synchronisation, nothing copied to the host."""
        pv = _dev(pred["smpl_vertices"], "smpl_vertices", (self.V, 3))
        B = int(pv.shape[0])
        pp = _dev(pred["pred_pose"], "pred_pose", (24, 3, 3))
        var = pred["var_pose"]
        if not (torch.is_tensor(var) and var.is_cuda and 2 <= var.dim() <= 4 and var.shape[1] == 24):
            raise PocoHipError("Evaluator.step: var_pose must be a CUDA tensor [B,24], [B,24,a] or [B,24,a,b]")
        var = _dev(var, "var_pose", var.shape[1:])
        t1, t2 = (1, 1) if var.dim() == 2 else ((1, int(var.shape[2])) if var.dim() == 3 else (int(var.shape[2]), int(var.shape[3])))
        gp = _dev(gt_pose, "gt_pose", (72,))
        gv = _dev(gt_vertices, "gt_vertices", (self.V, 3))
        gj = _dev(gt_joints, "gt_joints", (self.M, 3))
        for t in (pp, var, gp, gv, gj):
            if t is not None and t.shape[0] != B:
                raise PocoHipError("Evaluator.step: batch sizes differ")
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        with torch.cuda.device(self.device):
            check(lib().poco_evaluator_step(self._h, B, p(pv), p(gv), p(gj), p(pp), p(gp), p(var), t1, t2,
                                            C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "poco_evaluator_step")
        self.count += B

    def reset(self) -> None:
        check(lib().poco_evaluator_reset(self._h), "poco_evaluator_reset")
        self.count = 0

    def uncert_summary(self) -> Dict[str, float]:
        """val_mpjpe_var = mean_i(MPJPE_i / (mean_24(processed uncertainty_i) + 1e-9)) and val_var = mean_i(mean_24(...))
        (trainer.py:374,377-378; metres, not scaled by 1000) over the records written so far, reduced on the device; the records
        are only read.  Synchronises the current stream."""
        summ = np.zeros(2, np.float64)
        with torch.cuda.device(self.device):
            check(_bind().poco_evaluator_uncert_summary(self._h, summ.ctypes.data, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                  "poco_evaluator_uncert_summary")
        return {"val_mpjpe_var": float(summ[0]), "val_var": float(summ[1])}

    def rank_inputs(self, mode: int):
        """Keys and value planes for ops.rank_curve from the records written so far, as device tensors (key [n], vals [E,n]); the
        records are only read and nothing goes to the host.  mode 0 = per crop: key = the mean of the crop's 24 processed
        uncertainties (the u_i of uncert_summary), vals = MPJPE, PA-MPJPE, V2V.  mode 1 = per selected joint, crop-major: key =
        corr_y, vals = corr_x of finish().  Enqueued on the current stream."""
        if mode not in (0, 1):
            raise PocoHipError("Evaluator.rank_inputs: mode must be 0 (per crop) or 1 (per joint)")
        n, E = (self.count, 3) if mode == 0 else (self.count * int(self.sel.size), 1)
        key = torch.empty(max(n, 1), device=self.device, dtype=torch.float32)
        vals = torch.empty((E, max(n, 1)), device=self.device, dtype=torch.float32)
        hn, hE = C.c_int64(0), C.c_int(0)
        with torch.cuda.device(self.device):
            check(_bind().poco_evaluator_rank_inputs(self._h, int(mode), key.data_ptr(), vals.data_ptr(), n, C.byref(hn), C.byref(hE),
                                                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                  "poco_evaluator_rank_inputs")
        assert (hn.value, hE.value) == (n, E), (hn.value, hE.value, n, E)
        return key, vals

    def copy_records(self, order: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The records written so far as a device tensor [n, RECORD_FLOATS], copied on the device: record order[i] in row i (order
        int32 [n] on the device, entries in [0, count)), or all of them in their own order.  Enqueued on the current stream; nothing
        goes to the host."""
        if order is not None and not (torch.is_tensor(order) and order.is_cuda and order.dtype == torch.int32 and order.dim() == 1
                                      and order.numel() >= 1):
            raise PocoHipError("Evaluator.copy_records: order must be a CUDA int32 tensor [n], n >= 1")
        n = self.count if order is None else int(order.numel())
        out = torch.empty((max(n, 1), RECORD_FLOATS), device=self.device, dtype=torch.float32)
        L = _bind()
        L.poco_evaluator_copy_records.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        with torch.cuda.device(self.device):
            check(L.poco_evaluator_copy_records(self._h, None if order is None else order.contiguous().data_ptr(), n, out.data_ptr(),
                                                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                  "poco_evaluator_copy_records")
        return out

    def finish(self, save_results: bool = False, return_records: bool = False) -> Dict[str, object]:
        """Summary under the reference's log names (trainer.py:397-403) plus the per-sample arrays of
        SaveResults.evaluation_results (save_results.py:23-43): mpjpe / pampjpe [N,M], v2v [N], corr_x / corr_y (flattened over
        the selected joints), and with save_results pred_jnts3D / gt_jnts3D [N,M,3].  Synchronises the current stream."""
        summ = np.zeros(8, np.float64)
        rec = np.empty((self.count, RECORD_FLOATS), np.float32)
        with torch.cuda.device(self.device):
            check(lib().poco_evaluator_finish(self._h, summ.ctypes.data, rec.ctypes.data, rec.shape[0],
                                              C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "poco_evaluator_finish")
        M = self.M
        out = {"N": int(summ[0]), "val_mpjpe": float(summ[1]), "val_pampjpe": float(summ[2]), "val_v2v": float(summ[3]),
               "val_corr": float(summ[4]), "summary": summ,
               "mpjpe": rec[:, R_MPJPE_J:R_MPJPE_J + M].copy(), "pampjpe": rec[:, R_PA_J:R_PA_J + M].copy(), "v2v": rec[:, R_V2V].copy(),
               "corr_x": rec[:, R_POSE:R_POSE + 24][:, self.sel].reshape(-1), "corr_y": rec[:, R_UNC:R_UNC + 24][:, self.sel].reshape(-1)}
        if save_results:
            out["pred_jnts3D"] = rec[:, R_PRED:R_PRED + 3 * MAX_JOINTS].reshape(-1, MAX_JOINTS, 3)[:, :M].copy()
            out["gt_jnts3D"] = rec[:, R_GT:R_GT + 3 * MAX_JOINTS].reshape(-1, MAX_JOINTS, 3)[:, :M].copy()
        if return_records:
            out["records"] = rec
        return out


NLL_RECORD_FLOATS = 80
N_VALID, N_SUM, N_LOGPHI, N_LOGSIGMA, N_BAR = 0, 1, 8, 32, 56      # record offsets of poco_flow_nll (include/poco_hip.h)


class LikelihoodAccumulator:
    """Device-side accumulator of the flow likelihood (POCO.flow_nll), stepped next to an Evaluator on the same stream.

        lk = LikelihoodAccumulator(model, capacity=len(dataset))
        lk.step(model(batch), gt_pose, valid=has_smpl)           # per batch, enqueued on the current stream
        res = lk.finish()                                        # val_nll, val_log_phi, val_log_sigma + [N,24] arrays
    """

    def __init__(self, model, capacity: int):
        if int(capacity) < 1:
            raise PocoHipError("LikelihoodAccumulator: capacity must be at least 1")
        self.model, self.capacity, self.count = model, int(capacity), 0
        self.records = torch.zeros(self.capacity, NLL_RECORD_FLOATS, device=model.device, dtype=torch.float32)

    def step(self, pred: Dict[str, torch.Tensor], gt_pose: torch.Tensor, valid: Optional[torch.Tensor] = None) -> None:
        """Records of B crops at records[count .. count + B).  More crops than the capacity holds is an error and leaves the
        records as they were.  Nothing is copied to the host."""
        B = int(pred["pred_pose"].shape[0])
        if self.count + B > self.capacity:
            raise PocoHipError(f"LikelihoodAccumulator.step: {self.count} + {B} crops exceed the capacity of {self.capacity}")
        self.model.flow_nll(pred, gt_pose, valid, out=self.records[self.count:self.count + B])
        self.count += B

    def reset(self) -> None:
        self.count = 0

    def finish(self, return_records: bool = False) -> Dict[str, object]:
        """val_nll = loss_nf of losses.py:346 (nf_loss_weight = 1) over the valid crops, val_log_phi / val_log_sigma = the means of
        its two terms, and per crop log_phi / log_sigma / bar_pose [N,24] and nll_valid [N].  Synchronises the current stream."""
        if self.count < 1:
            raise PocoHipError("LikelihoodAccumulator.finish: no crop has been stepped")
        summ = self.model.flow_nll_summary(self.records[:self.count])
        rec = self.records[:self.count].cpu().numpy()
        out = {"nll_N": int(summ[0]), "val_log_phi": float(summ[1]), "val_log_sigma": float(summ[2]), "val_nll": float(summ[3]),
               "log_phi": rec[:, N_LOGPHI:N_LOGPHI + 24].copy(), "log_sigma": rec[:, N_LOGSIGMA:N_LOGSIGMA + 24].copy(),
               "bar_pose": rec[:, N_BAR:N_BAR + 24].copy(), "nll_valid": rec[:, N_VALID].astype(np.int32)}
        if return_records:
            out["nll_records"] = rec
        return out


# ---- datasets ------------------------------------------------------------------------------------------------------------------
def check_dataset_keys(files) -> str:
    """'smpl' (pose + shape: 3DPW-style, ground-truth vertices through SMPL) or 'joints' (S: H36M / MPI-INF-3DHP).  A file with
    neither is refused (base_dataset.py:54-147 reads the same keys)."""
    files = set(files)
    missing = [k for k in ("imgname", "center", "scale") if k not in files]
    if missing:
        raise ValueError(f"dataset file lacks {missing}")
    if "pose" in files and "shape" in files:
        return "smpl"
    if "S" in files:
        return "joints"
    raise ValueError("dataset file has neither `pose` + `shape` (SMPL ground truth) nor `S` (joint ground truth)")


class _Rows(dict):
    """The arrays of a dataset file restricted to some rows, read like the NpzFile they came from."""

    @property
    def files(self):
        return list(self)


def select_confident(z, threshold: float, path: str = "dataset") -> _Rows:
    """base_dataset.py:59-70: every array of the file indexed with the rows get_confident_frames keeps.  A file without `var` and a
    threshold that keeps nothing are refused."""
    from .postproc import confident_frames
    if "var" not in z.files:
        raise ValueError(f"{path}: --uncert_threshold needs `var` (the file was not inferred from POCO: demo.py --save_dataset writes it)")
    idx = confident_frames(z["var"], threshold)
    n = len(z["imgname"])
    if len(idx) == 0:
        raise ValueError(f"{path}: --uncert_threshold {threshold} keeps none of the {n} rows")
    out = _Rows({k: np.asarray(z[k])[idx] for k in z.files})
    out.total = n
    return out


class EvalDataset:
    """The reference's dataset .npz (base_dataset.py:54-147): imgname, center [N,2], scale [N] (bbox size / 200), and pose [N,72]
    + shape [N,10] or S [N,24,3|4]; optional gender, person_id, orig_shape [N,2] (h, w) and img [N,3,224,224] = already normalised
    crops.  Without `img` the images are read from img_dir and cropped on the GPU with the demo's crop (poco_amd/tester.py).
    uncert_threshold (eval.py --uncert_threshold): a file inferred from POCO carries `var` [N,24]; only its confident rows are
    kept, as base_dataset.py:59-70 keeps them (postproc.confident_frames); `total` is the file's row count."""

    def __init__(self, path: str, img_dir: Optional[str] = None, dataset_name: str = "3dpw", bbox_scale: float = 1.0,
                 uncert_threshold: Optional[float] = None, crop: str = "demo", augment=None, res: int = 224, occlude=None):
        if dataset_name not in DATASET_NAMES:
            raise ValueError(f"dataset_name must be one of {DATASET_NAMES}")
        if crop not in ("demo", "dataset"):
            raise ValueError("crop must be 'demo' or 'dataset'")
        if augment is not None and crop != "dataset":
            raise ValueError("an augmentation needs crop='dataset' (the demo crop has no rotation, flip or noise)")
        if occlude is not None and crop != "dataset":
            raise ValueError("synthetic occluders need crop='dataset' (they are pasted inside the dataset crop's launch)")
        self.crop, self.res, self.occlude = crop, int(res), occlude
        # want_occ_mask: set by the visibility step; with occluders, batch() then leaves the batch's mask uint8 [n,res,res] of the
        # pixels they touched in last_occ_mask (None without occluders), on the device
        self.want_occ_mask, self.last_occ_mask = False, None
        # raw_crop: set by run_eval_corrupt; batch() then hands out `img` as the raw float crop in [0, 255] (poco_dataset_crop with
        # normalize = 0), which poco_op_corrupt degrades and normalises
        self.raw_crop = False
        z = np.load(path, allow_pickle=False)
        self.gt_form = check_dataset_keys(z.files)
        if occlude is not None:
            check_occlusion_keys(z.files)
        if uncert_threshold is not None:
            z = select_confident(z, uncert_threshold, path)
        self.name, self.img_dir, self.bbox_scale = dataset_name, img_dir, float(bbox_scale)
        self.imgname = [str(x) for x in z["imgname"]]
        self.total = int(getattr(z, "total", len(self.imgname)))
        self.center = np.asarray(z["center"], np.float32).reshape(-1, 2)
        self.scale = np.asarray(z["scale"], np.float32).reshape(-1)
        n = len(self.imgname)
        self.has_pose = "pose" in z.files
        self.pose = np.asarray(z["pose"], np.float32).reshape(n, 72) if self.has_pose else np.zeros((n, 72), np.float32)
        self.shape = np.asarray(z["shape"], np.float32).reshape(n, 10) if "shape" in z.files else None
        self.joints = None
        if self.gt_form == "joints":
            jm = J24_TO_J17 if dataset_name == "mpi-inf-3dhp" else J24_TO_J14       # base_dataset.py:379
            self.joints = np.ascontiguousarray(np.asarray(z["S"], np.float32)[:, jm, :3])
        self.img = z["img"] if "img" in z.files else None
        self.orig_shape = np.asarray(z["orig_shape"], np.float32).reshape(n, 2) if "orig_shape" in z.files else None
        if self.img is None and not (img_dir and os.path.isdir(img_dir)):
            raise ValueError("the dataset file has no `img` crops: --img_dir must name the folder its imgname entries are relative to")
        for k in ("gender", "person_id"):
            setattr(self, k, np.asarray(z[k]) if k in z.files else None)
        # eval.py --kp_refit: the BODY_25 keypoints (x, y, confidence in image pixels) the pseudo-GT files carry
        self.openpose = np.asarray(z["openpose"], np.float32).reshape(n, 25, 3) if "openpose" in z.files else None
        if crop == "dataset":
            self._init_dataset_crop(z, augment)

    def _init_dataset_crop(self, z, augment) -> None:
        """crop='dataset' (DESIGN.md section 22): the samples' augmentation parameters, drawn once in dataset order, and the ground
        truth as BaseDataset.__getitem__ hands it out - pose_processing on `pose`, j3d_processing on `S` (before the joint map, as
        base_dataset.py:317,379) - so that run_eval reads `pose` / `joints` as before.  `scale` stays the file's; batch() hands the
        model sc * scale."""
        from . import datacrop
        if self.img is not None:
            raise ValueError("crop='dataset' cuts the crops from the images: the dataset file must not carry ready-made `img` crops")
        self.augment = augment if augment is not None else datacrop.AugSpec()
        if self.occlude is not None:
            # one generator for both, per sample: augm_params, then the occlusion draws (BaseDataset.__getitem__)
            (self.aug_flip, self.aug_pn, self.aug_rot, self.aug_scale), d = self.occlude.draw(self.augment, z["part"], self.center, self.scale,
                                                                                              self.res)
            self.occ_records = datacrop.occ_records(d["objects"])
            self.occ_count, self.occ_skipped, self.occ_no_visible = d["count"], int(d["skipped"]), int(d["no_visible"])
            self._occ_cover = np.full(len(self), np.nan)
            self._occ_pending = []
        else:
            self.aug_flip, self.aug_pn, self.aug_rot, self.aug_scale = self.augment.draw(len(self))
        self.scale_eff = self.aug_scale * self.scale.astype(np.float64)      # sc * scale (base_dataset.py:303,326,330)
        if self.has_pose:
            self.pose = np.stack([datacrop.pose_processing(p, r, f) for p, r, f in zip(self.pose, self.aug_rot, self.aug_flip)])
        if self.gt_form == "joints":
            jm = J24_TO_J17 if self.name == "mpi-inf-3dhp" else J24_TO_J14
            S = np.asarray(z["S"], np.float32)
            self.joints = np.ascontiguousarray(np.stack([datacrop.j3d_processing(s, r, f)
                                                         for s, r, f in zip(S, self.aug_rot, self.aug_flip)])[:, jm, :3])

    @property
    def occ_cover(self) -> np.ndarray:
        """Per sample, the fraction of the crop's pixels that a pasted texel with alpha > 0 touched (NaN until its batch was made).
        The counts stay on the device until they are asked for, so that making a batch does not wait for the launch."""
        for lo, hi, cover in self._occ_pending:
            self._occ_cover[lo:hi] = cover.cpu().numpy().astype(np.float64) / float(self.res * self.res)
        self._occ_pending.clear()
        return self._occ_cover

    def part_keypoints(self, part) -> np.ndarray:
        """`part` [N,24,3] of the dataset's rows in crop pixels: j2d_processing with the samples' sc * scale, rot and flip."""
        from . import datacrop
        return datacrop.crop_keypoints24(part, self.center, self.scale_eff, self.aug_rot, self.aug_flip, self.res)

    def _batch_dataset_crop(self, lo: int, hi: int, device) -> Dict[str, torch.Tensor]:
        """The reference's dataset crop for samples [lo, hi): every distinct image of the batch is read and uploaded once, all crops
        come from one launch (datacrop.dataset_crop); scale = sc * scale, bbox_info and focal_length as base_dataset.py:325-331."""
        from PIL import Image
        from . import datacrop
        from .tester import calculate_bbox_info, calculate_focal_length
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)   # noqa: E731
        names = self.imgname[lo:hi]
        distinct = list(dict.fromkeys(names))
        slot = {nm: k for k, nm in enumerate(distinct)}
        frames = [np.array(Image.open(os.path.join(self.img_dir, nm)).convert("RGB")) for nm in distinct]
        images = [datacrop.upload_image(fr, device) for fr in frames]
        idx = [slot[nm] for nm in names]
        params = datacrop.batch_params(self.center[lo:hi], self.scale[lo:hi], self.aug_rot[lo:hi], self.aug_flip[lo:hi], self.aug_pn[lo:hi],
                                       self.aug_scale[lo:hi], self.res)
        self.last_occ_mask = None
        if self.occlude is not None and self.want_occ_mask:
            # eval.py --visibility: the same crops and cover from the launch that also writes the per-pixel mask
            img, cover, self.last_occ_mask = datacrop.dataset_crop(images, idx, params, self.res, not self.raw_crop, want_mask=True,
                                                                   occlusion=(self.occlude.atlas(device), self.occ_records[lo:hi]))
            self._occ_pending.append((lo, hi, cover))
        elif self.occlude is not None:
            img, cover = datacrop.dataset_crop(images, idx, params, self.res, not self.raw_crop,
                                               occlusion=(self.occlude.atlas(device), self.occ_records[lo:hi]))
            self._occ_pending.append((lo, hi, cover))
        else:
            img = datacrop.dataset_crop(images, idx, params, self.res, not self.raw_crop)
        shapes = np.asarray([frames[k].shape[:2] for k in idx], np.float32)
        center, scale = self.center[lo:hi], self.scale_eff[lo:hi].astype(np.float32)      # float32, as the file's scale is held here
        info = np.stack([calculate_bbox_info(c, s, hw) for c, s, hw in zip(center, scale, shapes)])
        focal = np.array([calculate_focal_length(h, w) for h, w in shapes], np.float32)
        return {"img": img, "bbox_info": t(info), "focal_length": t(focal), "scale": t(scale), "center": t(center),
                "orig_shape": t(shapes)}

    def __len__(self) -> int:
        return len(self.imgname)

    def batch(self, lo: int, hi: int, device) -> Dict[str, torch.Tensor]:
        """Model inputs of samples [lo, hi) (the dict of tester.py:205-212) on the device."""
        if self.crop == "dataset":
            return self._batch_dataset_crop(lo, hi, device)
        from .tester import calculate_bbox_info, calculate_focal_length, crop_normalize
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)   # noqa: E731
        center, scale = self.center[lo:hi], self.scale[lo:hi]
        if self.img is not None:
            img = t(self.img[lo:hi])
            shapes = self.orig_shape[lo:hi] if self.orig_shape is not None else np.tile([[224.0, 224.0]], (hi - lo, 1))
        else:
            from PIL import Image
            crops, shapes = [], []
            for i in range(lo, hi):
                fr = np.array(Image.open(os.path.join(self.img_dir, self.imgname[i])).convert("RGB"))
                side = float(self.scale[i]) * 200.0
                box = torch.tensor([[self.center[i, 0], self.center[i, 1], side, side]], dtype=torch.float32, device=device)
                crops.append(crop_normalize(torch.from_numpy(np.ascontiguousarray(fr)).to(device), box, self.bbox_scale))
                shapes.append(fr.shape[:2])
            img, shapes = torch.cat(crops), np.asarray(shapes, np.float32)
        info = np.stack([calculate_bbox_info(c, s, hw) for c, s, hw in zip(center, scale, shapes)])
        focal = np.array([calculate_focal_length(h, w) for h, w in shapes], np.float32)
        return {"img": img, "bbox_info": t(info), "focal_length": t(focal), "scale": t(scale), "center": t(center),
                "orig_shape": t(shapes)}


@torch.no_grad()
def run_eval(model, dataset: EvalDataset, J_regressor, batch_size: int = 64, kinematic: bool = True,
             sel_uncert_part: Optional[Sequence[int]] = None, save_results: bool = False, return_records: bool = False,
             likelihood: bool = False, rank_metrics: Optional[int] = None, visibility=None, calibrate=None, bootstrap=None) -> Dict[str, object]:
    """trainer.py:298-336 over a whole dataset: forward, then the metrics of every batch (the ragged last one included) on the
    device.  SMPL ground truth: gt_vertices = POCO.smpl_lbs(shape, poco_op_rodrigues(pose)) (base_dataset.py:353-366, neutral
    model), also on the device.  Returns Evaluator.finish() plus `imgname`.  likelihood=True (needs `pose` in the dataset and
    cond_layer in the checkpoint): also the held-out flow NLL of every batch on the same stream (LikelihoodAccumulator: val_nll,
    val_log_phi, val_log_sigma, log_phi / log_sigma / bar_pose [N,24]) and Evaluator.uncert_summary() (val_mpjpe_var, val_var).
    rank_metrics=K (eval.py --rank_metrics --rank_bins K): also ranking.RankMetrics of the records with K cuts - the
    ranking.RANK_NPZ_KEYS arrays; everything else is what it is without the argument.
    visibility (eval.py --visibility): a visibility.VisibilityEval from visibility.prepare(); behind the metrics of every batch, on
    the same stream, it counts the visible pixels of every body part of the ground-truth mesh; the result gains the
    visibility.NPZ_KEYS arrays and `vis_stats`.  Needs SMPL ground truth; without the argument nothing changes.
    calibrate (eval.py --calibrate): dict(split, bins, meta); the result gains `calibration` (the calibrate.NPZ_KEYS arrays, for
    calibrate.save) and the array `calib_summary`; everything else is what it is without the argument.
    bootstrap (eval.py --bootstrap): a bootstrap.BootSpec; the result gains the bootstrap.NPZ_KEYS arrays (and boot_replicates with
    save_results), computed from the records after finish(); everything else is what it is without the argument."""
    from . import ops
    dev = model.device
    ev = Evaluator(J_regressor, joint_map(dataset.name), capacity=len(dataset), sel_uncert_part=sel_uncert_part, kinematic=kinematic,
                   device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    if likelihood and not dataset.has_pose:
        raise ValueError("likelihood=True needs a dataset with `pose` (the flow scores the ground-truth pose)")
    lk = LikelihoodAccumulator(model, capacity=len(dataset)) if likelihood else None
    for lo in range(0, len(dataset), batch_size):
        hi = min(lo + batch_size, len(dataset))
        out = model(dataset.batch(lo, hi, dev), want_segm=False)
        gt_pose = t(dataset.pose[lo:hi])
        if lk is not None:
            lk.step(out, gt_pose)
        if dataset.gt_form == "smpl":
            gt_verts, gt_j49 = model.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))
            ev.step(out, gt_pose, gt_vertices=gt_verts)
            if visibility is not None:
                visibility.step(lo, hi, gt_verts, gt_j49, dataset.last_occ_mask)
        else:
            ev.step(out, gt_pose, gt_joints=t(dataset.joints[lo:hi]))
    res = ev.finish(save_results=save_results, return_records=return_records)
    if lk is not None:
        res.update(ev.uncert_summary())
        res.update(lk.finish())
    if rank_metrics is not None:
        from .ranking import RankMetrics
        res.update(RankMetrics(ev, int(rank_metrics)).result)
    if visibility is not None:
        res.update(visibility.finish(res["corr_x"], res["corr_y"]))
    if calibrate is not None:
        from . import calibrate as calib
        res["calibration"] = calib.calibrate(ev, calibrate.get("split", "half"), int(calibrate.get("bins", 20)), calibrate.get("meta"))
        res["calib_summary"] = res["calibration"]["calib_summary"]
    if bootstrap is not None:
        res.update(_bootstrap([("", ev)], bootstrap, dataset, save_results))
    model.check_status()
    res["imgname"] = np.asarray(dataset.imgname)
    ev.close()
    return res


def _bootstrap(evaluators, spec, dataset: "EvalDataset", save_replicates: bool) -> Dict[str, object]:
    """bootstrap.bootstrap_evaluators on the run's evaluators, after their finish() calls (eval.py --bootstrap)."""
    from .bootstrap import bootstrap_evaluators
    return bootstrap_evaluators(evaluators, spec, imgname=dataset.imgname, person_id=dataset.person_id, save_replicates=save_replicates)


SEQ_NPZ_KEYS = ("seq_track", "seq_frame", "seq_accel", "seq_accel_err", "seq_track_names", "seq_pipelines", "seq_summary")


def _seq_accel(ev: "Evaluator", order_d, frames_d, offsets):
    """ops.track_accel on the evaluator's records gathered into track-major rows: the joints are read where they lie in the
    records (row stride RECORD_FLOATS).  -> (the gathered records, the operator's result)."""
    from . import ops
    rec = ev.copy_records(order_d)
    W = 3 * ev.M
    return rec, ops.track_accel(rec[:, R_PRED:R_PRED + W], rec[:, R_GT:R_GT + W], frames_d, offsets)


def _seq_row(res: Dict[str, object], total: np.ndarray, changed: float, n: int) -> np.ndarray:
    """One row of seq_summary (sequences.SUMMARY_FIELDS): MPJPE, PA-MPJPE, V2V, then Accel and Accel error x 1000 as means over the
    valid rows (NaN without one), the share of changed joint-frames and the share of valid rows."""
    cnt = float(total[2])
    acc, err = (1000.0 * float(total[1]) / cnt, 1000.0 * float(total[0]) / cnt) if cnt > 0 else (float("nan"), float("nan"))
    return np.array([res["val_mpjpe"], res["val_pampjpe"], res["val_v2v"], acc, err, changed, cnt / max(n, 1)], np.float64)


@torch.no_grad()
def run_eval_sequences(model, dataset: EvalDataset, J_regressor, batch_size: int = 64, kinematic: bool = True,
                       sel_uncert_part: Optional[Sequence[int]] = None, save_results: bool = False, return_records: bool = False,
                       pipelines=(), max_gap: int = 30, uncert_ref: float = 0.3, min_cutoff: float = 0.004,
                       beta: float = 1.5) -> Dict[str, object]:
    """run_eval on a dataset whose rows are consecutive frames (eval.py --sequences).  The loop is run_eval's;
    what it returns under run_eval's keys is bit for bit what run_eval returns.  The rows are grouped into tracks
    (sequences.group_tracks), the records are gathered track-major on the device and ops.track_accel scores them: seq_track /
    seq_frame / seq_accel / seq_accel_err [N] in file order (NaN where a row has no two neighbours at consecutive frames),
    seq_track_names, and seq_summary [1 + pipelines, 7] (sequences.SUMMARY_FIELDS; row 0 = the raw prediction).
    pipelines (sequences.parse_pipelines): each chain of video mode's post-processing operators is run on the device tensors of
    pose, shape and processed uncertainty kept from the loop - ops.track_infill, ops.track_smooth, the one-euro filter on the host -
    re-posed with model.smpl_lbs (the rows the in-fill touched; every row after a smoother) and scored with a second Evaluator
    stepped over the same batches against the same ground truth, and with ops.track_accel."""
    from . import ops
    from .sequences import group_tracks, pipeline_text
    dev, n = model.device, len(dataset)
    pipelines = list(pipelines)
    new_ev = lambda: Evaluator(J_regressor, joint_map(dataset.name), capacity=n, sel_uncert_part=sel_uncert_part,   # noqa: E731
                               kinematic=kinematic, device=dev)
    ev = new_ev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    g = group_tracks(dataset.imgname, dataset.person_id)                # refuses before any GPU work

    def ground_truth(lo, hi):
        gt_pose = t(dataset.pose[lo:hi])
        if dataset.gt_form == "smpl":
            return gt_pose, {"gt_vertices": model.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))[0]}
        return gt_pose, {"gt_joints": t(dataset.joints[lo:hi])}

    keep = None
    for lo in range(0, n, batch_size):
        hi = min(lo + batch_size, n)
        out = model(dataset.batch(lo, hi, dev), want_segm=False)
        gt_pose, gt = ground_truth(lo, hi)
        ev.step(out, gt_pose, **gt)
        if pipelines:
            if keep is None:
                keep = {k: torch.empty((n,) + tuple(out[k].shape[1:]), device=dev, dtype=torch.float32)
                        for k in ("pred_pose", "pred_shape", "var_pose", "smpl_vertices")}
            for k, buf in keep.items():
                buf[lo:hi].copy_(out[k])
    res = ev.finish(save_results=save_results, return_records=return_records)
    order_d, frames_d = torch.from_numpy(g["order"]).to(dev), torch.from_numpy(g["frames"]).to(dev)
    offsets = torch.from_numpy(g["offsets"])
    rec, acc = _seq_accel(ev, order_d, frames_d, offsets)
    P = len(g["names"])
    order = g["order"].astype(np.int64)

    def to_file_order(x, fill):
        a = np.full(n, fill, x.dtype)
        a[order] = x
        return a
    res["seq_track"] = to_file_order(np.repeat(np.arange(P, dtype=np.int32), np.diff(g["offsets"])), 0)
    res["seq_frame"] = to_file_order(g["frames"], 0)
    res["seq_accel"] = to_file_order(acc["accel"].cpu().numpy(), np.float32(np.nan))
    res["seq_accel_err"] = to_file_order(acc["accel_err"].cpu().numpy(), np.float32(np.nan))
    res["seq_track_sums"], res["seq_total"] = acc["track_sums"].cpu().numpy(), acc["total"].cpu().numpy()
    res["seq_track_names"] = np.asarray(g["names"])
    res["seq_pipelines"] = np.asarray([pipeline_text(p) for p in pipelines], dtype=str)
    rows = [_seq_row(res, res["seq_total"], 0.0, n)]
    if pipelines:
        order_l = order_d.long()
        u = rec[:, R_UNC:R_UNC + 24].contiguous()                       # the processed uncertainty, as regressed, for every step
        pose_t, betas_t = keep["pred_pose"].index_select(0, order_l), keep["pred_shape"].index_select(0, order_l)
        bs = max(int(model.max_batch), 1)
        res["seq_post"] = []
    for steps in pipelines:
        pose, betas = pose_t, betas_t
        stale = torch.zeros(n, dtype=torch.bool, device=dev)            # track-major rows whose mesh no longer fits their pose
        for name, val in steps:
            if name == "infill":
                pose, betas, _, touched = ops.track_infill(pose, u, frames_d, offsets, betas, float(val), int(max_gap))
                stale |= touched.bool()
            elif name == "smooth_uncert":
                pose, betas, _ = ops.track_smooth(pose, u, frames_d, offsets, betas, float(val), float(uncert_ref), int(max_gap))
                stale[:] = True
            else:
                from .smooth import one_euro_rotmats
                host = pose.cpu().numpy()
                pose = torch.from_numpy(np.concatenate([one_euro_rotmats(host[a:b], min_cutoff, beta)
                                                        for a, b in zip(g["offsets"][:-1], g["offsets"][1:])]).astype(np.float32)).to(dev)
                stale[:] = True
        verts = keep["smpl_vertices"].clone()                           # file order
        sel_all = torch.nonzero(stale).reshape(-1)                      # ascending, re-posed as infill.py / usmooth.py do
        for lo in range(0, int(sel_all.numel()), bs):
            sel = sel_all[lo:lo + bs]
            v, _ = model.smpl_lbs(betas.index_select(0, sel).contiguous(), pose.index_select(0, sel))
            verts.index_copy_(0, order_l.index_select(0, sel), v)
        pose_f = torch.empty_like(pose)
        pose_f.index_copy_(0, order_l, pose)
        ev2 = new_ev()
        for lo in range(0, n, batch_size):
            hi = min(lo + batch_size, n)
            gt_pose, gt = ground_truth(lo, hi)
            ev2.step({"smpl_vertices": verts[lo:hi], "pred_pose": pose_f[lo:hi], "var_pose": keep["var_pose"][lo:hi]}, gt_pose, **gt)
        r2 = ev2.finish(save_results=save_results)
        _, acc2 = _seq_accel(ev2, order_d, frames_d, offsets)
        changed = float((pose != pose_t).reshape(n, 24, 9).any(-1).sum().item()) / float(n * 24)
        r2["seq_accel"] = to_file_order(acc2["accel"].cpu().numpy(), np.float32(np.nan))
        r2["seq_accel_err"] = to_file_order(acc2["accel_err"].cpu().numpy(), np.float32(np.nan))
        r2["seq_total"] = acc2["total"].cpu().numpy()
        r2["pose"] = pose_f.cpu().numpy()
        rows.append(_seq_row(r2, r2["seq_total"], changed, n))
        res["seq_post"].append(r2)
        ev2.close()
    res["seq_summary"] = np.stack(rows)
    model.check_status()
    res["imgname"] = np.asarray(dataset.imgname)
    ev.close()
    return res


def sequence_lines(res: Dict[str, object]):
    """eval.py --sequences: Accel and Accel error (mm / frame^2) of the raw prediction, the tracks and the share of valid rows, then
    one line per --seq_post pipeline with every figure's difference to the raw prediction."""
    s = res["seq_summary"]
    lines = [f"Accel: {s[0, 3]}", f"Accel error: {s[0, 4]}",
             f"Tracks: {len(res['seq_track_names'])} (rows with both neighbours at consecutive frames: {100.0 * s[0, 6]:.2f} %)"]
    for name, row in zip(res["seq_pipelines"], s[1:]):
        d = row - s[0]
        lines.append(f"Post {name}: MPJPE {row[0]:.4f} ({d[0]:+.4f}), PA-MPJPE {row[1]:.4f} ({d[1]:+.4f}), V2V {row[2]:.4f} ({d[2]:+.4f}), "
                     f"Accel {row[3]:.4f} ({d[3]:+.4f}), Accel error {row[4]:.4f} ({d[4]:+.4f}), changed {100.0 * row[5]:.2f} % of "
                     "joint-frames")
    return lines


PAIR_SCALARS = ("val_oracle_mpjpe", "val_oracle_pampjpe", "select_accuracy", "select_share_m2")


def selection_summary(crop_mpjpe, crop_pampjpe, select) -> Dict[str, float]:
    """What the records of two models say about a selection, in float64 on the host.  crop_mpjpe / crop_pampjpe: ([N], [N]) = the
    two models' per-crop values (record words 0 and 1, metres); select [N,24].  val_oracle_* = 1000 x the mean over the crops of the
    smaller of the two values - the bound no selection beats; select_accuracy = the share of crops whose chosen model (the model of
    the root joint) is not the worse one in MPJPE (equal values count as right); select_share_m2 = the share taken from model 2."""
    root = np.asarray(select).reshape(-1, 24)[:, 0] != 0
    a1, a2 = (np.asarray(x, np.float64) for x in crop_mpjpe)
    p1, p2 = (np.asarray(x, np.float64) for x in crop_pampjpe)
    n = float(len(root))
    # 1000.0 * sum / n as eval_finish forms its means, the sum rounded once: where one model is the better on every crop the oracle
    # is that model's own mean whenever the device's fp64 sum of the fp32 values is exact, not one rounding above it
    return {"val_oracle_mpjpe": 1000.0 * math.fsum(np.minimum(a1, a2)) / n, "val_oracle_pampjpe": 1000.0 * math.fsum(np.minimum(p1, p2)) / n,
            "select_accuracy": float(np.where(root, a2 <= a1, a1 <= a2).mean()), "select_share_m2": float(root.mean())}


@torch.no_grad()
def run_eval_pair(pair, dataset: EvalDataset, J_regressor, batch_size: int = 64, kinematic: bool = True,
                  sel_uncert_part: Optional[Sequence[int]] = None, save_results: bool = False, bootstrap=None) -> Dict[str, object]:
    """run_eval with a second model (eval.py --cfg2 --ckpt2): per batch RegressorPair.forward_all, then three
    Evaluators - model 1, model 2, selected - stepped against the same ground truth on the same stream; the choices are kept in
    device buffers, so nothing goes to the host between the forward and the three finish() calls.  Returns the selected result
    under run_eval's keys, the two models' mpjpe / pampjpe / v2v and val_* with suffixes _m1 and _m2, their per-crop record values
    crop_mpjpe_m* / crop_pampjpe_m* [N], select [N,24] uint8, select_score [N,2] and selection_summary of them.
    bootstrap: a bootstrap.BootSpec; the result gains the bootstrap.NPZ_KEYS arrays for Model 1, Model 2 and Selected, the latter two
    also as paired differences to Model 1; nothing else changes."""
    from . import ops
    dev, n = pair.device, len(dataset)
    evs = [Evaluator(J_regressor, joint_map(dataset.name), capacity=n, sel_uncert_part=sel_uncert_part, kinematic=kinematic, device=dev)
           for _ in range(3)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    select = torch.zeros(n, 24, dtype=torch.uint8, device=dev)
    score = torch.zeros(n, 2, dtype=torch.float32, device=dev)
    for lo in range(0, n, batch_size):
        hi = min(lo + batch_size, n)
        outs = pair.forward_all(dataset.batch(lo, hi, dev))
        select[lo:hi].copy_(outs[2]["select"])
        score[lo:hi].copy_(outs[2]["select_score"])
        gt_pose = t(dataset.pose[lo:hi])
        if dataset.gt_form == "smpl":
            gt = {"gt_vertices": pair.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))[0]}
        else:
            gt = {"gt_joints": t(dataset.joints[lo:hi])}
        for ev, out in zip(evs, outs):
            ev.step(out, gt_pose, **gt)
    solo = [ev.finish(return_records=True) for ev in evs[:2]]
    res = evs[2].finish(save_results=save_results)
    for tag, r in zip(("_m1", "_m2"), solo):
        res.update({k + tag: r[k] for k in ("mpjpe", "pampjpe", "v2v", "val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")})
        res["crop_mpjpe" + tag], res["crop_pampjpe" + tag] = r["records"][:, R_MPJPE].copy(), r["records"][:, R_PA].copy()
    res["select"], res["select_score"] = select.cpu().numpy(), score.cpu().numpy()
    res.update(selection_summary((res["crop_mpjpe_m1"], res["crop_mpjpe_m2"]), (res["crop_pampjpe_m1"], res["crop_pampjpe_m2"]),
                                 res["select"]))
    if bootstrap is not None:
        res.update(_bootstrap(list(zip(("Model 1", "Model 2", "Selected"), evs)), bootstrap, dataset, save_results))
    pair.check_status()
    res["imgname"] = np.asarray(dataset.imgname)
    for ev in evs:
        ev.close()
    return res


def pair_report_lines(res: Dict[str, object], mode: str = "crop"):
    """report_lines for model 1, model 2 and the selection, labelled, then the oracle, the selection accuracy and model 2's share."""
    lines = []
    for label, tag in (("Model 1", "_m1"), ("Model 2", "_m2")):
        lines += [f"{label} MPJPE: {res['val_mpjpe' + tag]}", f"{label} PA-MPJPE: {res['val_pampjpe' + tag]}",
                  f"{label} V2V (mm): {res['val_v2v' + tag]}", f"{label} Uncert Error Correlation: {res['val_corr' + tag]}"]
    lines += [f"Selected ({mode}) {line}" for line in report_lines(res)]
    return lines + [f"Oracle MPJPE: {res['val_oracle_mpjpe']}", f"Oracle PA-MPJPE: {res['val_oracle_pampjpe']}",
                    f"Selection accuracy: {res['select_accuracy']}", f"Crops from model 2: {res['select_share_m2']}"]


TTA_SCALARS = tuple(k + "_base" for k in ("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")) + ("val_corr_spread",)
TTA_OUTPUT_KEYS = ("pred_pose", "var_pose", "pred_shape", "smpl_vertices", "smpl_joints3d", "smpl_joints2d", "pred_cam")


@torch.no_grad()
def run_eval_tta(tta_model, dataset: EvalDataset, J_regressor, batch_size: int = 64, kinematic: bool = True,
                 sel_uncert_part: Optional[Sequence[int]] = None, save_results: bool = False, return_outputs: bool = False,
                 bootstrap=None) -> Dict[str, object]:
    """run_eval with test-time views (eval.py --tta): per batch of b = max(1, batch_size // K) crops the K * b
    views are cut in one launch (tta.dataset_batch), TTAModel.forward_all regresses and fuses them, and three Evaluators are
    stepped against the base frame's ground truth on the same stream: the base view, the fused result, and the fused result with
    var_pose := tta_spread and kinematic off, whose correlation is Corr(view spread, pose distance).  Nothing goes to the host
    between the forward and the three finish() calls.  Returns the fused result under run_eval's keys, the base view's mpjpe /
    pampjpe / v2v and val_* with suffix _base, val_corr_spread, tta_spread [N,24] and tta_views [K,3] (flip, rot, scale).
    return_outputs (tests): also `outputs` = per batch (the K per-view dicts, the fused dict) of host arrays.
    bootstrap: a bootstrap.BootSpec; the result gains the bootstrap.NPZ_KEYS arrays for Base view and Fused and their paired
    difference; nothing else changes."""
    from . import ops, tta
    if dataset.crop != "dataset":
        raise ValueError("run_eval_tta cuts its views with the dataset crop: the dataset needs crop='dataset'")
    if dataset.occlude is not None or dataset.augment.random or np.any(dataset.aug_flip) or np.any(dataset.aug_rot) or np.any(dataset.aug_scale != 1) \
            or np.any(dataset.aug_pn != 1):
        raise ValueError("run_eval_tta makes its own views of the unperturbed crop: the dataset may carry no augmentation")
    dev, n, views = tta_model.device, len(dataset), tta_model.views
    b = max(1, min(int(batch_size) // len(views), tta_model.max_batch))
    kw = dict(capacity=n, sel_uncert_part=sel_uncert_part, device=dev)
    evs = [Evaluator(J_regressor, joint_map(dataset.name), kinematic=kinematic, **kw), Evaluator(J_regressor, joint_map(dataset.name), kinematic=kinematic, **kw),
           Evaluator(J_regressor, joint_map(dataset.name), kinematic=False, **kw)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    spread = torch.zeros(n, 24, dtype=torch.float32, device=dev)
    outputs = []
    for lo in range(0, n, b):
        hi = min(lo + b, n)
        per_view, fused = tta_model.forward_all(tta.dataset_batch(dataset, lo, hi, views, dev))
        spread[lo:hi].copy_(fused["tta_spread"])
        gt_pose = t(dataset.pose[lo:hi])
        if dataset.gt_form == "smpl":
            gt = {"gt_vertices": tta_model.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))[0]}
        else:
            gt = {"gt_joints": t(dataset.joints[lo:hi])}
        by_spread = dict(fused)
        by_spread["var_pose"] = fused["tta_spread"]
        for ev, out in zip(evs, (per_view[0], fused, by_spread)):
            ev.step(out, gt_pose, **gt)
        if return_outputs:
            host = lambda d: {k: d[k].cpu().numpy() for k in TTA_OUTPUT_KEYS + ("tta_spread",) if k in d}   # noqa: E731
            outputs.append(([host(v) for v in per_view], host(fused)))
    base = evs[0].finish()
    by_spread = evs[2].finish()
    res = evs[1].finish(save_results=save_results)
    res.update({k + "_base": base[k] for k in ("mpjpe", "pampjpe", "v2v", "val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")})
    res["val_corr_spread"] = by_spread["val_corr"]
    res["tta_spread"] = spread.cpu().numpy()
    res["tta_views"] = np.asarray([[float(v.flip), float(v.rot), float(v.scale)] for v in views], np.float64)
    res["tta_weight"] = tta_model.weight
    if bootstrap is not None:
        res.update(_bootstrap([("Base view", evs[0]), ("Fused", evs[1])], bootstrap, dataset, save_results))
    if return_outputs:
        res["outputs"] = outputs
    tta_model.check_status()
    res["imgname"] = np.asarray(dataset.imgname)
    for ev in evs:
        ev.close()
    return res


def tta_report_lines(res: Dict[str, object]):
    """The reference's lines for the base view and the fused result, then the correlation between the views' spread and the pose
    distance - the baseline a learnt uncertainty is compared against."""
    lines = [f"Base view MPJPE: {res['val_mpjpe_base']}", f"Base view PA-MPJPE: {res['val_pampjpe_base']}",
             f"Base view V2V (mm): {res['val_v2v_base']}", f"Base view Uncert Error Correlation: {res['val_corr_base']}"]
    label = f"Fused ({res['tta_weight']}, {len(res['tta_views'])} views)"
    lines += [f"{label} {line}" for line in report_lines(res)]
    return lines + [f"Corr(view spread, pose distance): {res['val_corr_spread']}"]


CORRUPT_SUMMARY_FIELDS = ("mpjpe", "pampjpe", "v2v", "corr", "var_mean", "var_median", "d_mpjpe", "d_pampjpe", "d_v2v", "d_var")
CORRUPT_SCALARS = ("val_corr_dvar_dmpjpe", "val_spearman_dvar_dmpjpe")


@torch.no_grad()
def run_eval_corrupt(cmodel, dataset: EvalDataset, J_regressor, batch_size: int = 64, kinematic: bool = True,
                     sel_uncert_part: Optional[Sequence[int]] = None, save_results: bool = False, return_outputs: bool = False,
                     bootstrap=None) -> Dict[str, object]:
    """run_eval under image degradation (eval.py --corrupt): per batch of b = max(1, batch_size // K) crops the
    dataset crop hands over the raw crops (after --aug_* / --aug_occlude), corrupt.CorruptModel makes their K level-major versions -
    level 0 the clean crop - and regresses them in one forward, and K Evaluators are stepped against the same ground truth on the
    same stream.  Returns level 0 under run_eval's keys; per level k the per-crop arrays mpjpe_l<k> / pampjpe_l<k> [N,M], v2v_l<k>
    and var_l<k> [N] (the mean of the crop's 24 processed uncertainties); corrupt_summary [K, 10] (CORRUPT_SUMMARY_FIELDS: the
    headline numbers, mean and median var, and the differences to level 0 in mm and in var); corrupt_levels; and over crops x
    levels >= 1 Pearson's and Spearman's Corr(var_k - var_0, MPJPE_k - MPJPE_0) through ops.pearson64 / ops.rank_curve.
    return_outputs (tests): also `outputs` = per batch the K per-level dicts of host arrays and `level_imgs` = the K * b crops the
    forward was given.  bootstrap: a bootstrap.BootSpec; every level gets its lines and every level after the first its paired
    difference to level 0."""
    from . import corrupt, ops
    if dataset.crop != "dataset":
        raise ValueError("run_eval_corrupt degrades the raw crops of the dataset crop: the dataset needs crop='dataset'")
    dev, n, levels, K = cmodel.device, len(dataset), cmodel.levels, cmodel.K
    b = max(1, min(int(batch_size) // K, cmodel.max_batch))
    evs = [Evaluator(J_regressor, joint_map(dataset.name), capacity=n, sel_uncert_part=sel_uncert_part, kinematic=kinematic, device=dev)
           for _ in range(K)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    outputs = []
    dataset.raw_crop = True
    try:
        for lo in range(0, n, b):
            hi = min(lo + b, n)
            lb = cmodel.level_batch(dataset.batch(lo, hi, dev), range(lo, hi))
            outs = cmodel.forward_rows(lb)
            gt_pose = t(dataset.pose[lo:hi])
            if dataset.gt_form == "smpl":
                gt = {"gt_vertices": cmodel.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))[0]}
            else:
                gt = {"gt_joints": t(dataset.joints[lo:hi])}
            for ev, out in zip(evs, outs):
                ev.step(out, gt_pose, **gt)
            if return_outputs:
                outputs.append(dict(level_imgs=lb["img"].cpu().numpy(),
                                    levels=[{k: o[k].cpu().numpy() for k in TTA_OUTPUT_KEYS if k in o} for o in outs]))
    finally:
        dataset.raw_crop = False
    res = evs[0].finish(save_results=save_results, return_records=True)
    per = [res] + [ev.finish(return_records=True) for ev in evs[1:]]
    summ = np.zeros((K, len(CORRUPT_SUMMARY_FIELDS)))
    crop_var = [r["records"][:, R_UNC:R_UNC + 24].astype(np.float64).mean(axis=1) for r in per]
    crop_err = [r["records"][:, R_MPJPE].astype(np.float64) for r in per]
    for k, r in enumerate(per):
        res[f"mpjpe_l{k}"], res[f"pampjpe_l{k}"], res[f"v2v_l{k}"] = r["mpjpe"].copy(), r["pampjpe"].copy(), r["v2v"].copy()
        res[f"var_l{k}"] = crop_var[k]
        summ[k, :6] = r["val_mpjpe"], r["val_pampjpe"], r["val_v2v"], r["val_corr"], crop_var[k].mean(), np.median(crop_var[k])
        summ[k, 6:9] = summ[k, :3] - summ[0, :3]
        summ[k, 9] = summ[k, 4] - summ[0, 4]
    res.pop("records")
    res["corrupt_summary"], res["corrupt_levels"] = summ, np.asarray([corrupt.describe(lv) for lv in levels])
    dvar = torch.from_numpy(np.concatenate([crop_var[k] - crop_var[0] for k in range(1, K)])).to(dev)
    derr = torch.from_numpy(np.concatenate([crop_err[k] - crop_err[0] for k in range(1, K)])).to(dev)
    res["val_corr_dvar_dmpjpe"] = float(ops.pearson64(dvar, derr).item())
    ranks = [ops.rank_curve(v.to(torch.float32).contiguous(), None, 1)["rank"] for v in (dvar, derr)]
    res["val_spearman_dvar_dmpjpe"] = float(ops.pearson64(ranks[0], ranks[1]).item())
    if bootstrap is not None:
        res.update(_bootstrap([(f"Level {k} ({corrupt.describe(lv)})", ev) for k, (lv, ev) in enumerate(zip(levels, evs))], bootstrap, dataset,
                              save_results))
    if return_outputs:
        res["outputs"] = outputs
    cmodel.check_status()
    res["imgname"] = np.asarray(dataset.imgname)
    for ev in evs:
        ev.close()
    return res


def corrupt_report_lines(res: Dict[str, object]):
    """Per level the usual lines, mean and median var and the differences to the clean crop; then the two correlations."""
    lines = []
    for k, (name, row) in enumerate(zip(res["corrupt_levels"], np.asarray(res["corrupt_summary"]))):
        s = dict(zip(CORRUPT_SUMMARY_FIELDS, row))
        label = f"Level {k} ({name})"
        lines += [f"{label} MPJPE: {s['mpjpe']}", f"{label} PA-MPJPE: {s['pampjpe']}", f"{label} V2V (mm): {s['v2v']}",
                  f"{label} Uncert Error Correlation: {s['corr']}", f"{label} var mean / median: {s['var_mean']} / {s['var_median']}"]
        if k:
            lines.append(f"{label} - clean: MPJPE {s['d_mpjpe']:+}, PA-MPJPE {s['d_pampjpe']:+}, V2V {s['d_v2v']:+} (mm), var {s['d_var']:+}")
    return lines + [f"N: {res['N']}", f"Corr(delta var, delta MPJPE) over crops x levels: Pearson {res['val_corr_dvar_dmpjpe']}, "
                                       f"Spearman {res['val_spearman_dvar_dmpjpe']}"]


REFIT_SCALARS = tuple(k + "_raw" for k in ("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")) + ("refit_mean_shift", "refit_corr_shift_var")


@torch.no_grad()
def run_eval_refit(model, dataset: EvalDataset, J_regressor, tables, lam: float, u_ref: float = 0.3, rho: float = 0.1,
                   conf_thresh: float = 0.3, iters: int = 10, batch_size: int = 64, kinematic: bool = True,
                   sel_uncert_part: Optional[Sequence[int]] = None, save_results: bool = False, bootstrap=None) -> Dict[str, object]:
    """run_eval with the keypoint refit (eval.py --kp_refit): per batch the forward, then refit.refit_rows on the
    batch's pose, processed uncertainty (trailing axes averaged, accumulated along the tree when `kinematic`) and shape against the
    dataset's `openpose` keypoints - camera a = s h / 2 from pred_cam, (px, py) = the box centre, norm = h = 200 scale - then LBS of
    the refitted pose (a row that was not fitted keeps the network's mesh), and two Evaluators stepped against the same ground truth
    on the same stream: the raw prediction and the refit.  tables = refit.joint_tables(the body model).  Returns the refit's result
    under run_eval's keys, the raw prediction's mpjpe / pampjpe / v2v and val_* with suffix _raw, refit_shift [N,24], refit_cost
    [N,2], refit_flag [N], refit_mean_shift and refit_corr_shift_var (Pearson r of shift and processed uncertainty over the fitted
    rows).  bootstrap: a bootstrap.BootSpec; the result gains the bootstrap.NPZ_KEYS arrays for Raw and Refit and their paired
    difference; nothing else changes."""
    from . import ops, refit
    from .synth import SMPL_PARENTS
    if dataset.openpose is None:
        raise ValueError("the keypoint refit needs `openpose` [N,25,3] in the dataset file (demo.py --save_dataset writes it)")
    dev, n = model.device, len(dataset)
    kw = dict(capacity=n, sel_uncert_part=sel_uncert_part, kinematic=kinematic, device=dev)
    evs = [Evaluator(J_regressor, joint_map(dataset.name), **kw), Evaluator(J_regressor, joint_map(dataset.name), **kw)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    shift = torch.zeros(n, 24, dtype=torch.float32, device=dev)
    cost = torch.zeros(n, 2, dtype=torch.float32, device=dev)
    flag = torch.zeros(n, dtype=torch.int32, device=dev)
    uvar = torch.zeros(n, 24, dtype=torch.float32, device=dev)
    for lo in range(0, n, batch_size):
        hi = min(lo + batch_size, n)
        batch = dataset.batch(lo, hi, dev)
        out = model(batch, want_segm=False)
        var = out["var_pose"].float()
        while var.dim() > 2:
            var = var.mean(-1)
        var = var.clone()
        if kinematic:
            for j in range(1, 24):
                var[:, j] += var[:, int(SMPL_PARENTS[j])]
        h = batch["scale"].reshape(-1).float() * 200.0
        pc = out["pred_cam"].float()
        cam = torch.stack([pc[:, 0] * h * 0.5, pc[:, 1], pc[:, 2], batch["center"][:, 0], batch["center"][:, 1]], 1).contiguous()
        fit = refit.refit_rows(tables, out["pred_pose"], var, out["pred_shape"], t(dataset.openpose[lo:hi]), cam, h.contiguous(), lam, u_ref,
                               rho, conf_thresh, iters)
        verts, _ = model.smpl_lbs(out["pred_shape"].contiguous(), fit["pose"])
        fitted = (fit["info"][:, 1] == 0)
        refitted = dict(out)
        refitted["pred_pose"] = fit["pose"]
        refitted["smpl_vertices"] = torch.where(fitted[:, None, None], verts, out["smpl_vertices"]).contiguous()
        shift[lo:hi].copy_(fit["shift"])
        cost[lo:hi].copy_(fit["cost"])
        flag[lo:hi].copy_(fit["info"][:, 1])
        uvar[lo:hi].copy_(var)
        gt_pose = t(dataset.pose[lo:hi])
        if dataset.gt_form == "smpl":
            gt = {"gt_vertices": model.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))[0]}
        else:
            gt = {"gt_joints": t(dataset.joints[lo:hi])}
        evs[0].step(out, gt_pose, **gt)
        evs[1].step(refitted, gt_pose, **gt)
    raw = evs[0].finish()
    res = evs[1].finish(save_results=save_results)
    res.update({k + "_raw": raw[k] for k in ("mpjpe", "pampjpe", "v2v", "val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")})
    res["refit_shift"], res["refit_cost"], res["refit_flag"] = shift.cpu().numpy(), cost.cpu().numpy(), flag.cpu().numpy()
    ok = res["refit_flag"] == 0
    res["refit_mean_shift"] = float(res["refit_shift"][ok].mean()) if ok.any() else 0.0
    res["refit_corr_shift_var"] = refit._pearson(res["refit_shift"][ok].astype(np.float64).reshape(-1),
                                                 uvar.cpu().numpy()[ok].astype(np.float64).reshape(-1))
    if bootstrap is not None:
        res.update(_bootstrap([("Raw", evs[0]), ("Refit", evs[1])], bootstrap, dataset, save_results))
    model.check_status()
    res["imgname"] = np.asarray(dataset.imgname)
    for ev in evs:
        ev.close()
    return res


def refit_report_lines(res: Dict[str, object]):
    """The reference's lines for the raw prediction and for the refit, their difference, and what moved."""
    lines = [f"Raw MPJPE: {res['val_mpjpe_raw']}", f"Raw PA-MPJPE: {res['val_pampjpe_raw']}", f"Raw V2V (mm): {res['val_v2v_raw']}",
             f"Raw Uncert Error Correlation: {res['val_corr_raw']}"]
    lines += [f"Refit {line}" for line in report_lines(res)]
    lines.append("Refit - raw: " + ", ".join(f"{name} {res[k] - res[k + '_raw']:+.4f}" for name, k in
                                             (("MPJPE", "val_mpjpe"), ("PA-MPJPE", "val_pampjpe"), ("V2V", "val_v2v"))))
    n_fit = int((res["refit_flag"] == 0).sum())
    return lines + [f"Refit shift: mean {res['refit_mean_shift']:.3f} deg over {n_fit} fitted of {len(res['refit_flag'])} rows, "
                    f"Pearson r(shift, var) {res['refit_corr_shift_var']:+.3f}"]


def check_occlusion_keys(files) -> None:
    """Synthetic occluders are centred on the ground-truth 2-D keypoints: refuse a dataset file without `part` or with ready-made
    `img` crops (ValueError)."""
    if "img" in files:
        raise ValueError("synthetic occluders are pasted inside the dataset crop, but the file carries ready-made `img` crops: remove "
                         "`img` and pass --img_dir")
    if "part" not in files:
        raise ValueError("synthetic occluders are centred on the ground-truth 2-D keypoints: the dataset file needs `part` [N,24,3] "
                         "(x, y, confidence in image pixels)")


def cover_uncert_corr(occ_cover, corr_y) -> float:
    """Pearson correlation, in float64 on the host, between the covered fraction of each crop and the crop's mean of corr_y (the
    uncertainty of the selected joints, flattened [N * J] as Evaluator.finish hands it out).  NaN when either side is constant."""
    c = np.asarray(occ_cover, np.float64).reshape(-1)
    u = np.asarray(corr_y, np.float64).reshape(len(c), -1).mean(axis=1)
    dc, du = c - c.mean(), u - u.mean()
    den = np.sqrt((dc * dc).sum() * (du * du).sum())
    return float((dc * du).sum() / den) if den > 0 else float("nan")


def occlusion_lines(dataset: "EvalDataset", res: Dict[str, object]):
    """eval.py --aug_occlude: mean objects per crop, mean cover, and the correlation the paper's argument predicts to be positive."""
    lines = [f"Occluders per crop: {float(np.mean(dataset.occ_count))} (skipped objects {dataset.occ_skipped}, crops without a visible "
             f"keypoint {dataset.occ_no_visible})", f"Occluder cover: {float(np.mean(dataset.occ_cover))}"]
    if "corr_y" in res:
        lines.append(f"Corr(cover, uncertainty): {cover_uncert_corr(dataset.occ_cover, res['corr_y'])}")
    return lines


def report_lines(res: Dict[str, object]):
    """The lines of trainer.py:386-391 this port computes."""
    return [f"MPJPE: {res['val_mpjpe']}", f"PA-MPJPE: {res['val_pampjpe']}", f"V2V (mm): {res['val_v2v']}",
            f"Uncert Error Correlation: {res['val_corr']}", f"N: {res['N']}"]


def rank_lines(res: Dict[str, object]):
    """eval.py --rank_metrics: Spearman beside Pearson, AUSE / AURG of the four errors and the threshold table (ranking.rank_lines)."""
    from .ranking import rank_lines as lines
    return lines(res)


def likelihood_lines(res: Dict[str, object]):
    """The two lines of trainer.py:389-390 report_lines leaves out, and the held-out flow NLL (losses.py:346) with its two terms."""
    return [f"Var-MPJPE: {res['val_mpjpe_var']}", f"Variance: {res['val_var']}",
            f"Flow NLL: {res['val_nll']} (log sigma {res['val_log_sigma']}, log phi {res['val_log_phi']}, crops {res['nll_N']})"]


def save_npz(path: str, res: Dict[str, object], dataset_name: str) -> None:
    """evaluation_results_<name>.npz: the numeric arrays of save_results.py:84-92 (the reference joblib-dumps a dict)."""
    keep = {k: v for k, v in res.items() if isinstance(v, np.ndarray) and k not in ("records", "summary") and v.dtype.kind in "fiu"}
    keep.update({k: np.float64(res[k]) for k in ("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")})
    keep["N"] = np.int64(res["N"])
    keep.update({k: np.float64(res[k]) for k in ("val_nll", "val_log_phi", "val_log_sigma", "val_mpjpe_var", "val_var") if k in res})
    pair = PAIR_SCALARS + tuple(k + tag for tag in ("_m1", "_m2") for k in ("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr"))
    keep.update({k: np.float64(res[k]) for k in pair if k in res})           # eval.py --cfg2 --ckpt2 (run_eval_pair)
    keep.update({k: np.float64(res[k]) for k in TTA_SCALARS if k in res})        # eval.py --tta (run_eval_tta)
    keep.update({k: np.float64(res[k]) for k in REFIT_SCALARS if k in res})      # eval.py --kp_refit (run_eval_refit)
    keep.update({k: np.float64(res[k]) for k in CORRUPT_SCALARS if k in res})    # eval.py --corrupt (run_eval_corrupt)
    keep.update({k: res[k] for k in ("corrupt_levels",) if k in res})
    keep.update({k: res[k] for k in ("seq_track_names", "seq_pipelines") if k in res})   # eval.py --sequences (run_eval_sequences)
    keep.update({k: res[k] for k in ("boot_names",) if k in res})                        # eval.py --bootstrap (poco_amd/bootstrap.py)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savez(path, **keep)
