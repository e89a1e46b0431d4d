"""Pseudo-ground-truth export (demo.py --save_dataset): a binding of poco_pseudo_* (include/poco_hip.h, csrc/pseudo_gt.hip) and
the writer of the dataset .npz that pocolib/dataset/base_dataset.py:54-147 - and this project's eval.py --dataset - read.  Per crop
nothing goes to the host between the forward and PseudoLabeler.finish(): the axis-angle pose, the keypoints, the selection by
uncertainty and the compaction of the kept crops are done on the device, into device records.

tests/pseudo_np.py restates the step in numpy and is the yardstick of tests/test_pseudo_*.py."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ._lib import PocoHipError, check, lib

RECORD_FLOATS = 384
MAX_TRAILING = 128
UNWRITTEN = 0xFFFFFFFF
# record offsets (include/poco_hip.h)
P_SRC, P_CENTER, P_SCALE, P_POSE, P_SHAPE, P_VAR, P_OPENPOSE, P_PART, P_S, P_PAD = 0, 1, 3, 4, 76, 86, 110, 185, 257, 353
DATASET_KEYS = ("imgname", "center", "scale", "pose", "shape", "var", "has_smpl", "part", "openpose", "S", "person_id")


def _bind():
    L = lib()
    if getattr(L, "_pseudo_bound", False):
        return L
    L.poco_pseudo_create.argtypes = [C.c_int64, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.poco_pseudo_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.poco_pseudo_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
    L.poco_pseudo_reset.argtypes = [C.c_void_p, C.c_void_p]
    L.poco_pseudo_destroy.argtypes = [C.c_void_p]
    L.poco_pseudo_destroy.restype = None
    L._pseudo_bound = True
    return L


def joints_in_crop(backbone: str) -> bool:
    """The PARE variants hand out smpl_joints2d in crop coordinates, the CLIFF variants in image coordinates (tester.py:225-230)."""
    return "cliff" not in backbone


class PseudoLabeler:
    """Device-side accumulator of dataset records.

        pl = PseudoLabeler(capacity=n_crops, threshold=0.3, backbone="hrnet_w48_cls-cliff")
        pl.step(model(batch), boxes, source_id)                  # per batch, enqueued on the current stream
        arrays = pl.finish(imgname=names, person_id=ids)         # the kept crops, in the order they were offered
        write_dataset("pseudo.npz", arrays)

    threshold None, NaN or <= 0 keeps every crop; otherwise a crop is kept as get_confident_frames keeps a row.  capacity counts the
    crops OFFERED: how many are kept is known only on the device."""

    def __init__(self, capacity: int, threshold: Optional[float], backbone: str, crop_res: int = 224, device=None):
        self.capacity, self.count = int(capacity), 0
        self.threshold = float("nan") if threshold is None else float(threshold)
        self.in_crop = joints_in_crop(backbone)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._h = C.c_void_p()
        check(_bind().poco_pseudo_create(self.capacity, self.threshold, int(self.in_crop), int(crop_res), C.byref(self._h)),
              "poco_pseudo_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_pseudo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _f32(self, t, what: str, tail) -> torch.Tensor:
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(self.device)
        if not t.is_cuda:
            raise PocoHipError(f"PseudoLabeler.step: {what} must be a CUDA tensor")
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        if tuple(t.shape[1:]) != tuple(tail):
            raise PocoHipError(f"PseudoLabeler.step: {what} must be [B, {', '.join(map(str, tail))}], got {tuple(t.shape)}")
        return t

    def step(self, pred: Dict[str, torch.Tensor], boxes, source_id) -> None:
        """pred = the model's output dict as it is (pred_pose [B,24,3,3], pred_shape [B,10], var_pose [B,24] or [B,24,T],
        smpl_joints2d [B,49,2], smpl_joints3d [B,49,3]); boxes [B,4] = cx, cy, w, h of the crops; source_id int32 [B], handed back
        by finish() for the kept crops.  Enqueued on the current stream: no synchronisation, nothing copied to the host."""
        pp = self._f32(pred["pred_pose"], "pred_pose", (24, 3, 3))
        B = int(pp.shape[0])
        ps = self._f32(pred["pred_shape"], "pred_shape", (10,))
        var = pred["var_pose"]
        if not (torch.is_tensor(var) and var.is_cuda and var.dim() in (2, 3) and var.shape[1] == 24):
            raise PocoHipError("PseudoLabeler.step: var_pose must be a CUDA tensor [B,24] or [B,24,T]")
        var = self._f32(var, "var_pose", var.shape[1:])
        T = 1 if var.dim() == 2 else int(var.shape[2])
        j2 = self._f32(pred["smpl_joints2d"], "smpl_joints2d", (49, 2))
        j3 = self._f32(pred["smpl_joints3d"], "smpl_joints3d", (49, 3))
        bx = self._f32(boxes, "boxes", (4,))
        if torch.is_tensor(source_id):
            sid = source_id.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            sid = torch.from_numpy(np.ascontiguousarray(source_id, dtype=np.int32)).to(self.device)
        for t in (ps, var, j2, j3, bx, sid):
            if t.shape[0] != B:
                raise PocoHipError("PseudoLabeler.step: batch sizes differ")
        if sid.dim() != 1:
            raise PocoHipError("PseudoLabeler.step: source_id must be [B]")
        with torch.cuda.device(self.device):
            check(_bind().poco_pseudo_step(self._h, B, pp.data_ptr(), ps.data_ptr(), var.data_ptr(), T, j2.data_ptr(), j3.data_ptr(),
                                           bx.data_ptr(), sid.data_ptr(), self._stream()), "poco_pseudo_step")
        self.count += B

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            check(_bind().poco_pseudo_reset(self._h, self._stream()), "poco_pseudo_reset")
        self.count = 0

    def finish(self, imgname: Optional[Sequence[str]] = None, person_id: Optional[Sequence[int]] = None,
               return_records: bool = False) -> Dict[str, object]:
        """The kept crops as the arrays of the dataset file, in the order they were offered, plus `source_id` [N], `offered` and
        `kept`.  imgname / person_id: tables indexed by source_id (without them the file's `imgname` is str(source_id) and
        `person_id` 0).  return_records: also `records`, the record memory of every offered crop (rows past `kept` unwritten).
        Synchronises the current stream."""
        rec = np.empty((self.count, RECORD_FLOATS), np.float32)
        kept, offered = C.c_int64(0), C.c_int64(0)
        with torch.cuda.device(self.device):
            check(_bind().poco_pseudo_finish(self._h, rec.ctypes.data if self.count else None, rec.shape[0], C.byref(kept),
                                             C.byref(offered), self._stream()), "poco_pseudo_finish")
        out = split_records(rec[:kept.value])
        sid = out["source_id"]
        out["imgname"] = np.asarray([str(imgname[i]) if imgname is not None else str(i) for i in sid], dtype=np.str_).reshape(-1)
        out["person_id"] = np.asarray([person_id[i] if person_id is not None else 0 for i in sid], np.int32).reshape(-1)
        out["kept"], out["offered"] = int(kept.value), int(offered.value)
        if return_records:
            out["records"] = rec
        return out


def split_records(rec: np.ndarray) -> Dict[str, np.ndarray]:
    """Record block [N, RECORD_FLOATS] -> named arrays, every one with N as its leading dimension."""
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, RECORD_FLOATS)
    n = rec.shape[0]
    return {"source_id": rec[:, P_SRC].copy().view(np.int32), "center": rec[:, P_CENTER:P_CENTER + 2].copy(),
            "scale": rec[:, P_SCALE].copy(), "pose": rec[:, P_POSE:P_POSE + 72].copy(), "shape": rec[:, P_SHAPE:P_SHAPE + 10].copy(),
            "var": rec[:, P_VAR:P_VAR + 24].copy(), "has_smpl": np.ones(n, np.float32),
            "part": rec[:, P_PART:P_S].reshape(n, 24, 3).copy(), "openpose": rec[:, P_OPENPOSE:P_PART].reshape(n, 25, 3).copy(),
            "S": rec[:, P_S:P_PAD].reshape(n, 24, 4).copy()}


def write_dataset(path: str, arrays: Dict[str, object]) -> int:
    """The dataset .npz: DATASET_KEYS, EVERY array with N as its leading dimension - the reference's reader indexes every array of
    the file with the rows it selects (base_dataset.py:68-69), so a scalar in the file would break it.  Returns N."""
    missing = [k for k in DATASET_KEYS if k not in arrays]
    if missing:
        raise ValueError(f"write_dataset: missing {missing}")
    out = {k: np.asarray(arrays[k]) for k in DATASET_KEYS}
    n = out["imgname"].shape[0] if out["imgname"].ndim else -1
    for k, v in out.items():
        if v.ndim < 1 or v.shape[0] != n:
            raise ValueError(f"write_dataset: `{k}` has shape {v.shape}: every array needs the leading dimension N = {n}")
    out["imgname"] = out["imgname"].astype(np.str_)
    out["person_id"] = out["person_id"].astype(np.int32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    return int(n)
