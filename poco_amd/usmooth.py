"""Video mode's uncertainty-weighted smoother (demo.py --mode video --smooth_uncert LAMBDA): per track and per joint, a non-causal
penalised least-squares fit over time whose data term is weighted by the precision (u_ref / var)^2 and whose penalty is LAMBDA
times the squared second divided difference over the frame indices; every solved matrix is taken back onto SO(3).  Frames the
model is sure of stay put, doubtful ones are drawn towards what their neighbours say, and no threshold has to be tuned.  Shape and
the original-image camera are smoothed with the root joint's weights; every frame is re-posed with the LBS operator.  The contract
is stated in include/poco_hip.h (poco_op_track_smooth) and DESIGN.md section 28.

All tracks of a clip go up as ONE ragged buffer and through ONE call of the operator."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import ops


def smooth_tracks(model, tracks: Dict[str, dict], lam: float, u_ref: float = 0.3, max_gap: int = 30) -> Dict[str, dict]:
    """tracks: {id: dict(pose [T,24,3,3], betas [T,10], orig_cam [T,4], var [T,24], frame_ids [T], verts, smpl_joints3d)} - host
    arrays, what _finish_track returns; `model` a finalized poco_amd.model.POCO.
    -> {id: dict(pose, betas, orig_cam, verts, smpl_joints3d, smooth_shift float32 [T,24] = the angle in degrees every rotation was
    moved by)}.  The inputs are not modified."""
    ids = [pid for pid, tr in tracks.items() if len(tr["frame_ids"])]
    out = {pid: {**{k: np.asarray(tracks[pid][k]) for k in ("pose", "betas", "orig_cam", "verts", "smpl_joints3d")},
                 "smooth_shift": np.zeros((0, 24), np.float32)} for pid in tracks if pid not in ids}
    if not ids:
        return out
    dev = model.device
    f32 = lambda key, shape: np.ascontiguousarray(np.concatenate(                                           # noqa: E731
        [np.asarray(tracks[pid][key], np.float32).reshape((-1,) + shape) for pid in ids]))
    pose, var = f32("pose", (24, 3, 3)), f32("var", (24,))
    lin = np.concatenate([f32("betas", (10,)), f32("orig_cam", (4,))], 1)
    frames = np.concatenate([np.asarray(tracks[pid]["frame_ids"]).astype(np.int32).reshape(-1) for pid in ids])
    offsets = np.concatenate([[0], np.cumsum([len(tracks[pid]["frame_ids"]) for pid in ids])]).astype(np.int32)
    up = lambda a: torch.from_numpy(a).to(dev)                                                            # noqa: E731
    pose_d, lin_d, shift_d = ops.track_smooth(up(pose), up(var), up(frames), torch.from_numpy(offsets), up(lin), float(lam), float(u_ref),
                                              int(max_gap))
    betas_d = lin_d[:, :10].contiguous()
    verts, j3d = [], []
    bs = max(int(model.max_batch), 1)
    for lo in range(0, pose_d.shape[0], bs):           # every row moved: LBS of all of them
        v, j = model.smpl_lbs(betas_d[lo:lo + bs], pose_d[lo:lo + bs])
        verts.append(v.cpu().numpy())
        j3d.append(j.cpu().numpy())
    verts, j3d = np.concatenate(verts), np.concatenate(j3d)
    pose_h, lin_h, shift_h = pose_d.cpu().numpy(), lin_d.cpu().numpy(), shift_d.cpu().numpy()
    for k, pid in enumerate(ids):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        out[pid] = {"pose": pose_h[lo:hi], "betas": lin_h[lo:hi, :10], "orig_cam": lin_h[lo:hi, 10:14], "verts": verts[lo:hi],
                    "smpl_joints3d": j3d[lo:hi], "smooth_shift": shift_h[lo:hi]}
    return {pid: out[pid] for pid in tracks}


def summary_line(results: Dict[str, dict], tracks: Dict[str, dict]) -> str:
    """The one printed line: mean and largest shift in degrees and Pearson's r between the shift and the uncertainty over all
    finite (frame, joint) entries - the confident frames should be the ones that moved least."""
    shift = np.concatenate([np.asarray(r["smooth_shift"], np.float64).reshape(-1) for r in results.values()] or [np.zeros(0)])
    var = np.concatenate([np.asarray(tracks[pid]["var"], np.float64).reshape(-1) for pid in results] or [np.zeros(0)])
    if shift.size == 0:
        return "smooth_uncert: no frames"
    ok = np.isfinite(shift) & np.isfinite(var)
    r = float("nan")
    if ok.sum() > 1 and shift[ok].std() > 0 and var[ok].std() > 0:
        r = float(np.corrcoef(shift[ok], var[ok])[0, 1])
    return (f"smooth_uncert: mean shift {shift.mean():.3f} deg, max {shift.max():.3f} deg, Pearson r(shift, var) {r:+.3f} over "
            f"{shift.size} joint-frames in {len(results)} tracks")
