"""Video mode's in-fill (demo.py --mode video --infill THRESH): per track and per joint, the rotations the model does not trust
(post-processed uncertainty above THRESH) are replaced by the shortest-arc interpolation between the nearest confident frames on
either side; shape and the original-image camera follow the root joint; the meshes of the touched frames are re-posed with the
LBS operator.  The contract is stated in include/poco_hip.h (poco_op_track_infill) and DESIGN.md section 24.

All tracks of a clip go up as ONE ragged buffer and through ONE call of the operator; only the touched rows go through LBS."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import ops

FLAG_NAMES = ("reliable", "interpolated", "held", "left")          # flags 0..3 of poco_op_track_infill


def infill_tracks(model, tracks: Dict[str, dict], thresh: float, max_gap: int) -> Dict[str, dict]:
    """tracks: {id: dict(pose [T,24,3,3], betas [T,10], orig_cam [T,4], var [T,24], frame_ids [T], verts [T,V,3],
    smpl_joints3d [T,49,3])} - host arrays, what _finish_track works on; `model` a finalized poco_amd.model.POCO.
    -> {id: dict(pose, betas, orig_cam, verts, smpl_joints3d, infill uint8 [T,24] = the flags, counts = dict(interpolated, held,
    left, touched_frames))}.  Rows the in-fill does not touch keep their input bits; the inputs are not modified."""
    ids = [pid for pid, tr in tracks.items() if len(tr["frame_ids"])]
    out = {pid: {**{k: np.asarray(tracks[pid][k]) for k in ("pose", "betas", "orig_cam", "verts", "smpl_joints3d")},
                 "infill": np.zeros((0, 24), np.uint8), "counts": {"interpolated": 0, "held": 0, "left": 0, "touched_frames": 0}}
           for pid in tracks if pid not in ids}
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
    pose_d, lin_d, flags_d, _, rows_d, count_d = ops.track_infill(up(pose), up(var), up(frames), torch.from_numpy(offsets), up(lin),
                                                                  float(thresh), int(max_gap), rows=True)
    n = int(count_d.item())
    rows_d = rows_d[:n].long()
    pose_h, lin_h, flags_h, rows_h = pose_d.cpu().numpy(), lin_d.cpu().numpy(), flags_d.cpu().numpy(), rows_d.cpu().numpy()
    verts_rows, j3d_rows = [], []
    bs = max(int(model.max_batch), 1)
    for lo in range(0, n, bs):                         # LBS of the touched rows only
        sel = rows_d[lo:lo + bs]
        v, j = model.smpl_lbs(lin_d.index_select(0, sel)[:, :10].contiguous(), pose_d.index_select(0, sel))
        verts_rows.append(v.cpu().numpy())
        j3d_rows.append(j.cpu().numpy())
    verts_rows = np.concatenate(verts_rows) if verts_rows else None
    j3d_rows = np.concatenate(j3d_rows) if j3d_rows else None
    for k, pid in enumerate(ids):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        tr = tracks[pid]
        verts, j3d = np.array(tr["verts"], np.float32), np.array(tr["smpl_joints3d"], np.float32)          # copies
        a, b = np.searchsorted(rows_h, lo), np.searchsorted(rows_h, hi)
        if b > a:
            verts[rows_h[a:b] - lo] = verts_rows[a:b]
            j3d[rows_h[a:b] - lo] = j3d_rows[a:b]
        fl = flags_h[lo:hi]
        out[pid] = {"pose": pose_h[lo:hi], "betas": lin_h[lo:hi, :10], "orig_cam": lin_h[lo:hi, 10:14], "verts": verts,
                    "smpl_joints3d": j3d, "infill": fl,
                    "counts": {"interpolated": int((fl == 1).sum()), "held": int((fl == 2).sum()), "left": int((fl == 3).sum()),
                               "touched_frames": int(b - a)}}
    return {pid: out[pid] for pid in tracks}


def summary_line(results: Dict[str, dict]) -> str:
    """The one printed line: in-filled joint-frames by flag, touched frames, tracks."""
    tot = {k: sum(r["counts"][k] for r in results.values()) for k in ("interpolated", "held", "left", "touched_frames")}
    return (f"infill: {tot['interpolated']} joint-frames interpolated, {tot['held']} held, {tot['left']} left as regressed; "
            f"{tot['touched_frames']} frames re-posed in {len(results)} tracks")
