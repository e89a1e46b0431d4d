"""The keypoint refit (demo.py --mode video --kp_refit LAMBDA, eval.py --kp_refit LAMBDA): the joints the model doubts are refitted to
the 2-D keypoints the track (or the dataset row) carries, the network's own pose being the prior and each joint held by its own
precision LAMBDA (u_ref / var)^2 - --smooth_uncert's weighting rule applied in space instead of time.  Joints the model is sure of
stay where they are; a hidden forearm or a truncated leg is free to follow the detector.  Shape is not optimised; the camera is
(scale, tx, ty of the weak-perspective camera the renderer draws with).  The contract is stated in include/poco_hip.h
(poco_op_kp_refit) and DESIGN.md section 31.

All rows of a clip go up as ONE buffer and through ONE call of the operator; every fitted row is re-posed with the LBS operator."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

# BODY_25: Nose Neck RShoulder RElbow RWrist LShoulder LElbow LWrist MidHip RHip RKnee RAnkle LHip LKnee LAnkle, then eyes, ears and
# feet.  The 14 body keypoints are posed kinematic joints of SMPL in the reference's joint set (constants.JOINT_MAP); the face and
# the feet come from vertices and are not observed here.
BODY25_TO_SMPL = np.array([-1, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7] + [-1] * 10, np.int32)
DEFAULT_REF, DEFAULT_RHO, DEFAULT_ITERS, CAM_PRIOR, MIN_KP = 0.3, 0.1, 10, 1.0, 4


def joint_tables(smpl_file) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(Jt float64 [24,3], Jd float64 [24,3,10], parents int32 [24]) of a body-model .npz (or its dict): the rest-pose joints of
    shape beta are J(beta) = J_regressor (v_template + shapedirs beta) = Jt + Jd beta."""
    z = np.load(smpl_file) if isinstance(smpl_file, (str, bytes)) or hasattr(smpl_file, "__fspath__") else smpl_file
    Jr = np.asarray(z["J_regressor"], np.float64)
    vt = np.asarray(z["v_template"], np.float64)
    sd = np.asarray(z["shapedirs"], np.float64)[:, :, :10]
    parents = np.asarray(z["parents"]).astype(np.int64).astype(np.int32).reshape(-1)[:24].copy()
    parents[0] = -1
    return Jr @ vt, np.einsum("jv,vck->jck", Jr, sd), parents


def rest_joints(tables, betas: torch.Tensor) -> torch.Tensor:
    """J(beta) [N,24,3] fp32 on the device of `betas` [N,10]: one matmul."""
    Jt, Jd, _ = tables
    M = torch.from_numpy(np.concatenate([Jd.reshape(72, 10), Jt.reshape(72, 1)], 1).astype(np.float32)).to(betas.device)
    b1 = torch.cat([betas.float(), torch.ones((betas.shape[0], 1), device=betas.device)], 1)
    return (b1 @ M.T).reshape(-1, 24, 3).contiguous()


def refit_rows(tables, pose, var, betas, kp, cam, norm, lam, u_ref=DEFAULT_REF, rho=DEFAULT_RHO, conf_thresh=0.3, iters=DEFAULT_ITERS,
               cam_prior=CAM_PRIOR, min_kp=MIN_KP, kp_joint=BODY25_TO_SMPL) -> dict:
    """Device tensors pose [N,24,3,3], var [N,24], betas [N,10], kp [N,K,3], cam [N,5], norm [N] -> ops.kp_refit's dict."""
    return ops.kp_refit(pose, var, rest_joints(tables, betas), kp, cam, norm, kp_joint, tables[2], float(lam), float(u_ref), float(rho),
                        float(cam_prior), float(conf_thresh), int(min_kp), int(iters))


def refit_tracks(model, tracks: Dict[str, dict], lam: float, u_ref: float = DEFAULT_REF, rho: float = DEFAULT_RHO, conf_thresh: float = 0.3,
                 iters: int = DEFAULT_ITERS, *, tables, img_w: int, img_h: int, cam_prior: float = CAM_PRIOR,
                 min_kp: int = MIN_KP) -> Dict[str, dict]:
    """tracks: {id: dict(pose [T,24,3,3], betas [T,10], orig_cam [T,4], var [T,24], joints2d [T,25,3], bboxes [T,4], verts,
    smpl_joints3d)} - host arrays, what _finish_track returns; `model` a finalized poco_amd.model.POCO; tables = joint_tables(...).
    The camera of a row is the one the renderer draws with: a = sx W / 2, (px, py) = (W / 2, H / 2); the norm is bboxes[:, 2], the
    side of the square the demo's crop cuts and the h of convert_crop_cam_to_orig_img (a box that is not square is cropped by it too).
    -> {id: dict(pose, orig_cam, verts, smpl_joints3d, refit_shift float32 [T,24] (degrees), refit_cost float32 [T,2] (F before and
    after), refit_flag int32 [T] (0 fitted, 1 too few keypoints, 2 non-finite input))}.  A row that is not fitted keeps its pose,
    camera and mesh bit for bit.  The inputs are not modified."""
    ids = [pid for pid, tr in tracks.items() if len(tr["frame_ids"])]
    out = {pid: {**{k: np.asarray(tracks[pid][k]) for k in ("pose", "orig_cam", "verts", "smpl_joints3d")},
                 "refit_shift": np.zeros((0, 24), np.float32), "refit_cost": np.zeros((0, 2), np.float32),
                 "refit_flag": np.zeros((0,), np.int32)} for pid in tracks if pid not in ids}
    if not ids:
        return out
    dev = model.device
    f32 = lambda key, shape: np.ascontiguousarray(np.concatenate(                                           # noqa: E731
        [np.asarray(tracks[pid][key], np.float32).reshape((-1,) + shape) for pid in ids]))
    pose, var, betas, oc = f32("pose", (24, 3, 3)), f32("var", (24,)), f32("betas", (10,)), f32("orig_cam", (4,))
    kp, box = f32("joints2d", (25, 3)), f32("bboxes", (4,))
    W, H = float(img_w), float(img_h)
    cam = np.stack([oc[:, 0] * np.float32(W / 2), oc[:, 2], oc[:, 3], np.full(len(oc), W / 2, np.float32), np.full(len(oc), H / 2, np.float32)],
                   1).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(tracks[pid]["frame_ids"]) for pid in ids])])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                                      # noqa: E731
    pose_d, betas_d = up(pose), up(betas)
    res = refit_rows(tables, pose_d, up(var), betas_d, up(kp), up(cam), up(box[:, 2]), lam, u_ref, rho, conf_thresh, iters, cam_prior, min_kp)
    info = res["info"].cpu().numpy()
    fitted = np.nonzero(info[:, 1] == 0)[0]
    verts = np.ascontiguousarray(np.concatenate([np.asarray(tracks[pid]["verts"], np.float32) for pid in ids]))
    j3d = np.ascontiguousarray(np.concatenate([np.asarray(tracks[pid]["smpl_joints3d"], np.float32) for pid in ids]))
    bs = max(int(model.max_batch), 1)
    rows_d = torch.from_numpy(fitted).to(dev)
    for lo in range(0, len(fitted), bs):               # LBS of every fitted row
        sel = rows_d[lo:lo + bs]
        v, j = model.smpl_lbs(betas_d[sel].contiguous(), res["pose"][sel].contiguous())
        verts[fitted[lo:lo + bs]] = v.cpu().numpy()
        j3d[fitted[lo:lo + bs]] = j.cpu().numpy()
    pose_h, cam_h = res["pose"].cpu().numpy(), res["cam"].cpu().numpy()
    shift_h, cost_h = res["shift"].cpu().numpy(), res["cost"].cpu().numpy()
    oc_new = oc.copy()
    f = fitted
    oc_new[f] = np.stack([cam_h[f, 0] * np.float32(2 / W), cam_h[f, 0] * np.float32(2 / H), cam_h[f, 1], cam_h[f, 2]], 1)
    for k, pid in enumerate(ids):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        out[pid] = {"pose": pose_h[lo:hi], "orig_cam": oc_new[lo:hi], "verts": verts[lo:hi], "smpl_joints3d": j3d[lo:hi],
                    "refit_shift": shift_h[lo:hi], "refit_cost": cost_h[lo:hi], "refit_flag": info[lo:hi, 1].copy()}
    return {pid: out[pid] for pid in tracks}


def reprojection_error(tables, pose, betas, kp, cam3, cam5, norm, conf_thresh=0.3, kp_joint=BODY25_TO_SMPL) -> np.ndarray:
    """Host: per row the mean over the observed keypoints of |proj(p_k) - kp_k| / norm (NaN where none is observed), in float64."""
    Jt, Jd, parents = tables
    pose, betas, kp = np.asarray(pose, np.float64), np.asarray(betas, np.float64), np.asarray(kp, np.float64)
    N = len(pose)
    J = Jt[None] + np.einsum("jck,nk->njc", Jd, betas)
    G, p = np.empty((N, 24, 3, 3)), np.empty((N, 24, 3))
    G[:, 0], p[:, 0] = pose[:, 0], J[:, 0]
    for j in range(1, 24):
        a = int(parents[j])
        G[:, j] = G[:, a] @ pose[:, j]
        p[:, j] = p[:, a] + np.einsum("nrc,nc->nr", G[:, a], J[:, j] - J[:, a])
    ks = np.nonzero(np.asarray(kp_joint) >= 0)[0]
    pk = p[:, np.asarray(kp_joint)[ks]]
    cam3, cam5, norm = np.asarray(cam3, np.float64), np.asarray(cam5, np.float64), np.asarray(norm, np.float64)
    u = cam3[:, None, 0] * (pk[:, :, 0] + cam3[:, None, 1]) + cam5[:, None, 3]
    v = cam3[:, None, 0] * (pk[:, :, 1] + cam3[:, None, 2]) + cam5[:, None, 4]
    e = np.hypot(u - kp[:, ks, 0], v - kp[:, ks, 1]) / norm[:, None]
    seen = kp[:, ks, 2] > conf_thresh
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(seen.any(1), (e * seen).sum(1) / seen.sum(1), np.nan)


def _pearson(x, y) -> float:
    ok = np.isfinite(x) & np.isfinite(y)
    if ok.sum() > 1 and x[ok].std() > 0 and y[ok].std() > 0:
        return float(np.corrcoef(x[ok], y[ok])[0, 1])
    return float("nan")


def summary_line(results: Dict[str, dict], tracks: Dict[str, dict], tables=None, img_w: Optional[int] = None, img_h: Optional[int] = None,
                 conf_thresh: float = 0.3) -> str:
    """The one printed line: the mean reprojection error in box fractions before and after (over the fitted rows; with `tables` and
    the image size), the mean and largest shift in degrees and Pearson's r between the shift and the uncertainty over all finite
    (frame, joint) entries - the doubtful joints should be the ones that moved."""
    cat = lambda d, k, w: np.concatenate([np.asarray(d[pid][k], np.float64).reshape((-1,) + w) for pid in results] or      # noqa: E731
                                         [np.zeros((0,) + w)])
    shift, var, flag = cat(results, "refit_shift", (24,)), cat(tracks, "var", (24,)), cat(results, "refit_flag", ())
    if shift.size == 0:
        return "kp_refit: no frames"
    reproj = ""
    fit = flag == 0
    if tables is not None and fit.any():
        W, H = float(img_w), float(img_h)
        cam5 = lambda oc: np.stack([oc[:, 0] * W / 2, oc[:, 2], oc[:, 3], np.full(len(oc), W / 2), np.full(len(oc), H / 2)], 1)   # noqa: E731
        kp, betas, norm = cat(tracks, "joints2d", (25, 3)), cat(tracks, "betas", (10,)), cat(tracks, "bboxes", (4,))[:, 2]
        c0, c1 = cam5(cat(tracks, "orig_cam", (4,))), cam5(cat(results, "orig_cam", (4,)))
        e0 = reprojection_error(tables, cat(tracks, "pose", (24, 3, 3))[fit], betas[fit], kp[fit], c0[fit, :3], c0[fit], norm[fit], conf_thresh)
        e1 = reprojection_error(tables, cat(results, "pose", (24, 3, 3))[fit], betas[fit], kp[fit], c1[fit, :3], c1[fit], norm[fit], conf_thresh)
        reproj = f"reprojection error {np.nanmean(e0):.4f} -> {np.nanmean(e1):.4f} of the box, "
    return (f"kp_refit: {reproj}mean shift {shift[fit].mean() if fit.any() else 0.0:.3f} deg, max {shift.max():.3f} deg, Pearson r(shift, var) "
            f"{_pearson(shift[fit].reshape(-1), var[fit].reshape(-1)):+.3f} over {int(fit.sum())} fitted of {len(flag)} frames in "
            f"{len(results)} tracks")


def tracking_error(tracking) -> Optional[str]:
    """The one sentence that refuses --kp_refit on tracks it cannot fit, or None: every track needs BODY_25 keypoints."""
    if not isinstance(tracking, dict) or not tracking:
        return ("--kp_refit fits the tracks to their 2-D keypoints: it needs a --tracking file whose tracks carry joints2d "
                "(--tracking_method pose)")
    for pid, tr in tracking.items():
        j = tr.get("joints2d")
        if j is None:
            return f"--kp_refit fits a track to its 2-D keypoints: track {pid!r} has no joints2d (--tracking_method pose reads them)"
        K = np.asarray(j).shape[1] if np.asarray(j).ndim == 3 else -1
        if K != 25:
            return f"--kp_refit maps BODY_25 keypoints only: track {pid!r} has joints2d with {K} keypoints, not 25"
    return None


def flag_error(args, prog: str):
    """The one sentence that refuses --kp_refit and its companions where they cannot work, or None; prog = "eval" | "demo"."""
    lam = getattr(args, "kp_refit", None)
    ref, rho, iters = getattr(args, "kp_refit_ref", DEFAULT_REF), getattr(args, "kp_refit_rho", DEFAULT_RHO), getattr(args, "kp_refit_iters", DEFAULT_ITERS)
    if lam is None:
        if ref != DEFAULT_REF or rho != DEFAULT_RHO or iters != DEFAULT_ITERS:
            return "--kp_refit_ref, --kp_refit_rho and --kp_refit_iters tune --kp_refit: they need --kp_refit LAMBDA"
        return None
    if not (lam > 0.0 and lam < float("inf")):
        return f"--kp_refit LAMBDA must be finite and > 0, got {lam}"
    if not (ref > 0.0 and ref < float("inf")):
        return f"--kp_refit_ref must be finite and > 0, got {ref}"
    if not abs(rho) < float("inf"):
        return f"--kp_refit_rho must be finite (<= 0 turns the robustifier off), got {rho}"
    if not 1 <= iters <= ops.REFIT_MAX_ITERS:
        return f"--kp_refit_iters must be in 1..{ops.REFIT_MAX_ITERS}, got {iters}"
    if getattr(args, "cfg2", None) or getattr(args, "ckpt2", None):
        return "--kp_refit with a second model (--cfg2 / --ckpt2) is not supported: refit one model's prediction"
    if prog == "eval":
        for flag, on in (("--tta", getattr(args, "tta", None) is not None), ("--segm", bool(getattr(args, "segm", False))),
                         ("--likelihood", bool(getattr(args, "likelihood", False))), ("--sequences", bool(getattr(args, "sequences", False))),
                         ("--rank_metrics", bool(getattr(args, "rank_metrics", False))), ("--visibility", bool(getattr(args, "visibility", False))),
                         ("--aug_rot", getattr(args, "aug_rot", None) is not None), ("--aug_scale", getattr(args, "aug_scale", None) is not None),
                         ("--aug_flip", bool(getattr(args, "aug_flip", False))), ("--aug_noise", getattr(args, "aug_noise", None) is not None),
                         ("--aug_occlude", getattr(args, "aug_occlude", None) is not None), ("--augment", bool(getattr(args, "augment", False)))):
            if on:
                return f"--kp_refit scores one plain forward beside its refit: it cannot be combined with {flag}"
        return None
    if getattr(args, "mode", "folder") != "video":
        return f"--kp_refit fits the keypoint tracks of video mode: --mode {getattr(args, 'mode', 'folder')} is not supported"
    if getattr(args, "gpus", 1) > 1:
        return "--kp_refit with --gpus N > 1 is not supported: the packed record the ranks exchange has no room for the refit's outputs; run with --gpus 1"
    return None
