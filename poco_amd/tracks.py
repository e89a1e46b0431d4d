"""Keypoint tracks -> person boxes: the input of `--tracking_method pose` (reference tester.py:371-392 hands a track's
`joints2d` to dataset/inference.py:58-67, which derives the boxes with pocolib/utils/smooth_bbox.py).  A 2-D pose tracker
(STAF / OpenPose in the reference) writes, per person, `joints2d` [T,K,3] (x, y in original-image pixels, confidence) and
`frames` [T]; a frame the person was not seen in is None or has no confident joint.

Host numpy, once per track before the first frame is decoded: a few hundred scalars, nothing for the device.
The arithmetic keeps the reference's operand types and order (per-parameter np.linspace, parameters in the keypoints' own
float type), so that float64 keypoints give the reference's float64 parameters and float32 ones its float32 parameters."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

MIN_DIAGONAL = 0.5          # smooth_bbox.py:55: a person whose visible joints span less than half a pixel is no prediction
PERSON_SIZE = 150.0         # smooth_bbox.py:58: scale = 150 / diagonal; inference.py:60: side = 150 / scale


def _entries(joints2d) -> list:
    """The per-frame entries of a track: [K,3] float arrays (their float type kept, anything else as float64) or None."""
    out = []
    for kp in joints2d:
        if kp is None:
            out.append(None)
            continue
        kp = np.asarray(kp)
        if kp.dtype not in (np.float32, np.float64):
            kp = kp.astype(np.float64)
        if kp.ndim != 2 or kp.shape[1] < 3:
            raise ValueError(f"a frame's keypoints must be [K,3] (x, y, confidence), got {kp.shape}")
        out.append(kp)
    return out


def _frame_param(kp: Optional[np.ndarray], vis_thresh: float) -> Optional[np.ndarray]:
    """(cx, cy, scale) of one frame (kp_to_bbox_param, smooth_bbox.py:36-59), or None where the frame has no prediction."""
    if kp is None:
        return None
    vis = kp[:, 2] > vis_thresh
    if not vis.any():
        return None
    lo, hi = kp[vis, :2].min(0), kp[vis, :2].max(0)
    diagonal = np.linalg.norm(hi - lo)
    if diagonal < MIN_DIAGONAL:
        return None
    return np.append((lo + hi) / 2.0, PERSON_SIZE / diagonal)


def bbox_params_from_keypoints(joints2d, vis_thresh: float = 0.3) -> Tuple[np.ndarray, int, int]:
    """joints2d: [T,K,3] array, list of [K,3] arrays, or list with None entries -> (params [T',3] (cx, cy, scale), start, end)
    with T' = end - start (get_all_bbox_params, smooth_bbox.py:62-103): frames before the first and after the last prediction
    are trimmed, runs without a prediction in between are filled by np.linspace between their neighbours, per parameter.  A track
    without any prediction gives (empty [0,3], 0, 0)."""
    rows, dtype = [], np.dtype(np.float32)
    start, gap, end = -1, 0, 0
    for i, kp in enumerate(_entries(joints2d)):
        p = _frame_param(kp, vis_thresh)
        if p is None:
            gap += 1
            continue
        dtype = np.result_type(dtype, p.dtype)             # what stacking onto the reference's float32 [0,3] array leaves
        if start < 0:
            start = i
        elif gap:
            prev = rows[-1].astype(dtype, copy=False)
            filled = np.array([np.linspace(a, b, gap + 2) for a, b in zip(prev, p)])          # [3, gap + 2]
            dtype = np.result_type(dtype, filled.dtype)
            rows.extend(filled.T[1:-1])
        gap = 0
        rows.append(p)
        end = i + 1
    if not rows:
        return np.empty((0, 3), np.float32), 0, 0
    return np.stack([np.asarray(r, dtype) for r in rows]), start, end


def smooth_bbox_params(params: np.ndarray, kernel_size: int = 11, sigma: float = 8.0) -> np.ndarray:
    """smooth_bbox.py:106-121: per parameter a median filter (scipy.signal.medfilt: zero padded) and then a Gaussian
    (scipy.ndimage.gaussian_filter1d: reflect boundary, truncated at 4 sigma)."""
    from scipy import signal
    from scipy.ndimage import gaussian_filter1d
    med = np.array([signal.medfilt(p, kernel_size) for p in params.T]).T
    return np.array([gaussian_filter1d(p, sigma) for p in med.T]).T


def boxes_from_keypoints(joints2d, frames: Sequence[int], vis_thresh: float = 0.3, smooth: bool = False, kernel_size: int = 11,
                         sigma: float = 8.0) -> dict:
    """One keypoint track as the box track run_on_video reads: {'bbox': [T',4] float32 (cx, cy, side, side) with side =
    150 / scale (inference.py:59-61), 'frames': [T'], 'joints2d': [T',K,3]}, frames and keypoints cut to [start:end]
    (inference.py:63-67); a None entry inside the kept range becomes a row of zeros (confidence 0).  smooth: the parameters go
    through smooth_bbox_params first (the reference's Inference never does)."""
    frames = np.asarray(frames, np.int64).reshape(-1)
    entries = _entries(joints2d)
    if len(entries) != frames.shape[0]:
        raise ValueError(f"{len(entries)} keypoint entries for {frames.shape[0]} frames")
    params, start, end = bbox_params_from_keypoints(entries, vis_thresh)
    if not len(params):
        K = next((e.shape[0] for e in entries if e is not None), 0)
        return {"bbox": np.empty((0, 4), np.float32), "frames": frames[:0], "joints2d": np.empty((0, K, 3), np.float32)}
    if smooth:
        params = smooth_bbox_params(params, kernel_size, sigma)
    side = PERSON_SIZE / params[:, 2]
    kept = entries[start:end]
    shape = next(e.shape for e in kept if e is not None)
    kdt = np.result_type(*[e.dtype for e in kept if e is not None])
    return {"bbox": np.stack([params[:, 0], params[:, 1], side, side], 1).astype(np.float32), "frames": frames[start:end],
            "joints2d": np.stack([np.zeros(shape, kdt) if e is None else e.astype(kdt, copy=False) for e in kept])}
