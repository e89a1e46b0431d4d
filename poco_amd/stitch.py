"""Video mode's --track_stitch: the fragments an occlusion left of one person joined into chains, after the forward (DESIGN.md
section 36).

A box tracker forgets a person it has not seen for a few frames, and whoever comes out from behind the pillar is a new id.
--infill, --smooth_uncert and --kp_refit repair uncertain frames from confident ones of the SAME track: they cannot reach across
such a break.  After the forward we hold what no box tracker has: the regressor's body shape of every fragment, which belongs to
the person and not to the frame, and the model's own uncertainty, which says which frames to trust for it.  ops.track_stitch
(csrc/track_stitch.hip) decides from shape and extrapolated box motion which fragment continues which, as one optimal assignment
per clip, on the device.  What stays on the host is bookkeeping: packing the fragments into one buffer, and concatenating the rows
of a chain.

The tolerances' defaults (motion_tol, shape_tol, shape_floor) are guesses: nobody has measured them on real video."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ops

MIN_NUM_FRAMES = 25               # the reference's rule for a track (tester.py:133-136), applied here to the chains
PARAMS = ("max_gap", "fit_len", "u_ref", "motion_tol", "shape_tol", "shape_floor", "shape_w")


def _pid_key(pid):
    s = str(pid)
    return (0, int(s), "") if s.lstrip("-").isdigit() else (1, 0, s)


def pack_fragments(tracking_results: dict, stacked: dict) -> dict:
    """The fragments, sorted by person id (numbers by value, then names), as the operator's buffers: dict(pids, frag_offsets int32
    [P+1], frames int32 [N], boxes float64 [N,4], betas float32 [N,10], var float32 [N,24])."""
    pids = sorted(tracking_results, key=_pid_key)
    fo = [0]
    for pid in pids:
        n = len(tracking_results[pid]["frames"])
        if len(stacked[pid]["pred_shape"]) != n or len(stacked[pid]["var_pose"]) != n:
            raise ValueError(f"track {pid!r}: {n} frames but {len(stacked[pid]['pred_shape'])} regressed rows")
        fo.append(fo[-1] + n)
    cat = lambda parts, dt, w: (np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros((0,) + w, dt))   # noqa: E731
    return {"pids": pids, "frag_offsets": np.asarray(fo, np.int32),
            "frames": cat([np.asarray(tracking_results[p]["frames"]).reshape(-1) for p in pids], np.int32, ()),
            "boxes": np.ascontiguousarray(cat([np.asarray(tracking_results[p]["bbox"], np.float64).reshape(-1, 4) for p in pids], np.float64, (4,))),
            "betas": np.ascontiguousarray(cat([np.asarray(stacked[p]["pred_shape"], np.float32).reshape(-1, 10) for p in pids], np.float32, (10,))),
            "var": np.ascontiguousarray(cat([np.asarray(stacked[p]["var_pose"], np.float32).reshape(-1, 24) for p in pids], np.float32, (24,)))}


def interpolate_boxes(last: np.ndarray, first: np.ndarray, e: int, s: int, dtype) -> np.ndarray:
    """The D - 1 = s - e - 1 boxes of the frames between a fragment's last row (frame e) and its successor's first (frame s): the
    float64 linear interpolation of (cx, cy, w, h), cast to the tracks' dtype."""
    D = int(s) - int(e)
    a, b = np.asarray(last, np.float64), np.asarray(first, np.float64)
    rows = [a + (b - a) * (float(k) / float(D)) for k in range(1, D)]
    return np.asarray(rows, np.float64).reshape(-1, 4).astype(dtype)


def stitch_tracks(tracking_results: dict, stacked: dict, frames_total: Optional[int] = None, *, fill: bool = True, device="cuda",
                  **params):
    """(merged tracking_results, merged stacked, chains) of one clip.  tracking_results: {pid: {'bbox': [T,4], 'frames': [T]}};
    stacked: run_on_video's raw rows per track ({pid: {key: [T, ...]}}, among them pred_shape [T,10] and var_pose [T,24]);
    frames_total: the number of frames of the clip (a frame index outside it is a ValueError) or None; params: the operator's
    (ops.STITCH_DEFAULTS).  The operator is called once.

    A chain takes the person id of its first fragment.  merged tracking_results[pid] holds the chain's rows in frame order - with
    fill, the rows of the holes between joined fragments among them, their boxes interpolated (interpolate_boxes) - and
    merged stacked[pid] the chain's OWN regressed rows in that order (gap_tracks names the rows that still have to go through the
    forward, merge_gap_rows splices them in).  chains: per chain, in the order of the merged dicts, dict(pid, fragments = the
    joined person ids in order, gains = the gain of each link, stitch uint8 [T] (0 an own row, 1 a gap row), stitch_frag int32 [T]
    (the index of the source fragment in the chain, -1 on a gap row))."""
    import torch
    unknown = set(params) - set(PARAMS)
    if unknown:
        raise TypeError(f"stitch_tracks: unknown parameter {sorted(unknown)[0]!r}")
    buf = pack_fragments(tracking_results, stacked)
    pids, fo = buf["pids"], buf["frag_offsets"]
    if frames_total is not None and len(buf["frames"]) and (buf["frames"].min() < 0 or buf["frames"].max() >= frames_total):
        raise ValueError(f"stitch_tracks: a frame index lies outside the clip's {frames_total} frames")
    res = ops.track_stitch(None, fo, *(torch.from_numpy(buf[k]).to(device) for k in ("frames", "boxes", "betas", "var")),
                           **{**ops.STITCH_DEFAULTS, **params})
    status = int(res["status"].cpu().numpy()[0])
    if status != 0:
        raise ValueError(f"stitch_tracks: the operator could not read the fragment tables (status {status})")
    succ, pred, gain = (res[k].cpu().numpy() for k in ("succ", "pred", "gain"))
    merged_tr, merged_st, chains = {}, {}, []
    for first in range(len(pids)):
        if pred[first] >= 0:
            continue
        members, g = [], first
        while g >= 0 and len(members) <= len(pids):
            members.append(g)
            g = int(succ[g])
        dtype = np.asarray(tracking_results[pids[first]]["bbox"]).dtype
        boxes, frames, flag, src = [], [], [], []
        for k, m in enumerate(members):
            tr = tracking_results[pids[m]]
            bb, fr = np.asarray(tr["bbox"]).reshape(-1, 4), np.asarray(tr["frames"], np.int64).reshape(-1)
            if k and fill:
                e, s = int(frames[-1][-1]), int(fr[0])
                boxes.append(interpolate_boxes(boxes[-1][-1], bb[0], e, s, dtype))
                frames.append(np.arange(e + 1, s, dtype=np.int64))
                flag.append(np.ones(s - e - 1, np.uint8))
                src.append(np.full(s - e - 1, -1, np.int32))
            boxes.append(bb.astype(dtype, copy=False))
            frames.append(fr)
            flag.append(np.zeros(len(fr), np.uint8))
            src.append(np.full(len(fr), k, np.int32))
        pid = pids[first]
        merged_tr[pid] = {"bbox": np.concatenate(boxes), "frames": np.concatenate(frames)}
        merged_st[pid] = {key: np.concatenate([np.asarray(stacked[pids[m]][key]) for m in members]) for key in stacked[pid]}
        chains.append({"pid": pid, "fragments": [pids[m] for m in members], "gains": [float(gain[m]) for m in members[:-1]],
                       "stitch": np.concatenate(flag), "stitch_frag": np.concatenate(src)})
    return merged_tr, merged_st, chains


def gap_tracks(merged_tracks: dict, chains) -> dict:
    """The gap rows as a tracking dict of their own ({pid: {'bbox', 'frames'}}, chains without a hole left out): what the forward
    still has to see."""
    out = {}
    for ch in chains:
        gap = ch["stitch"] == 1
        if gap.any():
            tr = merged_tracks[ch["pid"]]
            out[ch["pid"]] = {"bbox": tr["bbox"][gap], "frames": tr["frames"][gap]}
    return out


def merge_gap_rows(merged_stacked: dict, gap_stacked: dict, chains) -> dict:
    """merged stacked with the forward's rows for the gap frames (gap_stacked: run_on_video(gap_tracks(...), raw=True)) spliced in,
    in frame order: every array of a chain gets one row per row of its merged track."""
    out = {}
    for ch in chains:
        pid, gap = ch["pid"], ch["stitch"] == 1
        if not gap.any():
            out[pid] = merged_stacked[pid]
            continue
        out[pid] = {}
        for key, own in merged_stacked[pid].items():
            rows = np.asarray(gap_stacked[pid][key])
            if len(rows) != int(gap.sum()) or len(own) != int((~gap).sum()):
                raise ValueError(f"merge_gap_rows: chain {pid!r}, {key}: {len(own)} own and {len(rows)} gap rows for {len(gap)} frames")
            full = np.empty((len(gap),) + own.shape[1:], own.dtype)
            full[~gap], full[gap] = own, rows
            out[pid][key] = full
    return out


def drop_short(merged_tracks: dict, merged_stacked: dict, chains, min_frames: int = MIN_NUM_FRAMES):
    """The 25-frame rule on the chains: (tracks, stacked, chains kept, number dropped)."""
    keep = [ch for ch in chains if len(ch["stitch"]) >= min_frames]
    return ({ch["pid"]: merged_tracks[ch["pid"]] for ch in keep}, {ch["pid"]: merged_stacked[ch["pid"]] for ch in keep}, keep,
            len(chains) - len(keep))


def summary_line(n_fragments: int, chains, dropped: int) -> str:
    links = sum(len(ch["fragments"]) - 1 for ch in chains)
    gaps = sum(int((ch["stitch"] == 1).sum()) for ch in chains)
    return f"track_stitch: {n_fragments} fragments, {links} links, {len(chains)} chains, {gaps} gap rows, {dropped} chains dropped"


def flag_error(args) -> Optional[str]:
    """demo.py's --track_stitch and --stitch_* flags: what cannot work, as one line, or None."""
    d = ops.STITCH_DEFAULTS
    given = [f for f, v in (("stitch_max_gap", d["max_gap"]), ("stitch_fit_len", d["fit_len"]), ("stitch_motion_tol", d["motion_tol"]),
                            ("stitch_shape_tol", d["shape_tol"]), ("stitch_shape", d["shape_w"]), ("stitch_min_frag", 5),
                            ("stitch_no_fill", False)) if getattr(args, f, v) != v]
    if not getattr(args, "track_stitch", False):
        return f"--{given[0]} tunes --track_stitch: it needs --track_stitch" if given else None
    if args.mode != "video":
        return "--track_stitch joins the tracks of video mode: it needs --mode video"
    if getattr(args, "kp_refit", None) is not None:
        return "--track_stitch with --kp_refit: the rows that fill a hole have no keypoints to refit to"
    if (getattr(args, "tracking_method", "bbox") or "bbox") == "pose":
        return "--track_stitch with --tracking_method pose: the rows that fill a hole have no keypoints"
    if getattr(args, "gpus", 1) > 1:
        return "--track_stitch with --gpus N > 1 is not supported: whole tracks are sharded across the ranks, a chain may span two; run with --gpus 1"
    if getattr(args, "save_dataset", None):
        return "--track_stitch with --save_dataset: the dataset is written from the tracks as they went into the forward, not from the chains"
    if args.stitch_max_gap < 0:
        return f"--stitch_max_gap must be >= 0, got {args.stitch_max_gap}"
    if not 1 <= args.stitch_fit_len <= 32:
        return f"--stitch_fit_len must be in 1..32, got {args.stitch_fit_len}"
    for f in ("stitch_motion_tol", "stitch_shape_tol"):
        v = getattr(args, f)
        if not (v > 0.0 and v < float("inf")):
            return f"--{f} must be finite and > 0, got {v}"
    if not (args.stitch_shape >= 0.0 and args.stitch_shape < float("inf")):
        return f"--stitch_shape must be finite and >= 0, got {args.stitch_shape}"
    if args.stitch_min_frag < 1:
        return f"--stitch_min_frag must be >= 1, got {args.stitch_min_frag}"
    return None


def tracking_error(tracking) -> Optional[str]:
    """--track_stitch on keypoint tracks: the rows that fill a hole would have no keypoints."""
    if isinstance(tracking, dict):
        for pid, tr in tracking.items():
            if tr.get("joints2d") is not None:
                return f"--track_stitch: track {pid!r} carries keypoints (joints2d); the rows that fill a hole have none"
    return None


def params_of(args) -> dict:
    """The operator's parameters from the demo's flags."""
    return {"max_gap": int(args.stitch_max_gap), "fit_len": int(args.stitch_fit_len), "motion_tol": float(args.stitch_motion_tol),
            "shape_tol": float(args.stitch_shape_tol), "shape_w": float(args.stitch_shape)}
