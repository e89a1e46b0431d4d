"""Video mode's --tracker sort: per-frame person boxes -> the tracks run_on_video reads.

The reference makes its tracks itself: POCOTester.run_tracking calls multi_person_tracker, a detector followed by SORT.  The detector
is out of scope (its weights and code are outside the reference tree); its OUTPUT is what --detections already reads in folder mode.
This module is the other half: the association, on the device (ops.sort_tracks, csrc/sort_tracks.hip).  What stays on the host is
bookkeeping on a few integers per detection: flattening the file into one buffer, and grouping the ids that came back."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np

from . import ops

MIN_NUM_FRAMES = 25               # the reference's tester.py:133-136, as tester.load_tracking applies it to the tracker's cache
IMG_EXT = (".jpg", ".jpeg", ".png", ".bmp")


def frame_names(vid_file: str) -> list:
    """The frame names of video mode's input in frame order: the sorted image files of a folder, or NNNNNN.jpg (from 000001, as the
    reference's ffmpeg extraction names them) for the frames of a Motion-JPEG .avi."""
    if os.path.isfile(vid_file):
        from .jpeg import MjpegReader
        with MjpegReader(vid_file) as reader:
            return [f"{i + 1:06d}.jpg" for i in range(len(reader))]
    return sorted(x for x in os.listdir(vid_file) if x.lower().endswith(IMG_EXT))


def detections_to_buffers(detections, names: Sequence[str]) -> dict:
    """Both accepted forms of --detections - {image name: [[cx, cy, w, h], ...]} or the reference's detection_results.pkl, a sequence
    indexed by the image's position in the sorted listing - for the frames `names`, in order -> dict(dets float64 [N,4],
    frame_offsets int32 [F+1], rows = per frame the user's own [n,4] rows (float32 / float64 kept, anything else as float32: folder
    mode's rule)).  A fifth column (the detector's score) is ignored; a frame that is not listed, None or empty holds no detection."""
    rows, offsets = [], [0]
    for pos, n in enumerate(names):
        if isinstance(detections, dict):
            d = detections.get(n)
        else:
            d = detections[pos] if detections is not None and pos < len(detections) else None
        if d is None or len(d) == 0:
            a = np.zeros((0, 4), np.float32)
        else:
            a = np.asarray(d)
            if a.ndim == 1:
                a = a.reshape(1, -1)
            if a.ndim != 2 or a.shape[1] not in (4, 5):
                raise ValueError(f"frame {pos} ({n}): detections must be [n,4] (cx, cy, w, h) or [n,5] with a score, got {a.shape}")
            a = a[:, :4]
            a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float32)
        rows.append(a)
        offsets.append(offsets[-1] + len(a))
    dets = np.concatenate(rows, 0).astype(np.float64) if rows else np.zeros((0, 4), np.float64)
    return {"dets": np.ascontiguousarray(dets), "frame_offsets": np.asarray(offsets, np.int32), "rows": rows}


def build_tracks(detections, names: Sequence[str], *, iou_thresh: float = 0.3, max_age: int = 1, min_hits: int = 3,
                 max_trackers: int = ops.SORT_MAX, boxes: str = "detection", backfill: bool = False,
                 min_frames: int = MIN_NUM_FRAMES, device="cuda") -> dict:
    """{person_id: {'bbox': [T,4] (cx, cy, w, h), 'frames': [T]}} - exactly what tester.load_tracking returns - from per-frame
    detections (detections_to_buffers reads them), one clip, the association made by ops.sort_tracks on `device`.  person_id is the
    tracker's id as a string; a track holds the frames in which SORT emitted its tracker, `frames` being positions in `names`.
    boxes = 'detection': the rows of `bbox` are the user's own detection rows taken by index, their dtype kept, so the crop is the one
    folder mode cuts from the same file; 'filtered': the Kalman filter's boxes (float64).  backfill: a track that was emitted at
    least once also takes every other frame in which its tracker took a detection - the first min_hits frames of a person who
    enters late, and the frames after a miss while the hit streak builds up again.  Tracks shorter than min_frames are dropped.
    More than max_trackers live people at a frame is a ValueError that names the frame."""
    import torch
    if boxes not in ("detection", "filtered"):
        raise ValueError(f"boxes must be 'detection' or 'filtered', got {boxes!r}")
    buf = detections_to_buffers(detections, names)
    fo = buf["frame_offsets"]
    res = ops.sort_tracks(torch.from_numpy(buf["dets"]).to(device), fo, None, iou_thresh=iou_thresh, max_age=max_age,
                          min_hits=min_hits, max_trackers=max_trackers)
    tracker, ident = res["tracker"].cpu().numpy(), res["id"].cpu().numpy()
    status = int(res["status"].cpu().numpy()[0])
    frame_of = (np.searchsorted(fo, np.arange(len(tracker)), side="right") - 1).astype(np.int64)
    if status != 0:
        first = int(frame_of[np.nonzero(tracker < 0)[0][0]]) if (tracker < 0).any() else -1
        raise ValueError(f"sort: more than {max_trackers} people are alive at frame {first} ({names[first]}): the tracker holds at most "
                         f"{ops.SORT_MAX}; thin the detections or raise --track_iou")
    user = np.concatenate(buf["rows"], 0) if len(tracker) else np.zeros((0, 4), np.float32)
    src = user if boxes == "detection" else res["box"].cpu().numpy()
    out = {}
    for pid in range(int(res["count"].cpu().numpy()[0])):
        emitted = ident == pid
        if not emitted.any():
            continue
        take = np.nonzero(tracker == pid if backfill else emitted)[0]       # ascending: frame order, one detection per frame
        if len(take) >= min_frames:
            out[str(pid)] = {"bbox": src[take], "frames": frame_of[take]}
    return out


def write_tracking(path: str, tracks: dict) -> None:
    """The tracks as a --tracking json (tester.load_tracking reads it back; repr keeps every float's value)."""
    import json
    with open(path, "w") as f:
        json.dump({pid: {"bbox": np.asarray(tr["bbox"], np.float64).tolist(), "frames": [int(v) for v in tr["frames"]]}
                   for pid, tr in tracks.items()}, f)


def flag_error(args) -> Optional[str]:
    """demo.py's --tracker and --track_* flags: what cannot work, as one line, or None."""
    tracker = getattr(args, "tracker", "none") or "none"
    given = [f for f, d in (("track_iou", 0.3), ("track_max_age", 1), ("track_min_hits", 3), ("track_boxes", "detection"),
                            ("track_backfill", False)) if getattr(args, f, d) != d]
    if tracker == "none":
        return f"--{given[0]} tunes --tracker sort: it needs --tracker sort" if given else None
    if args.mode != "video":
        return "--tracker sort builds the tracks of video mode: it needs --mode video"
    if getattr(args, "tracking", None):
        return "--tracker sort with --tracking: the tracks are either built from --detections or read from the file; choose one"
    if not getattr(args, "detections", None):
        return "--tracker sort associates per-frame person boxes: it needs --detections FILE"
    if getattr(args, "kp_refit", None) is not None:
        return "--kp_refit needs keypoint tracks (joints2d); --tracker sort builds box tracks"
    if not 0.0 < args.track_iou < 1.0:
        return f"--track_iou must be in (0, 1), got {args.track_iou}"
    if args.track_max_age < 0 or args.track_min_hits < 0:
        return "--track_max_age and --track_min_hits must be >= 0"
    return None
