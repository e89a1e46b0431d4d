"""Sequences in a dataset file (eval.py --sequences): the rows of the reference's dataset .npz are single
crops, but 3DPW and Human3.6M list consecutive frames.  group_tracks finds the tracks from the image names on the host;
parse_pipelines reads --seq_post; flag_error refuses what cannot work with --sequences.  The temporal metric itself is
ops.track_accel (csrc/track_accel.hip), the evaluation loop evaluate.run_eval_sequences."""
from __future__ import annotations

import math
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_PIPELINES = 4
STEP_NAMES = ("infill", "smooth_uncert", "smooth")
SUMMARY_FIELDS = ("mpjpe", "pampjpe", "v2v", "accel", "accel_err", "changed", "valid")   # the columns of seq_summary
_DIGITS = re.compile(r"\d+")


def group_tracks(imgname: Sequence[str], person_id=None) -> Dict[str, object]:
    """-> dict(order int32 [N], offsets int32 [P+1], frames int32 [N], names list[str]).  A track is the rows that share (imgname
    with its basename removed, person): person = person_id[i] where the file has that key, else the rank of row i among the rows
    with the identical imgname, in file order (3DPW lists two people of one frame as two rows).  The frame id is the last run of
    decimal digits of the basename without its extension.  Within a track the rows are ordered by frame id; the tracks are ordered
    by their first row in the file.  `order` gathers file rows into track-major rows; `frames` is in track-major order.
    ValueError: a basename without digits (the row is named), two rows of one track with the same frame id."""
    names = [str(x) for x in imgname]
    n = len(names)
    if person_id is not None:
        person_id = np.asarray(person_id).reshape(-1)
        if len(person_id) != n:
            raise ValueError(f"person_id has {len(person_id)} entries for {n} rows")
    seen: Dict[str, int] = {}
    tracks: Dict[Tuple[str, object], List[Tuple[int, int]]] = {}                # key -> [(frame id, row)], keys in first-row order
    for i, nm in enumerate(names):
        folder, base = os.path.split(nm)
        runs = _DIGITS.findall(os.path.splitext(base)[0])
        if not runs:
            raise ValueError(f"row {i}: the basename of {nm!r} holds no frame number")
        if person_id is not None:
            person = person_id[i].item()
        else:
            person = seen.get(nm, 0)
            seen[nm] = person + 1
        tracks.setdefault((folder, person), []).append((int(runs[-1]), i))
    order, frames, offsets, out_names = [], [], [0], []
    for (folder, person), rows in tracks.items():
        rows.sort()                                                              # by frame id (rows of equal id: caught below)
        for (fa, ia), (fb, ib) in zip(rows, rows[1:]):
            if fa == fb:
                raise ValueError(f"rows {ia} and {ib} are both frame {fa} of track {folder!r} person {person}")
        frames += [f for f, _ in rows]
        order += [i for _, i in rows]
        offsets.append(len(order))
        out_names.append(f"{folder}#{person}")
    if frames and (max(frames) > 2 ** 31 - 2):
        raise ValueError("a frame number exceeds the int32 range")
    return {"order": np.asarray(order, np.int32), "offsets": np.asarray(offsets, np.int32), "frames": np.asarray(frames, np.int32),
            "names": out_names}


def parse_pipelines(text: Optional[str]) -> List[List[Tuple[str, Optional[float]]]]:
    """--seq_post: at most four comma-separated pipelines, each a '+'-joined chain of infill:<thresh>, smooth_uncert:<lambda> and
    smooth -> [[(step, parameter | None), ...], ...].  ValueError names what is wrong."""
    if text is None or not str(text).strip():
        return []
    out = []
    for pipe in str(text).split(","):
        steps = []
        for word in pipe.strip().split("+"):
            name, sep, arg = word.strip().partition(":")
            if name not in STEP_NAMES:
                raise ValueError(f"--seq_post: unknown step {word.strip()!r} (infill:<thresh>, smooth_uncert:<lambda>, smooth)")
            if name == "smooth":
                if sep:
                    raise ValueError("--seq_post: smooth takes no parameter (--min_cutoff and --beta set the one-euro filter)")
                steps.append((name, None))
                continue
            try:
                val = float(arg)
            except ValueError:
                val = float("nan")
            if not sep or not math.isfinite(val):
                raise ValueError(f"--seq_post: {name} needs a finite parameter, as in {name}:{'0.3' if name == 'infill' else '10'}")
            if name == "smooth_uncert" and not 0.0 < val <= 1e4:
                raise ValueError(f"--seq_post: the lambda of smooth_uncert must be in (0, 1e4], got {val!r}")
            steps.append((name, val))
        out.append(steps)
    if len(out) > MAX_PIPELINES:
        raise ValueError(f"--seq_post: at most {MAX_PIPELINES} pipelines, got {len(out)}")
    return out


def pipeline_text(steps) -> str:
    return "+".join(name if val is None else f"{name}:{val:g}" for name, val in steps)


def flag_error(args) -> Optional[str]:
    """eval.py: what cannot work with --sequences, and --seq_* without it; None when all is well.  An augmentation drawn per sample
    breaks the continuity in time that the metric measures, so every --aug_* flag and --augment is refused."""
    seq = bool(getattr(args, "sequences", False))
    post = getattr(args, "seq_post", None)
    if not seq:
        for flag in ("seq_post", "seq_max_gap", "seq_uncert_ref", "min_cutoff", "beta"):
            if getattr(args, flag, None) is not None:
                return f"--{flag} needs --sequences"
        return None
    for flag, on in (("--cfg2", getattr(args, "cfg2", None) is not None), ("--ckpt2", getattr(args, "ckpt2", None) is not None),
                     ("--tta", getattr(args, "tta", None) is not None), ("--segm", bool(getattr(args, "segm", False))),
                     ("--likelihood", bool(getattr(args, "likelihood", False))),
                     ("--rank_metrics", bool(getattr(args, "rank_metrics", False))),
                     ("--aug_rot", getattr(args, "aug_rot", None) is not None), ("--aug_scale", getattr(args, "aug_scale", None) is not None),
                     ("--aug_flip", bool(getattr(args, "aug_flip", False))), ("--aug_noise", getattr(args, "aug_noise", None) is not None),
                     ("--aug_occlude", getattr(args, "aug_occlude", None) is not None), ("--augment", bool(getattr(args, "augment", False)))):
        if on:
            return f"--sequences cannot be combined with {flag}"
    try:
        parse_pipelines(post)
    except ValueError as e:
        return str(e)
    gap = getattr(args, "seq_max_gap", None)
    if gap is not None and int(gap) < 1:
        return f"--seq_max_gap must be at least 1, got {gap}"
    ref = getattr(args, "seq_uncert_ref", None)
    if ref is not None and not (math.isfinite(float(ref)) and float(ref) > 0):
        return f"--seq_uncert_ref must be finite and positive, got {ref}"
    return None
