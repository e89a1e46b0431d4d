"""Image degradation sweep (eval.py --corrupt LEVELS [--corrupt_seed S]): every crop is cut raw by the dataset crop, K versions of it -
the clean crop and one per level - are made by poco_op_corrupt (csrc/corrupt.hip; a jpeg step goes through the device's JPEG encoder
and decoder), normalised and regressed in ONE forward of K * b rows, level-major; every level is then scored side by side like the
labels of --cfg2.  The question the sweep answers: does `var` grow when the error grows, and by how much.  The contract is stated in
include/poco_hip.h and DESIGN.md section 35; tests/corrupt_np.py restates it."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import PocoHipError

MAX_LEVELS = 8
MAX_STEPS = ops.CORRUPT_MAX_STEPS
# kind -> (what its value is, lowest, highest, lowest is excluded)
RANGES = {"gaussian_blur": ("sigma", 0.0, 5.0, True), "motion_blur": ("length", 3, 31, False), "pixelate": ("factor", 2, 32, False),
          "contrast": ("c", 0.0, 2.0, False), "gamma": ("g", 0.2, 5.0, False), "gaussian_noise": ("sigma", 0.0, 255.0, False),
          "jpeg": ("quality", 1, 100, False)}
INTEGER = ("motion_blur", "pixelate", "jpeg")


@dataclass(frozen=True)
class Step:
    """One step of a chain: its kind, its value (sigma, length, factor, c, g, sigma, quality) and for motion_blur the direction in
    degrees (0 = along x, counter-clockwise in image coordinates with y down: the sample offsets are k (cos, sin))."""
    kind: str
    value: float
    degrees: float = 0.0

    def describe(self) -> str:
        return f"{self.kind}:{self.value:g}" + (f":{self.degrees:g}" if self.kind == "motion_blur" else "")


Level = Tuple[Step, ...]


def describe(level: Level) -> str:
    return "+".join(s.describe() for s in level) or "clean"


def levels_text(levels: Sequence[Level]) -> str:
    return ",".join(describe(lv) for lv in levels)


def parse_levels(text: str) -> List[Level]:
    """"gaussian_blur:1,gaussian_blur:2+jpeg:30,motion_blur:9:45" -> [(), (blur 1), (blur 2, jpeg 30), (motion 9 at 45 degrees)]:
    levels separated by commas, each a '+'-joined chain of kind:value (motion_blur:L:degrees); the clean crop is always level 0.
    ValueError: an empty or unreadable level, an unknown kind, a value outside its range or not finite, a chain of more than 4
    steps, a level given twice, more than 8 levels in all."""
    levels: List[Level] = [()]
    if not isinstance(text, str) or not text.strip():
        raise ValueError("--corrupt needs at least one level, e.g. --corrupt gaussian_blur:2")
    for item in text.split(","):
        chain = []
        for part in item.strip().split("+"):
            fields = part.strip().split(":")
            kind = fields[0]
            if kind not in RANGES:
                raise ValueError(f"--corrupt: cannot read {part.strip()!r} in level {item.strip()!r}: a level is a '+'-joined chain of kind:value with "
                                 f"kind one of {', '.join(RANGES)}")
            if len(fields) != (3 if kind == "motion_blur" else 2):
                raise ValueError(f"--corrupt: {part.strip()!r} must read {kind}:{'L:degrees' if kind == 'motion_blur' else RANGES[kind][0]}")
            try:
                nums = [float(f) for f in fields[1:]]
            except ValueError:
                nums = [float("nan")]
            if not all(math.isfinite(v) for v in nums):
                raise ValueError(f"--corrupt: {part.strip()!r} needs finite numbers")
            what, lo, hi, open_lo = RANGES[kind]
            v = nums[0]
            if v < lo or v > hi or (open_lo and v == lo) or (kind in INTEGER and v != int(v)) or (kind == "motion_blur" and int(v) % 2 == 0):
                kindly = "an odd integer" if kind == "motion_blur" else ("an integer" if kind in INTEGER else "a number")
                raise ValueError(f"--corrupt: {kind} needs {what} = {kindly} in {'(' if open_lo else '['}{lo:g}, {hi:g}], got {fields[1]}")
            chain.append(Step(kind, float(v), float(nums[1]) if kind == "motion_blur" else 0.0))
        if len(chain) > MAX_STEPS:
            raise ValueError(f"--corrupt: level {item.strip()!r} chains {len(chain)} steps, at most {MAX_STEPS}")
        level = tuple(chain)
        if level in levels:
            raise ValueError(f"--corrupt: level {item.strip()!r} is given twice")
        levels.append(level)
        if len(levels) > MAX_LEVELS:
            raise ValueError(f"--corrupt: at most {MAX_LEVELS} levels in all, the clean crop included")
    return levels


# ---- records -------------------------------------------------------------------------------------------------------------------
def step_record(step: Step, seed: int = 0, stream: int = 0) -> tuple:
    """One ops.CORRUPT_STEP record.  motion_blur's unit direction is computed here, in float64, and rounded to float32."""
    kind = ops.CORRUPT_KINDS.index(step.kind)
    ival, p0, p1 = 0, 0.0, 0.0
    if step.kind in INTEGER:
        ival = int(step.value)
    else:
        p0 = step.value
    if step.kind == "motion_blur":
        a = math.radians(step.degrees)
        p0, p1 = math.cos(a), math.sin(a)
    return (kind, ival, p0, p1, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF), int(stream) & 0xFFFFFFFF)


def records(chains: Sequence[Level], streams: Sequence[int], seed: int = 0) -> np.ndarray:
    """The [N, L] record array of ops.corrupt for N crops with the chains given (L = the longest, at least 1); streams[i] = the
    name crop i's noise is drawn under (eval.py: its dataset row)."""
    if len(chains) != len(streams) or not len(chains):
        raise ValueError("records: one stream per chain, at least one chain")
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"records: seed must be in 0..2^64-1, got {seed}")
    L = max(1, max(len(c) for c in chains))
    if L > MAX_STEPS:
        raise ValueError(f"records: a chain of {L} steps, at most {MAX_STEPS}")
    rec = np.zeros((len(chains), L), ops.CORRUPT_STEP)
    for i, (chain, stream) in enumerate(zip(chains, streams)):
        for p, step in enumerate(chain):
            rec[i, p] = step_record(step, seed, stream)
    return rec


def level_major_records(levels: Sequence[Level], rows: Sequence[int], seed: int = 0) -> np.ndarray:
    """records for K levels of the b crops `rows`, level-major: row k * b + i is level k of crop i, its noise named by rows[i]."""
    b = len(rows)
    return records([lv for lv in levels for _ in range(b)], [int(r) for _ in levels for r in rows], seed)


# ---- the flags of eval.py --------------------------------------------------------------------------------------------------------
EXCLUDED = ("tta", "cfg2", "segm", "likelihood", "sequences", "visibility", "kp_refit", "calibrate", "rank_metrics")


def flag_error(args):
    """The one sentence that refuses --corrupt / --corrupt_seed where they cannot work, or None."""
    text = getattr(args, "corrupt", None)
    if text is None:
        if getattr(args, "corrupt_seed", None) is not None:
            return "--corrupt_seed seeds the noise of --corrupt: it needs --corrupt"
        return None
    try:
        parse_levels(text)
    except ValueError as e:
        return str(e)
    seed = getattr(args, "corrupt_seed", None)
    if seed is not None and not 0 <= int(seed) < 1 << 64:
        return f"--corrupt_seed must be in 0..2^64-1, got {seed}"
    for flag in EXCLUDED:
        v = getattr(args, flag, None)
        if v is not None and v is not False:
            return f"--{flag} reads one forward's outputs of one version of a crop: it cannot be combined with --corrupt"
    if getattr(args, "ckpt2", None):
        return "--ckpt2 names a second model: it cannot be combined with --corrupt"
    if getattr(args, "crop", "demo") != "dataset":
        return "--corrupt degrades the raw crops of the dataset crop: it needs --crop dataset"
    return None


# ---- the model behind K levels ---------------------------------------------------------------------------------------------------
class CorruptModel:
    """A finalized engine behind K levels, modelled on tta.TTAModel: forward_levels(batch, rows) takes the batch dict of b RAW crops
    (EvalDataset with raw_crop = True), makes the K level-major versions with ops.corrupt, normalised, and regresses them in ONE
    forward of K * b rows; max_batch = the crops one forward takes = max(1, the engine's max_batch // K)."""

    def __init__(self, model, levels: Sequence[Level], seed: int = 0):
        levels = list(levels)
        if not 2 <= len(levels) <= MAX_LEVELS or levels[0] != ():
            raise ValueError(f"CorruptModel needs 2 to {MAX_LEVELS} levels, the clean crop first")
        if not getattr(model, "_finalized", False):
            raise PocoHipError("CorruptModel needs a finalized engine")
        if model.max_batch < len(levels):
            raise PocoHipError(f"CorruptModel: the engine's max_batch {model.max_batch} does not hold the {len(levels)} levels of one crop")
        self.model, self.levels, self.seed, self.K = model, levels, int(seed), len(levels)
        self.device, self.max_batch = model.device, max(1, model.max_batch // len(levels))
        self._bufs = {}

    def level_batch(self, batch: Dict[str, torch.Tensor], rows: Sequence[int]) -> Dict[str, torch.Tensor]:
        """The K * b-row level-major batch dict: `img` from ops.corrupt, every other entry repeated K times."""
        raw = batch["img"]
        b, K = int(raw.shape[0]), self.K
        if len(rows) != b:
            raise PocoHipError(f"CorruptModel: {b} crops but {len(rows)} row names")
        x = raw.repeat(K, 1, 1, 1)
        key = tuple(x.shape)
        if key not in self._bufs:
            self._bufs = {key: (torch.empty_like(x), torch.empty_like(x))}
        out, tmp = self._bufs[key]
        img = ops.corrupt(x, level_major_records(self.levels, rows, self.seed), True, out=out, tmp=tmp)
        rep = {k: (v.repeat(K, *([1] * (v.dim() - 1))) if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == b else v) for k, v in batch.items()}
        rep["img"] = img
        return rep

    @torch.no_grad()
    def forward_levels(self, batch: Dict[str, torch.Tensor], rows: Sequence[int]):
        """The K per-level output dicts of the raw batch: level_batch, then forward_rows."""
        return self.forward_rows(self.level_batch(batch, rows))

    @torch.no_grad()
    def forward_rows(self, lb: Dict[str, torch.Tensor]):
        """The K per-level output dicts of a level-major batch: row slices of the one forward's output."""
        n = int(lb["img"].shape[0])
        if n % self.K:
            raise PocoHipError(f"CorruptModel: a batch of {n} rows is not {self.K} levels of whole crops")
        b = n // self.K
        out = self.model(lb, want_segm=False)
        return [{k: (v[i * b:(i + 1) * b] if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == n else v) for k, v in out.items()}
                for i in range(self.K)]

    def smpl_lbs(self, betas, rotmat):
        return self.model.smpl_lbs(betas, rotmat)

    def check_status(self, sync: bool = False) -> None:
        self.model.check_status(sync)
