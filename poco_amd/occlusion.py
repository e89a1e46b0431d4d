"""Occlusion sensitivity maps (demo.py --occlusion_map): PARE's occlusion sweep around the MI355X engine.  A constant
square slides over the 224 x 224 crop, the regressor runs on every occluded copy, and the change of the mesh and of each joint's
uncertainty against the unoccluded crop is kept per position and drawn as a heat map over the crop.

    sweep = OcclusionSweep(model, patch=40, stride=10)
    res = sweep.run(row)                               # row: one crop of POCOTester.make_batch
    pic = heat_overlay(field_of(res.records, "v2v"), res.positions, 40, canvas_u8)

The engine is used as it stands, in full batches with no host work between them; the three kernels around it are csrc/occlusion.hip
(poco_op_occlude_batch, poco_op_occlusion_records, poco_op_heat_overlay of include/poco_hip.h).  Nothing of size n x 6890 leaves
the device.  numpy restatement: tests/occlusion_np.py."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import PocoHipError, check, lib

REC = 77                            # POCO_OCCLUSION_RECORD_FLOATS
COL_V2V, COL_V2V_MAX, COL_VAR_MEAN, COL_DVAR_MEAN, COL_DVAR, COL_JOINTS = 0, 1, 2, 3, 4, 28
METRICS = ("v2v", "var", "joints")  # and "var:<0..23>"
# ToTensor + Normalize of the crop kernel (csrc/kernels_misc.hip; tester.crop_canvas inverts the same constants)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)

_FN = {}


def _fn(name: str, argtypes):
    if name not in _FN:
        f = getattr(lib(), name)
        f.argtypes = argtypes
        _FN[name] = f
    return _FN[name]


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def sweep_positions(res: int = 224, patch: int = 40, stride: int = 10) -> np.ndarray:
    """int32 [n, 2]: the (y0, x0) top-left corners of the sweep, row-major.  Per axis k * stride for k = 0 .. ceil((res - patch) /
    stride), the last one clamped to res - patch: every pixel lies under at least one patch and no patch leaves the crop."""
    res, patch, stride = int(res), int(patch), int(stride)
    if res < 1 or not 1 <= patch <= res or stride < 1:
        raise ValueError(f"sweep_positions: need 1 <= patch <= res and stride >= 1, got res {res}, patch {patch}, stride {stride}")
    steps = -(-(res - patch) // stride)
    axis = np.minimum(np.arange(steps + 1, dtype=np.int64) * stride, res - patch)
    yy, xx = np.meshgrid(axis, axis, indexing="ij")
    return np.ascontiguousarray(np.stack([yy.reshape(-1), xx.reshape(-1)], 1), dtype=np.int32)


def sweep_grid(res: int = 224, patch: int = 40, stride: int = 10) -> Tuple[int, int]:
    """(nh, nw) of sweep_positions: positions i = h * nw + w."""
    k = -(-(int(res) - int(patch)) // int(stride)) + 1
    return k, k


def fill_from_grey(level: float) -> Tuple[float, float, float]:
    """The normalised fill of a grey level 0..255, by the crop kernel's own constants: (level / 255 - mean) / std per channel, in
    float32 like the kernel."""
    if not 0 <= float(level) <= 255:
        raise ValueError(f"fill_from_grey: the grey level must be in 0..255, got {level}")
    p = np.float32(level) / np.float32(255)
    return tuple(float((p - np.float32(m)) / np.float32(s)) for m, s in zip(MEAN, STD))


def parse_metric(metric: str) -> Union[str, int]:
    """'v2v' | 'var' | 'joints' as they are, 'var:<j>' -> j (0..23); anything else is a ValueError."""
    if metric in METRICS:
        return metric
    if isinstance(metric, str) and metric.startswith("var:") and metric[4:].isdigit() and 0 <= int(metric[4:]) <= 23:
        return int(metric[4:])
    raise ValueError(f"occlusion metric must be v2v, var, joints or var:<0..23>, got {metric!r}")


def _positions(positions, device) -> torch.Tensor:
    if torch.is_tensor(positions):
        if not (positions.device == device and positions.dtype == torch.int32 and positions.is_contiguous() and positions.dim() == 2
                and positions.shape[1] == 2):
            raise PocoHipError("positions must be a contiguous int32 [n,2] tensor on the data's device")
        return positions
    p = np.ascontiguousarray(np.asarray(positions).reshape(-1, 2), np.int32)
    return torch.from_numpy(p).to(device)


def occlude_batch(src: torch.Tensor, positions, patch: int, fill: Sequence[float] = (0.0, 0.0, 0.0),
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[m,3,res,res] float32: m copies of the normalised crop `src` [3,res,res], copy i with fill[c] inside the patch x patch
    square at positions[i] = (y0, x0).  out: a contiguous float32 [m,3,res,res] tensor on src's device (a slice of a larger batch
    is fine).  One launch on the current stream."""
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.float32 and src.dim() == 3 and src.shape[0] == 3
            and src.shape[1] == src.shape[2] and src.is_contiguous()):
        raise PocoHipError("occlude_batch: src must be a contiguous float32 [3,res,res] device tensor")
    res = int(src.shape[1])
    pos = _positions(positions, src.device)
    m = int(pos.shape[0])
    f = np.ascontiguousarray(np.asarray(fill, np.float32).reshape(-1))
    if f.shape[0] != 3:
        raise PocoHipError("occlude_batch: fill must be three normalised values")
    if out is None:
        out = torch.empty(m, 3, res, res, device=src.device, dtype=torch.float32)
    elif not (torch.is_tensor(out) and out.device == src.device and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (m, 3, res, res)):
        raise PocoHipError(f"occlude_batch: out must be a contiguous float32 [{m},3,{res},{res}] tensor on src's device")
    fn = _fn("poco_op_occlude_batch", [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    check(fn(src.data_ptr(), res, pos.data_ptr() if m else None, m, int(patch), f.ctypes.data, out.data_ptr(), _stream(src)),
          "poco_op_occlude_batch")
    return out


def _rows(t, what: str, tail, device=None) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape[1:]) == tuple(tail)
            and (device is None or t.device == device)):
        raise PocoHipError(f"occlusion_records: {what} must be a contiguous float32 [m, {', '.join(map(str, tail))}] tensor on one device")
    return t


def occlusion_records(verts: torch.Tensor, var_pose: torch.Tensor, joints3d: torch.Tensor, base_verts: torch.Tensor,
                      base_var: torch.Tensor, base_joints3d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[m, 77] float32 records of the rows verts [m,V,3] / var_pose [m,24] / joints3d [m,49,3] against ONE baseline row
    (base_verts [1,V,3] or [V,3], base_var [1,24] or [24], base_joints3d [1,49,3] or [49,3]); the columns are those of
    poco_op_occlusion_records.  One launch on the current stream; two calls give the same bits."""
    if not (torch.is_tensor(verts) and verts.dim() == 3 and verts.shape[2] == 3):
        raise PocoHipError("occlusion_records: verts must be [m,V,3]")
    m, V = int(verts.shape[0]), int(verts.shape[1])
    dev = verts.device
    _rows(verts, "verts", (V, 3))
    _rows(var_pose, "var_pose", (24,), dev)
    _rows(joints3d, "joints3d", (49, 3), dev)
    if var_pose.shape[0] != m or joints3d.shape[0] != m:
        raise PocoHipError("occlusion_records: verts, var_pose and joints3d must have the same number of rows")
    bv = _rows(base_verts.reshape(-1, V, 3) if torch.is_tensor(base_verts) else base_verts, "base_verts", (V, 3), dev)
    ba = _rows(base_var.reshape(-1, 24) if torch.is_tensor(base_var) else base_var, "base_var", (24,), dev)
    bj = _rows(base_joints3d.reshape(-1, 49, 3) if torch.is_tensor(base_joints3d) else base_joints3d, "base_joints3d", (49, 3), dev)
    if not (bv.shape[0] == ba.shape[0] == bj.shape[0] == 1):
        raise PocoHipError("occlusion_records: the baseline is one row")
    if out is None:
        out = torch.empty(m, REC, device=dev, dtype=torch.float32)
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (m, REC)):
        raise PocoHipError(f"occlusion_records: out must be a contiguous float32 [{m},{REC}] tensor on the data's device")
    fn = _fn("poco_op_occlusion_records", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p])
    check(fn(verts.data_ptr(), var_pose.data_ptr(), joints3d.data_ptr(), m, V, bv.data_ptr(), ba.data_ptr(), bj.data_ptr(),
             out.data_ptr(), _stream(verts)), "poco_op_occlusion_records")
    return out


_LUT_U8 = None


def jet_lut_u8() -> np.ndarray:
    """uint8 [256,3]: render.jet_lut() as bytes, round(255 x)."""
    global _LUT_U8
    if _LUT_U8 is None:
        from .render import jet_lut
        _LUT_U8 = np.ascontiguousarray(np.round(jet_lut() * 255.0).astype(np.uint8))
    return _LUT_U8


_LUT_DEV: Dict[torch.device, torch.Tensor] = {}


def heat_overlay(field: torch.Tensor, positions, patch: int, crop: torch.Tensor, scale: Union[str, float] = "auto",
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [res,res,3]: the heat map of `field` (float32 [n], one value per sweep position) over `crop` (uint8 [res,res,3], the
    --render_crop canvas of POCOTester.crop_canvas).  Per pixel the field is averaged over the patches covering it, divided by
    `scale` (a positive float, or "auto" = the field's maximum, found on the device), clamped to [0, 1], looked up in jet and
    blended 50 % over the crop (poco_op_heat_overlay); byte-equal to tests/occlusion_np.py.  One launch on the current stream."""
    if not (torch.is_tensor(crop) and crop.is_cuda and crop.dtype == torch.uint8 and crop.dim() == 3 and crop.shape[2] == 3
            and crop.shape[0] == crop.shape[1] and crop.is_contiguous()):
        raise PocoHipError("heat_overlay: crop must be a contiguous uint8 [res,res,3] device tensor")
    dev = crop.device
    pos = _positions(positions, dev)
    n = int(pos.shape[0])
    if not (torch.is_tensor(field) and field.device == dev and field.dtype == torch.float32 and field.is_contiguous()
            and tuple(field.shape) == (n,)):
        raise PocoHipError(f"heat_overlay: field must be a contiguous float32 [{n}] tensor on the crop's device")
    if isinstance(scale, str):
        if scale != "auto":
            raise PocoHipError(f"heat_overlay: scale must be a positive float or 'auto', got {scale!r}")
        sc = 0.0
    else:
        sc = float(scale)
        if not (sc > 0 and np.isfinite(sc)):
            raise PocoHipError(f"heat_overlay: scale must be a positive float or 'auto', got {scale!r}")
    if out is None:
        out = torch.empty_like(crop)
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.uint8 and out.is_contiguous()
              and out.shape == crop.shape):
        raise PocoHipError("heat_overlay: out must be a contiguous uint8 tensor of the crop's shape on its device")
    if dev not in _LUT_DEV:
        _LUT_DEV[dev] = torch.from_numpy(jet_lut_u8()).to(dev)
    fn = _fn("poco_op_heat_overlay", [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p])
    check(fn(field.data_ptr(), pos.data_ptr(), n, int(patch), int(crop.shape[0]), sc, _LUT_DEV[dev].data_ptr(), crop.data_ptr(),
             out.data_ptr(), _stream(crop)), "poco_op_heat_overlay")
    return out


def field_of(records: torch.Tensor, metric: Union[str, int] = "v2v") -> torch.Tensor:
    """The scalar field [n] a metric draws: 'v2v' = column 0 (mean vertex displacement), 'var' = column 3 (mean change of the
    per-joint uncertainty), an int j or 'var:<j>' = column 4 + j (that joint's change), 'joints' = the mean of columns 28:77 (the 49
    joints' displacement; a float32 torch reduction on the device).  A negative change (the occluder made the model surer) is
    drawn at the cold end."""
    m = parse_metric(metric) if isinstance(metric, str) else int(metric)
    if m == "v2v":
        return records[:, COL_V2V].contiguous()
    if m == "var":
        return records[:, COL_DVAR_MEAN].contiguous()
    if m == "joints":
        return records[:, COL_JOINTS:REC].mean(1).contiguous()
    if not 0 <= m <= 23:
        raise ValueError(f"field_of: joint index must be in 0..23, got {m}")
    return records[:, COL_DVAR + m].contiguous()


BASELINE_KEYS = ("smpl_vertices", "smpl_joints3d", "smpl_joints2d", "pred_cam", "pred_pose", "pred_shape", "var_pose")


@dataclass
class SweepResult:
    records: torch.Tensor            # [n, 77] float32 on the device
    positions: torch.Tensor          # [n, 2] int32 on the device, (y0, x0) row-major
    baseline: Dict[str, torch.Tensor]    # the unoccluded crop's outputs, one row each (BASELINE_KEYS)
    grid: Tuple[int, int]            # (nh, nw): records.view(nh, nw, 77)
    patch: int
    stride: int


class OcclusionSweep:
    """The sweep on one normalised crop.

        OcclusionSweep(model, patch=40, stride=10, fill=(0, 0, 0)).run(row) -> SweepResult

    row: ONE row of the batch dict POCOTester.make_batch produces (img [1,3,224,224] and the per-crop keys); bbox_info and the
    other per-crop keys are repeated unchanged for every occluded copy.  Row 0 of the first chunk is the unoccluded crop (the
    baseline), the n occluded copies follow; chunks hold model.max_batch rows, the last one is short.  Per chunk: one
    occlude_batch launch into the chunk's image buffer, one forward, one occlusion_records launch against the baseline row - all
    on the current stream, nothing read back in between.  fill: three normalised values (0 = the dataset mean colour)."""

    def __init__(self, model, patch: int = 40, stride: int = 10, fill: Sequence[float] = (0.0, 0.0, 0.0)):
        self.model = model
        self.patch, self.stride = int(patch), int(stride)
        self.fill = tuple(float(v) for v in np.asarray(fill, np.float32).reshape(-1))
        if len(self.fill) != 3:
            raise ValueError("OcclusionSweep: fill must be three normalised values")
        if int(model.max_batch) < 2:
            raise ValueError("OcclusionSweep: the model needs max_batch >= 2 (the baseline row shares the first chunk)")
        sweep_positions(224, self.patch, self.stride)            # raises on a bad patch / stride

    @torch.no_grad()
    def run(self, row: Dict[str, torch.Tensor], check: bool = True) -> SweepResult:
        img = row["img"]
        if not (torch.is_tensor(img) and img.is_cuda and img.dtype == torch.float32 and img.dim() == 4 and img.shape[0] == 1
                and img.shape[1] == 3 and img.shape[2] == img.shape[3]):
            raise PocoHipError("OcclusionSweep.run: row['img'] must be a float32 [1,3,res,res] device tensor (one crop)")
        src = img[0].contiguous()
        res = int(src.shape[1])
        dev = src.device
        pos = torch.from_numpy(sweep_positions(res, self.patch, self.stride)).to(dev)
        n = int(pos.shape[0])
        mb = int(self.model.max_batch)
        records = torch.empty(n, REC, device=dev, dtype=torch.float32)
        buf = torch.empty(min(mb, n + 1), 3, res, res, device=dev, dtype=torch.float32)
        others = {k: v for k, v in row.items() if k != "img"}
        for k, v in others.items():
            if not (torch.is_tensor(v) and v.shape[0] == 1):
                raise PocoHipError(f"OcclusionSweep.run: row[{k!r}] must be a tensor with one row")
        rep = {}                                                 # chunk size -> the per-crop keys repeated (two sizes at most)
        baseline = None
        done = 0
        while done < n:
            lead = 1 if baseline is None else 0                 # the first chunk starts with the unoccluded crop
            k = min(mb - lead, n - done)
            B = lead + k
            if lead:
                buf[0].copy_(src)
            occlude_batch(src, pos[done:done + k], self.patch, self.fill, out=buf[lead:B])
            if B not in rep:
                rep[B] = {key: v.expand(B, *v.shape[1:]).contiguous() for key, v in others.items()}
            out = self.model({"img": buf[:B], **rep[B]}, want_segm=False)
            if lead:
                baseline = {key: out[key][:1].clone() for key in BASELINE_KEYS}
            occlusion_records(out["smpl_vertices"][lead:], out["var_pose"][lead:], out["smpl_joints3d"][lead:],
                              baseline["smpl_vertices"], baseline["var_pose"], baseline["smpl_joints3d"],
                              out=records[done:done + k])
            done += k
        if check:
            self.model.check_status(sync=True)                   # a timed-out in-kernel wait = invalid rows: raise
        return SweepResult(records, pos, baseline, sweep_grid(res, self.patch, self.stride), self.patch, self.stride)
