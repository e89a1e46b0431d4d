"""Body-part segmentation (eval.py --segm, demo.py --save_segm): the ground truth the reference trains PARE's pred_segm_mask against -
the SMPL mesh rasterised into a map of 24 body parts plus background (pocolib/core/trainer.py:231-262, image_utils.generate_part_labels,
geometry.estimate_translation) - and the score of the mask against it (pocolib/losses/segmentation.py:CrossEntropy, pixel accuracy,
IoU), made on the GPU: poco_amd/ops.py part_labels / estimate_translation / segm_score / segm_argmax (csrc/part_labels.hip,
csrc/segm_metrics.hip).  Per crop nothing goes to the host between the forward and SegmAccumulator.finish().

tests/segm_np.py restates all of it in numpy and is the yardstick of tests/test_segm_*.py.  DESIGN.md section 21 has the contract."""
from __future__ import annotations

import os
import pickle
from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from ._lib import PocoHipError

NUM_PARTS = 24
NUM_CLASSES = NUM_PARTS + 1                  # background = 0, part p = p + 1
FOCAL_LENGTH = 5000.0                        # DATASET.FOCAL_LENGTH of the reference's configs
SEGM_DATASET_KEYS = ("pose", "shape", "part")


# ---- which part a face belongs to ------------------------------------------------------------------------------------------------
def vertex_parts_from_weights(lbs_weights) -> np.ndarray:
    """uint8 [V]: the joint with the largest skinning weight of each vertex (the lowest joint on a tie).  The default mapping: the
    reference's data/smpl_partSegmentation_mapping.pkl is not redistributable; pass it with --part_mapping to use it instead."""
    w = np.asarray(lbs_weights)
    if w.ndim != 2 or w.shape[1] != NUM_PARTS:
        raise ValueError(f"lbs_weights must be [V, {NUM_PARTS}], got {w.shape}")
    return np.argmax(w, axis=1).astype(np.uint8)


def _check_mapping(a, path: str) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iuf":
        raise ValueError(f"{path}: the part mapping must be one number per vertex, got shape {a.shape} of {a.dtype}")
    r = np.rint(a.astype(np.float64))
    if not (np.all(np.isfinite(r)) and np.all(r == a) and r.min() >= 0 and r.max() < NUM_PARTS):
        raise ValueError(f"{path}: the part mapping must hold integers in 0..{NUM_PARTS - 1}")
    return r.astype(np.uint8)


def load_part_mapping(path: str) -> np.ndarray:
    """uint8 [V] from a .npy, a .npz (its `smpl_index`, or its only array) or the reference's smpl_partSegmentation_mapping.pkl (a
    dict with `smpl_index`; written with joblib, which is used when it is installed, plain pickle otherwise)."""
    if not os.path.isfile(path):
        raise ValueError(f"part mapping not found: {path}")
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return _check_mapping(np.load(path, allow_pickle=False), path)
    if ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            if "smpl_index" in z.files:
                return _check_mapping(z["smpl_index"], path)
            if len(z.files) == 1:
                return _check_mapping(z[z.files[0]], path)
            raise ValueError(f"{path}: no `smpl_index` among {z.files}")
    try:
        import joblib
        d = joblib.load(path)
    except ImportError:
        with open(path, "rb") as f:
            d = pickle.load(f, encoding="latin1")
    if not (isinstance(d, dict) and "smpl_index" in d):
        raise ValueError(f"{path}: expected a dict with `smpl_index`")
    return _check_mapping(d["smpl_index"], path)


def face_parts(vertex_part, faces) -> np.ndarray:
    """uint8 [F]: the minimum over a face's three vertices, as get_body_part_texture's vertex_colors[faces].min(axis=1)."""
    vp = np.asarray(vertex_part)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= vp.shape[0]):
        raise ValueError(f"faces index vertices outside 0..{vp.shape[0] - 1}")
    return vp[f].min(axis=1).astype(np.uint8)


# ---- the two device operators ----------------------------------------------------------------------------------------------------
def _dev_f32(a, device) -> torch.Tensor:
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return a.to(device=device, dtype=torch.float32).contiguous()


class PartMesh:
    """The triangles and their parts on the device: PartMesh(faces [F,3], face_part [F], device)."""

    def __init__(self, faces, face_part, device):
        f = np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1, 3).astype(np.int32))
        fp = np.ascontiguousarray(np.asarray(face_part, np.uint8).reshape(-1))
        if f.shape[0] < 1 or fp.shape[0] != f.shape[0]:
            raise ValueError(f"need one part per face: {f.shape[0]} faces, {fp.shape[0]} parts")
        if fp.max() >= NUM_PARTS:
            raise ValueError(f"face parts must be in 0..{NUM_PARTS - 1}")
        self.device = torch.device(device)
        self.faces = torch.from_numpy(f).to(self.device)
        self.face_part = torch.from_numpy(fp).to(self.device)

    @classmethod
    def from_smpl(cls, smpl, device, part_mapping: Optional[str] = None) -> "PartMesh":
        """smpl: the body-model arrays (a dict or an open .npz) with `faces` and `lbs_weights`."""
        if "faces" not in smpl:
            raise ValueError("the body-model file has no `faces` array (convert the SMPL .pkl with tools/convert_smpl.py)")
        vp = load_part_mapping(part_mapping) if part_mapping else vertex_parts_from_weights(smpl["lbs_weights"])
        nv = int(np.asarray(smpl["lbs_weights"]).shape[0])
        if vp.shape[0] != nv:
            raise ValueError(f"the part mapping has {vp.shape[0]} entries, the body model {nv} vertices")
        return cls(smpl["faces"], face_parts(vp, smpl["faces"]), device)


def part_labels(verts, cam_t, mesh: PartMesh, focal: float = FOCAL_LENGTH, res: int = 224, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,res,res] on the device: 0 = background, p + 1 = part p, of verts [B,V,3] seen from cam_t [B,3] with the reference's
    crop camera (ops.part_labels).  Enqueued on the current stream."""
    return ops.part_labels(_dev_f32(verts, mesh.device), _dev_f32(cam_t, mesh.device), mesh.faces, mesh.face_part, float(focal), int(res), out)


def estimate_translation(joints3d, joints2d, focal: float = FOCAL_LENGTH, res: int = 224, device=None) -> torch.Tensor:
    """geometry.estimate_translation without its slice: joints3d [B,J,3], joints2d [B,J,3] = (x, y, confidence) in crop pixels ->
    cam_t [B,3] on the device (ops.estimate_translation)."""
    dev = joints3d.device if torch.is_tensor(joints3d) else (device or torch.device("cuda", torch.cuda.current_device()))
    return ops.estimate_translation(_dev_f32(joints3d, dev), _dev_f32(joints2d, dev), float(focal), int(res))


def crop_keypoints24(part, center, scale, res: int = 224) -> np.ndarray:
    """base_dataset.py:223-235 j2d_processing without augmentation, followed by trainer.py:231-234: the dataset's `part` [N,24,3]
    (x, y, confidence in original-image pixels) in crop pixels.  The reference's transform() truncates toward zero and adds 1
    (image_utils.py:111-118); normalising to [-1, 1] and back is the identity up to float32 rounding and is not repeated.
    float32 [N,24,3]; the confidence is passed through."""
    p = np.asarray(part, np.float64).reshape(-1, NUM_PARTS, 3)
    c = np.asarray(center, np.float64).reshape(-1, 1, 2)
    h = 200.0 * np.asarray(scale, np.float64).reshape(-1, 1)
    out = np.empty_like(p)
    for k in range(2):
        t = p[:, :, k] * (res / h) + res * (-c[:, :, k] / h + 0.5)
        out[:, :, k] = np.trunc(t) + 1.0
    out[:, :, 2] = p[:, :, 2]
    return out.astype(np.float32)


# ---- accumulation --------------------------------------------------------------------------------------------------------------------
class SegmAccumulator:
    """Device-side accumulator of the segmentation score.

        acc = SegmAccumulator(capacity=len(dataset))
        acc.step(out["pred_segm_mask"], labels)                  # per batch, enqueued on the current stream
        res = acc.finish()                                       # val_segm_ce, val_segm_pixel_acc, val_segm_iou [25], val_segm_miou ...

    One record of 2 + 3C 64-bit words per crop stays on the device (ops.segm_score); finish() reduces them once, in fp64."""

    def __init__(self, capacity: int, num_classes: int = NUM_CLASSES, device=None):
        if int(capacity) < 1:
            raise PocoHipError("SegmAccumulator: capacity must be at least 1")
        if not 1 <= int(num_classes) <= 32:
            raise PocoHipError("SegmAccumulator: num_classes must be in 1..32")
        self.capacity, self.count, self.C = int(capacity), 0, int(num_classes)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.records = torch.zeros(self.capacity, ops.segm_record_words(self.C), device=self.device, dtype=torch.int64)
        self.pixels = 0                                          # label pixels per crop, the same for every step

    def step(self, logits: torch.Tensor, labels: torch.Tensor) -> None:
        """logits [B,C,h,w], labels uint8 [B,H,W]: records of B crops at records[count .. count + B).  More crops than the capacity
        holds is an error and leaves the records as they were.  Nothing is copied to the host."""
        B = int(logits.shape[0])
        if logits.dim() != 4 or int(logits.shape[1]) != self.C:
            raise PocoHipError(f"SegmAccumulator.step: logits must be [B, {self.C}, h, w], got {tuple(logits.shape)}")
        if labels.dim() != 3 or int(labels.shape[0]) != B:
            raise PocoHipError("SegmAccumulator.step: labels must be [B, H, W] with the batch size of the logits")
        if self.count + B > self.capacity:
            raise PocoHipError(f"SegmAccumulator.step: {self.count} + {B} crops exceed the capacity of {self.capacity}")
        pix = int(labels.shape[1]) * int(labels.shape[2])
        if self.count and pix != self.pixels:
            raise PocoHipError("SegmAccumulator.step: the label maps of one run must have one size")
        self.pixels = pix
        with torch.cuda.device(self.device):
            ops.segm_score(logits, labels, out=self.records[self.count:self.count + B])
        self.count += B

    def reset(self) -> None:
        self.count = 0

    def finish(self, return_records: bool = False) -> Dict[str, object]:
        """val_segm_ce = the mean of -log_softmax[label] over all pixels of all crops (what CrossEntropy returns for the whole set as
        one batch), val_segm_pixel_acc, val_segm_iou [C] (NaN for a class absent from prediction and ground truth), val_segm_miou
        = the mean over the other classes, val_segm_miou_fg = the same without background.  return_records: also segm_ce [N] (the
        per-crop sums, fp64) and segm_counts int64 [N, 1 + 3C].  Synchronises the current stream."""
        if self.count < 1:
            raise PocoHipError("SegmAccumulator.finish: no crop has been stepped")
        rec = self.records[:self.count]
        ce_sum = rec[:, 0].contiguous().view(torch.float64).sum()           # one fp64 reduction on the device ...
        tot = rec[:, 1:].sum(0)                                            # ... and one of the integer counts
        host = torch.cat([ce_sum.reshape(1), tot.to(torch.float64)]).cpu().numpy()
        out = summarize(host[0], host[1:], self.count * self.pixels, self.C)
        out["segm_N"] = self.count
        if return_records:
            r = rec.cpu()
            out["segm_ce"] = r[:, 0].contiguous().view(torch.float64).numpy().copy()
            out["segm_counts"] = r[:, 1:].numpy().copy()
        return out


def summarize(ce_sum: float, counts, pixels: int, C: int = NUM_CLASSES) -> Dict[str, object]:
    """The summary of finish() from the totals: counts = [correct, then per class intersection, predicted, ground truth]."""
    counts = np.asarray(counts, np.float64).reshape(-1)
    cls = counts[1:1 + 3 * C].reshape(C, 3)
    union = cls[:, 1] + cls[:, 2] - cls[:, 0]
    iou = np.full(C, np.nan)
    np.divide(cls[:, 0], union, out=iou, where=union > 0)
    fg = iou[1:]
    return {"val_segm_ce": float(ce_sum) / pixels, "val_segm_pixel_acc": float(counts[0]) / pixels, "val_segm_iou": iou,
            "val_segm_miou": float(np.nanmean(iou)) if np.any(union > 0) else float("nan"),
            "val_segm_miou_fg": float(np.nanmean(fg)) if np.any(union[1:] > 0) else float("nan")}


def report_lines(res: Dict[str, object]):
    return [f"Segm CE: {res['val_segm_ce']}", f"Segm pixel acc: {res['val_segm_pixel_acc']}",
            f"Segm mIoU: {res['val_segm_miou']} (without background {res['val_segm_miou_fg']}, crops {res['segm_N']})"]


# ---- evaluation (eval.py --segm) ----------------------------------------------------------------------------------------------------
def check_eval_inputs(backbone: str, dataset_files) -> None:
    """eval.py --segm: PARE variants only, and the dataset needs pose, shape and part.  Raises ValueError with the message."""
    if "pare" not in backbone:
        raise ValueError(f"--segm scores PARE's part segmentation head: the {backbone} model has none")
    missing = [k for k in SEGM_DATASET_KEYS if k not in set(dataset_files)]
    if missing:
        raise ValueError(f"--segm needs {missing} in the dataset (ground-truth SMPL parameters and the 24 2-D keypoints place the mesh "
                         "in the crop)")


class SegmEval:
    """The per-batch step of eval.py --segm behind a forward with want_segm=True, on the current stream:
    ground-truth joints -> gt_cam_t (trainer.py:236-243) -> labels (:251-262) -> score."""

    def __init__(self, model, mesh: PartMesh, capacity: int, res: int = 224, focal: float = FOCAL_LENGTH):
        self.model, self.mesh, self.res, self.focal = model, mesh, int(res), float(focal)
        self.acc = SegmAccumulator(capacity, NUM_CLASSES, model.device)
        self.last_labels = None

    def step(self, out: Dict[str, torch.Tensor], gt_verts: torch.Tensor, gt_joints49: torch.Tensor, part_crop) -> None:
        """gt_verts [B,V,3] / gt_joints49 [B,49,3] from smpl_lbs of the ground truth, part_crop [B,24,3] = crop_keypoints24."""
        if "pred_segm_mask" not in out:
            raise PocoHipError("SegmEval.step: the forward was not asked for pred_segm_mask (want_segm=True)")
        k2d = _dev_f32(part_crop, self.model.device)
        cam_t = ops.estimate_translation(gt_joints49[:, 25:49].contiguous(), k2d, self.focal, self.res)
        self.last_labels = part_labels(gt_verts, cam_t, self.mesh, self.focal, self.res)
        self.acc.step(out["pred_segm_mask"], self.last_labels)

    def finish(self, save_results: bool = False) -> Dict[str, object]:
        return self.acc.finish(return_records=save_results)


@torch.no_grad()
def run_eval(model, dataset, dataset_path: str, J_regressor, smpl_path: str, part_mapping: Optional[str] = None, batch_size: int = 64,
             kinematic: bool = True, save_results: bool = False, likelihood: bool = False, uncert_threshold: Optional[float] = None,
             res: int = 224, return_labels: bool = False, visibility=None) -> Dict[str, object]:
    """eval.py --segm: evaluate.run_eval's loop (trainer.py:298-336) with the forward asked for pred_segm_mask and, behind the
    metrics of every batch on the same stream, the segmentation step.  dataset: the evaluate.EvalDataset of dataset_path (SMPL
    ground truth); its `part` rows are read here, restricted like the dataset's own rows.  Returns run_eval's result plus
    SegmAccumulator.finish() and `segm_summary` = [CE, pixel accuracy, mIoU, mIoU without background]; with save_results the
    per-crop records `segm_ce` / `segm_counts`; with return_labels `segm_labels` uint8 [N,res,res] (tests).  visibility: as
    evaluate.run_eval's (eval.py --visibility --segm)."""
    from . import evaluate
    if dataset.gt_form != "smpl" or dataset.shape is None:
        raise ValueError("--segm needs SMPL ground truth (`pose` and `shape`) in the dataset")
    with np.load(dataset_path, allow_pickle=False) as z:
        check_eval_inputs("pare", z.files)
        rows = evaluate.select_confident(z, uncert_threshold, dataset_path) if uncert_threshold is not None else z
        # crop='dataset' (DESIGN.md section 22): j2d_processing with the samples' rotation, flip and scale, so that the mesh lands on
        # the perturbed crop
        part = dataset.part_keypoints(rows["part"]) if getattr(dataset, "crop", "demo") == "dataset" \
            else crop_keypoints24(rows["part"], dataset.center, dataset.scale, res)
    if part.shape[0] != len(dataset):
        raise ValueError(f"`part` has {part.shape[0]} rows, the dataset {len(dataset)}")
    with np.load(smpl_path) as z:
        mesh = PartMesh.from_smpl({k: z[k] for k in ("faces", "lbs_weights") if k in z.files}, model.device, part_mapping)
    dev = model.device
    ev = evaluate.Evaluator(J_regressor, evaluate.joint_map(dataset.name), capacity=len(dataset), kinematic=kinematic, device=dev)
    lk = evaluate.LikelihoodAccumulator(model, capacity=len(dataset)) if likelihood else None
    sg = SegmEval(model, mesh, len(dataset), res)
    labels = []
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    for lo in range(0, len(dataset), batch_size):
        hi = min(lo + batch_size, len(dataset))
        out = model(dataset.batch(lo, hi, dev), want_segm=True)
        gt_pose = t(dataset.pose[lo:hi])
        if lk is not None:
            lk.step(out, gt_pose)
        gt_verts, gt_j49 = model.smpl_lbs(t(dataset.shape[lo:hi]), ops.rodrigues(gt_pose))
        ev.step(out, gt_pose, gt_vertices=gt_verts)
        sg.step(out, gt_verts, gt_j49, part[lo:hi])
        if visibility is not None:
            visibility.step(lo, hi, gt_verts, gt_j49, dataset.last_occ_mask)
        if return_labels:
            labels.append(sg.last_labels)
    out = ev.finish(save_results=save_results)
    if lk is not None:
        out.update(ev.uncert_summary())
        out.update(lk.finish())
    out.update(sg.finish(save_results))
    if visibility is not None:
        out.update(visibility.finish(out["corr_x"], out["corr_y"]))
    model.check_status()
    out["segm_summary"] = np.array([out["val_segm_ce"], out["val_segm_pixel_acc"], out["val_segm_miou"], out["val_segm_miou_fg"]], np.float64)
    out["imgname"] = np.asarray(dataset.imgname)
    if return_labels:
        out["segm_labels"] = torch.cat(labels).cpu().numpy()
    ev.close()
    return out


# ---- pictures (demo.py --save_segm) --------------------------------------------------------------------------------------------------
def palette() -> np.ndarray:
    """uint8 [25,3]: black for the background, then 24 fixed, well separated colours (hue steps of the golden angle)."""
    import colorsys
    pal = np.zeros((NUM_CLASSES, 3), np.uint8)
    for p in range(NUM_PARTS):
        hue = (p * 0.6180339887498949) % 1.0
        r, g, b = colorsys.hsv_to_rgb(hue, 0.65 + 0.35 * ((p % 3) / 2.0), 1.0 - 0.25 * ((p // 3) % 2))
        pal[p + 1] = [int(round(255 * r)), int(round(255 * g)), int(round(255 * b))]
    return pal


def colorize(labels: torch.Tensor, pal: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels uint8 [..., H, W] on the device -> uint8 [..., H, W, 3]: a device gather from the palette."""
    if pal is None:
        pal = torch.from_numpy(palette()).to(labels.device)
    return pal[labels.to(torch.int64).clamp_(max=pal.shape[0] - 1)]


def blend_half(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The 50/50 blend of two uint8 pictures, rounded half up: (a + b + 1) >> 1."""
    return ((a.to(torch.int16) + b.to(torch.int16) + 1) >> 1).to(torch.uint8)


def segm_picture(crop_u8: torch.Tensor, logits: torch.Tensor, mesh_labels: torch.Tensor) -> torch.Tensor:
    """uint8 [res, 2 res, 3]: the crop blended with the coloured argmax of the upsampled logits [C,h,w], and beside it the crop blended
    with the colours of mesh_labels [res,res]."""
    res = int(crop_u8.shape[0])
    pred = ops.segm_argmax(logits[None].contiguous(), res, res)[0]
    pal = torch.from_numpy(palette()).to(crop_u8.device)
    return torch.cat([blend_half(crop_u8, colorize(pred, pal)), blend_half(crop_u8, colorize(mesh_labels, pal))], dim=1).contiguous()


def check_demo_inputs(args, backbone: str) -> None:
    """demo.py --save_segm: folder mode, PARE only, and a body-model file with triangles.  Raises ValueError with the message."""
    if args.mode not in ("folder", "directory"):
        raise ValueError("--save_segm writes one picture per detection of folder mode: it needs --mode folder")
    if "pare" not in backbone:
        raise ValueError(f"--save_segm shows PARE's part segmentation head: the {backbone} model has none")
    if not (isinstance(args.smpl, str) and os.path.isfile(args.smpl)):
        raise ValueError(f"--save_segm: body-model file not found: {args.smpl}")
    with np.load(args.smpl) as z:
        if "faces" not in z.files:
            raise ValueError(f"--save_segm: {args.smpl} has no `faces` array (convert the SMPL .pkl with tools/convert_smpl.py, which "
                             "keeps its triangles)")


@torch.no_grad()
def write_segm_pictures(tester, image_folder: str, detections, out_dir: str, bbox_scale: float = 1.0) -> int:
    """demo.py --save_segm: <out_dir>/segm/<image>_<det>.png for every detection of every image the folder run regresses, through
    the tester's PNG writers (--encode gpu compresses on the device).  The crops go through the engine once more, with
    want_segm=True; the labels come from the predicted mesh at pred_cam_t.  Returns the number of pictures."""
    from PIL import Image
    from .tester import IMG_EXT, _write_bytes, _write_png
    res = int(tester.model_cfg.DATASET.IMG_RES)
    with np.load(tester.args.smpl) as z:
        mesh = PartMesh.from_smpl({k: z[k] for k in ("faces", "lbs_weights")}, tester.device, getattr(tester.args, "part_mapping", None))
    seg_dir = os.path.join(out_dir, "segm")
    os.makedirs(seg_dir, exist_ok=True)
    names = sorted(x for x in os.listdir(image_folder) if x.lower().endswith(IMG_EXT))
    skip = max(int(getattr(tester.args, "skip_frame", 1) or 1), 1)
    bs = tester.model.max_batch
    n = 0
    for pos in range(0, len(names), skip):
        name = names[pos]
        img = np.asarray(Image.open(os.path.join(image_folder, name)).convert("RGB"))
        d = detections.get(name) if isinstance(detections, dict) else (
            detections[pos] if detections is not None and pos < len(detections) else None)
        if d is None or len(d) == 0:
            s = float(min(img.shape[:2]))
            d = [[img.shape[1] / 2.0, img.shape[0] / 2.0, s, s]]
        d = np.asarray(d).reshape(-1, 4)
        d = d if d.dtype in (np.float32, np.float64) else d.astype(np.float32)
        fr = tester.to_device(img)
        for lo in range(0, len(d), bs):
            out = tester.model(tester.make_batch(fr, d[lo:lo + bs], bbox_scale), want_segm=True)
            labels = part_labels(out["smpl_vertices"], out["pred_cam_t"], mesh, FOCAL_LENGTH, res)
            for k in range(labels.shape[0]):
                pic = segm_picture(tester.crop_canvas(fr, d[lo + k], bbox_scale), out["pred_segm_mask"][k], labels[k])
                stem = os.path.join(seg_dir, f"{os.path.splitext(name)[0]}_{lo + k}")
                if tester.encode_on_gpu:
                    _write_bytes(stem + ".png", tester.encode_png(pic))
                else:
                    _write_png(stem + ".png", pic.cpu().numpy())
                n += 1
    tester.model.check_status()
    return n
