"""POCOTester for the MI355X engine: batch assembly + post-processing of
pocolib/core/tester.py:153-245 (folder mode) and :362-479 (per-track video mode), without the
third-party detector / tracker (out of scope: SURVEY.md 2 rows 2,27).  Detections are an
input: {image name: [[cx, cy, w, h], ...]} (what multi_person_tracker hands to the reference).  With --render the
uncertainty-coloured meshes are drawn on the GPU (poco_amd/render.py; tester.py:248-345 and :482-580).

Per image the crops are produced on the GPU (poco_crop_normalize) from the decoded frame, so the
reference's per-detection cv2.warpAffine + per-crop H2D copy (tester.py:182-203) disappears."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from typing import Dict, List, Optional

import numpy as np
import torch

from . import postproc
from ._lib import check, lib
from .config import model_kwargs, update_hparams
from .model import POCO

IMG_EXT = (".png", ".jpg", ".jpeg")


def calculate_focal_length(img_h, img_w):
    return float((img_w ** 2 + img_h ** 2) ** 0.5)          # image_utils.py:171-172


def calculate_bbox_info(center, scale, orig_shape):
    img_h, img_w = orig_shape
    f = calculate_focal_length(img_h, img_w)
    info = np.array([center[0] - img_w / 2.0, center[1] - img_h / 2.0, scale * 200.0])
    info[:2] = info[:2] / f * 2.8
    info[2] = (info[2] - 0.24 * f) / (0.06 * f)
    return info.astype(np.float32)                            # image_utils.py:174-187


def crop_normalize(frame_u8: torch.Tensor, boxes: torch.Tensor, bbox_scale: float = 1.0, res: int = 224,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frame uint8 [H,W,3] RGB cuda, boxes [N,4] (cx,cy,w,h) cuda float32 or float64 -> [N,3,res,res] fp32: the normalised
    crop of get_single_image_crop_demo (vibe_image_utils.py:233-266), byte-exact with cv2's fixed-point warpAffine.
    out: a contiguous float32 [N,3,res,res] tensor on the frame's device to write into (made here if not given).
    A ValueError, before any GPU work: a frame that is not a contiguous uint8 CUDA [H,W,3]; boxes that are not a contiguous
    float32 / float64 [N,4] tensor on the frame's device with N >= 1; res < 1; an `out` of another form."""
    if not (torch.is_tensor(frame_u8) and frame_u8.is_cuda and frame_u8.dtype == torch.uint8 and frame_u8.dim() == 3
            and frame_u8.shape[2] == 3 and frame_u8.is_contiguous()):
        raise ValueError("crop_normalize: the frame must be a contiguous uint8 CUDA tensor [H,W,3]")
    if not (torch.is_tensor(boxes) and boxes.is_cuda and boxes.device == frame_u8.device and boxes.dtype in (torch.float32, torch.float64)
            and boxes.dim() == 2 and boxes.shape[1] == 4 and boxes.shape[0] >= 1 and boxes.is_contiguous()):
        raise ValueError("crop_normalize: boxes must be a contiguous float32 or float64 [N,4] tensor on the frame's device, N >= 1")
    if isinstance(res, bool) or not isinstance(res, (int, np.integer)) or res < 1:
        raise ValueError(f"crop_normalize: res must be an integer >= 1, got {res!r}")
    res = int(res)
    H, W, _ = frame_u8.shape
    N = boxes.shape[0]
    if out is None:
        out = torch.empty(N, 3, res, res, device=frame_u8.device, dtype=torch.float32)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == frame_u8.device and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (N, 3, res, res)):
        raise ValueError(f"crop_normalize: out must be a contiguous float32 [{N},3,{res},{res}] tensor on the frame's device")
    L = lib()
    fn = L.poco_crop_normalize if boxes.dtype == torch.float32 else L.poco_crop_normalize_f64
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    with torch.cuda.device(frame_u8.device):
        check(fn(frame_u8.data_ptr(), H, W, boxes.data_ptr(), N, float(bbox_scale), res, out.data_ptr(),
                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "poco_crop_normalize")
    return out


# outputs of a forward that postprocess() never reads: they stay on the device (uncert_feat alone is 2048-3072 floats per crop)
DEVICE_ONLY_KEYS = ("uncert_feat", "body_feat2", "pred_pose6d", "pred_pose_6d", "pred_cam_t", "pred_fullimg_cam_t", "record",
                    "pred_segm_mask", "backbone_feat")


def crop_keypoints(joints2d, box, res: int = 224, bbox_scale: float = 1.0) -> np.ndarray:
    """Original-image keypoints [K, >= 2] in the pixel coordinates of the crop of `box` = (cx, cy, w, h): where the crop's affine
    map (gen_trans_from_patch_cv, vibe_image_utils.py:58-92) puts them, x_c = res / 2 + (x - cx) res / (w scale), y_c = res / 2 +
    (y - cy) res / (h scale); computed in float64, returned as float32 [K,2]."""
    j = np.asarray(joints2d, np.float64)[:, :2]
    cx, cy, bw, bh = (float(v) for v in np.asarray(box, np.float64).reshape(4))
    out = np.empty((j.shape[0], 2), np.float64)
    out[:, 0] = res / 2.0 + (j[:, 0] - cx) * (res / (bw * bbox_scale))
    out[:, 1] = res / 2.0 + (j[:, 1] - cy) * (res / (bh * bbox_scale))
    return out.astype(np.float32)


class POCOTester:
    _pseudo = None                      # --save_dataset: the device-side labeler of the current run (pseudo_begin), else None
    pair = None                         # --cfg2 / --ckpt2: the RegressorPair that stands where self.model is used for forwards, else None
    tta = None                          # --tta: the TTAModel that stands where self.model is used for forwards, else None
    corrupt = None                      # eval.py --corrupt: the CorruptModel around self.model (which stays the engine), else None

    def __init__(self, args):
        self.args = args
        self.model_cfg = update_hparams(args.cfg)
        # demo.py:305 passes store_false: default True = kinematic post-processing on
        self.model_cfg.POCO.KINEMATIC_UNCERT = getattr(args, "no_kinematic_uncert", True)
        self.backbone = self.model_cfg.POCO.BACKBONE
        # one process per GPU (demo.py --gpus N): LOCAL_RANK picks the device; ranks beyond the visible devices
        # (gloo smoke runs on a smaller box) share them round-robin
        ndev = max(torch.cuda.device_count(), 1)
        self.device = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0')) % ndev}")
        torch.cuda.set_device(self.device)
        views = None
        if getattr(args, "tta", None):
            from . import tta
            views = tta.parse_views(args.tta)
        levels = None
        if getattr(args, "corrupt", None):
            from . import corrupt
            levels = corrupt.parse_levels(args.corrupt)
        # --tta / --corrupt: a forward takes the K views (levels) of max(1, batch_size // K) crops, so the engine holds at least the K of one crop
        self.model = self._build_engine(self.model_cfg, args.ckpt, getattr(args, "inf_model", "best"),
                                        min_batch=len(views) if views else (len(levels) if levels else 1))
        if levels:
            self.corrupt = corrupt.CorruptModel(self.model, levels, int(getattr(args, "corrupt_seed", None) or 0))
        if views:
            self.model = self.tta = tta.TTAModel(self.model, views, getattr(args, "tta_weight", None) or "uncert")
            self.tta_text = tta.views_text(views)
        if getattr(args, "cfg2", None):
            from .select import RegressorPair
            cfg2 = update_hparams(args.cfg2)
            if cfg2.DATASET.IMG_RES != self.model_cfg.DATASET.IMG_RES:
                raise ValueError(f"--cfg2: DATASET.IMG_RES {cfg2.DATASET.IMG_RES} differs from --cfg's {self.model_cfg.DATASET.IMG_RES}")
            # POCO.KINEMATIC_UNCERT is neither config's: --no_kinematic_uncert decides it (above), for both models alike
            second = self._build_engine(cfg2, args.ckpt2, getattr(args, "inf_model2", "best"))
            self.model = self.pair = RegressorPair(self.model, second, mode=getattr(args, "select", None) or "crop",
                                                   scale=float(getattr(args, "select_scale", None) or 1.0),
                                                   kinematic=self.model_cfg.POCO.KINEMATIC_UNCERT)
            self._select_rows = []              # the `select` of every batch, for the printed line
            self._select_mixed = 0
        self.faces = None                       # triangle list for --save_obj / --render, if the body-model file carries one
        if isinstance(args.smpl, str) and os.path.isfile(args.smpl):
            with np.load(args.smpl) as z:
                if "faces" in z.files:
                    self.faces = np.asarray(z["faces"], np.int64)
        self.calibration = None                 # --calibration FILE: the final var -> err_pose, err_mpjpe, err_pampjpe, err_v2v
        if getattr(args, "calibration", None):
            from .calibrate import Calibration
            self.calibration = Calibration(args.calibration, self.device, bool(self.model_cfg.POCO.KINEMATIC_UNCERT), str(self.backbone))
        self._renderer = None
        self._refit_tables = None               # --kp_refit: (Jt, Jd, parents) of the body-model file, made at first use
        self._pseudo_src = []                   # --save_dataset: the label of every crop offered to the labeler

    def _build_engine(self, model_cfg, ckpt, inf_model, min_batch: int = 1):
        """One finalized engine for a config and a checkpoint, with this tester's --smpl, batch size and device."""
        return POCO(**model_kwargs(model_cfg), pretrained=ckpt, inf_model=inf_model, max_batch=max(int(self.args.batch_size), min_batch),
                    smpl=self.args.smpl, device=str(self.device),
                    keep_state_dict=False).finalize()     # (state_dict() re-reads the checkpoint file on demand)

    # ---- --cfg2 / --ckpt2 -------------------------------------------------------------------------------------------
    def _select_note(self, out) -> None:
        """Keep a forward's choices for the printed line (host copies of [B,24] and [B] bytes)."""
        self._select_rows.append(np.asarray(out["select"].cpu().numpy() if torch.is_tensor(out["select"]) else out["select"]))
        self._select_mixed += int(np.asarray(out["select_mixed"].cpu().numpy() if torch.is_tensor(out["select_mixed"])
                                             else out["select_mixed"]).sum())

    def select_summary(self) -> None:
        """Print the one line of a run with a second model and forget its counts."""
        if self.pair is None or not self._select_rows:
            return
        from .select import summary_line
        print(summary_line(np.concatenate(self._select_rows), self._select_mixed, self.pair.mode))
        self._select_rows, self._select_mixed = [], 0

    # ---- --save_dataset ---------------------------------------------------------------------------------------------
    def pseudo_begin(self, capacity: int) -> None:
        """--save_dataset: a PseudoLabeler (poco_amd/pseudo.py) for the `capacity` crops this run will regress; every forward
        of iter_frame_results / run_on_video then offers its device outputs to it."""
        if not getattr(self.args, "save_dataset", None):
            return
        from .pseudo import PseudoLabeler
        self._pseudo = PseudoLabeler(max(int(capacity), 1), getattr(self.args, "uncert_threshold", None), self.backbone,
                                     self.model_cfg.DATASET.IMG_RES, self.device)
        self._pseudo_src = []

    def _pseudo_offer(self, out, boxes: np.ndarray, labels) -> None:
        """One batch behind its forward, on the same stream: nothing is read back.  labels: one per crop, kept on the host and
        found again through the crop's source_id = its position among the offered crops."""
        base = len(self._pseudo_src)
        self._pseudo_src.extend(labels)
        self._pseudo.step(out, np.ascontiguousarray(boxes, np.float32).reshape(-1, 4), np.arange(base, base + len(labels), dtype=np.int32))

    def pseudo_finish(self, imgname_of, person_of) -> dict:
        """Write --save_dataset from the kept records; imgname_of / person_of map a label to the file's imgname / person_id.
        Returns the counters of the printed JSON line."""
        pl, self._pseudo = self._pseudo, None
        if pl is None:
            return {}
        from .pseudo import write_dataset
        arrays = pl.finish(imgname=[imgname_of(x) for x in self._pseudo_src], person_id=[person_of(x) for x in self._pseudo_src])
        pl.close()
        write_dataset(self.args.save_dataset, arrays)
        thr = getattr(self.args, "uncert_threshold", None)
        return {"dataset_offered": arrays["offered"], "dataset_kept": arrays["kept"],
                "dataset_threshold": None if thr is None else float(thr)}

    # ---- --render ---------------------------------------------------------------------------------------------------
    @property
    def render_on(self) -> bool:
        """--render is opt-in; --no_render wins (demo.py render_enabled)."""
        return bool(getattr(self.args, "render", False)) and not getattr(self.args, "no_render", False)

    def render_frame(self, frame: torch.Tensor, verts, orig_cam, var, side_bg: int, keypoints=None) -> torch.Tensor:
        """The picture of one frame: people (in painter's order) drawn over the device frame `frame` (in place), with
        --sideview the Ry(270) view on a canvas of value side_bg to its right; --no_uncert_color = plain grey; --wireframe =
        both views as wireframes.  keypoints (--draw_keypoints): per person (points, rgb), stamped on the main view after that
        person's mesh."""
        from . import render
        if self.faces is None:
            raise RuntimeError(f"--render: {self.args.smpl} has no `faces` array")
        V = int(np.asarray(verts).shape[-2])
        if self._renderer is None or self._renderer.V != V:
            self._renderer = render.Renderer(self.faces, V, self.device)
        return render.render_people(self._renderer, frame, verts, orig_cam, var, self.backbone,
                                    uncert_color=not getattr(self.args, "no_uncert_color", False),
                                    sideview=bool(getattr(self.args, "sideview", False)), side_bg=side_bg,
                                    wireframe=bool(getattr(self.args, "wireframe", False)), keypoints=keypoints)

    @property
    def draw_keypoints(self) -> bool:
        return bool(getattr(self.args, "draw_keypoints", False))

    def crop_canvas(self, frame_u8: torch.Tensor, box, bbox_scale: float = 1.0) -> torch.Tensor:
        """--render_crop: the uint8 [res,res,3] crop of one detection, the bytes cv2.warpAffine cuts before ToTensor / Normalize
        (`raw_img` of get_single_image_crop_demo, tester.py:184-190,257).  The crop kernel hands out the normalised floats
        (x = (p / 255 - mean) / std); p is recovered exactly by inverting that and rounding.  This relies on the crop output
        being float32 (the float error is then below 1e-3 of a level; a half-precision output would not round back) and on the
        mean / std constants below being the kernel's."""
        res = self.model_cfg.DATASET.IMG_RES
        raw = np.asarray(box)
        b = torch.from_numpy(np.ascontiguousarray(raw.reshape(1, 4), np.float64 if raw.dtype == np.float64 else np.float32)).to(self.device)
        x = crop_normalize(frame_u8, b, bbox_scale, res)[0]
        assert x.dtype == torch.float32
        mean = torch.tensor([0.485, 0.456, 0.406], device=self.device).view(3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225], device=self.device).view(3, 1, 1)
        return ((x * std + mean) * 255.0).round_().clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()

    def render_crop_frame(self, frame_u8: torch.Tensor, r: dict, box, bbox_scale: float = 1.0) -> torch.Tensor:
        """--render_crop (folder mode, tester.py:256-285): the FIRST detection of the image on its own 224 x 224 crop, camera
        (s, s, tx, ty) of that crop's pred_cam; keypoints in crop pixel coordinates (crop_keypoints)."""
        from . import render
        s, tx, ty = (float(c) for c in r["pred_cam"][0][:3])
        kp = None
        if self.draw_keypoints:
            j = crop_keypoints(r["smpl_joints2d"][0], box, self.model_cfg.DATASET.IMG_RES, bbox_scale)
            kp = [render.folder_keypoints(j)]
        return self.render_frame(self.crop_canvas(frame_u8, box, bbox_scale), r["verts"][:1], np.array([[s, s, tx, ty]], np.float32),
                                 r["var"][:1], side_bg=255, keypoints=kp)

    # ---- --occlusion_map ---------------------------------------------------------------------------------------------------
    @property
    def occlusion_on(self) -> bool:
        return bool(getattr(self.args, "occlusion_map", False))

    def occlusion_maps(self, frame_u8: torch.Tensor, dets: np.ndarray, bbox_scale: float = 1.0):
        """--occlusion_map: per detection of one frame, (picture, arrays) - the heat map of --occ_metric over the detection's own
        crop (a device uint8 [res,res,3]) and what <image>_<det>.npz holds.  One OcclusionSweep per detection (poco_amd/
        occlusion.py): full batches of occluded copies through the engine, the records and the picture made on the device; only the
        [n,77] records, the positions and the baseline's var_pose / pred_cam are copied to the host."""
        from . import occlusion
        a = self.args
        if getattr(self, "_occ", None) is None:
            fill = (0.0, 0.0, 0.0) if getattr(a, "occ_fill", None) is None else occlusion.fill_from_grey(a.occ_fill)
            self._occ = occlusion.OcclusionSweep(self.model, getattr(a, "occ_patch", 40), getattr(a, "occ_stride", 10), fill)
        scale = getattr(a, "occ_scale", "auto")
        scale = scale if scale == "auto" else float(scale)
        raw = np.asarray(dets)
        for i in range(len(raw)):
            res = self._occ.run(self.make_batch(frame_u8, raw[i:i + 1], bbox_scale))
            field = occlusion.field_of(res.records, getattr(a, "occ_metric", "v2v"))
            pic = occlusion.heat_overlay(field, res.positions, res.patch, self.crop_canvas(frame_u8, raw[i], bbox_scale), scale)
            nh, nw = res.grid
            yield pic, {"records": res.records.cpu().numpy().reshape(nh, nw, occlusion.REC), "positions": res.positions.cpu().numpy(),
                        "patch": np.int32(res.patch), "stride": np.int32(res.stride),
                        "var_pose": res.baseline["var_pose"][0].cpu().numpy(), "pred_cam": res.baseline["pred_cam"][0].cpu().numpy()}

    # ---- --image_format jpg / --save_video ------------------------------------------------------------------------------
    @property
    def image_format(self) -> str:
        return getattr(self.args, "image_format", "png") or "png"

    def encode_jpeg(self, pic: torch.Tensor) -> bytes:
        """The .jpg bytes of a device picture, encoded on the device (poco_amd/jpeg.py): only the bytes cross to the host.  The
        encoder is created for the first picture's size and re-created when a larger one arrives (folder mode)."""
        from .jpeg import JpegEncoder
        H, W = int(pic.shape[0]), int(pic.shape[1])
        enc = getattr(self, "_jpeg", None)
        if enc is None or H > enc.max_h or W > enc.max_w:
            self._jpeg = enc = JpegEncoder(self.device, max(H, enc.max_h if enc else 0), max(W, enc.max_w if enc else 0))
        return enc.encode(pic.contiguous(), int(getattr(self.args, "jpeg_quality", 90)))

    # ---- --encode gpu --------------------------------------------------------------------------------------------------------
    @property
    def encode_on_gpu(self) -> bool:
        return getattr(self.args, "encode", "host") == "gpu"

    def encode_png(self, pic: torch.Tensor) -> bytes:
        """The .png bytes of a device picture, filtered and deflated on the device (poco_amd/png.py): only the bytes cross to the
        host.  The encoder is created for the first picture's size and re-created when a larger one arrives."""
        from .png import PngEncoder
        H, W = int(pic.shape[0]), int(pic.shape[1])
        enc = getattr(self, "_png", None)
        if enc is None or H > enc.max_h or W > enc.max_w:
            old = (enc.max_h, enc.max_w) if enc else (0, 0)
            if enc is not None:
                enc.close()
            self._png = enc = PngEncoder(self.device, max(H, old[0]), max(W, old[1]))
        return enc.encode(pic.contiguous())

    # ---- --decode gpu / --decode_png gpu -----------------------------------------------------------------------------------
    @property
    def decode_on_gpu(self) -> bool:
        return getattr(self.args, "decode", "host") == "gpu"

    @property
    def decode_png_on_gpu(self) -> bool:
        return getattr(self.args, "decode_png", "host") == "gpu"

    @property
    def decode_progressive_on_gpu(self) -> bool:
        return getattr(self.args, "decode_progressive", "host") == "gpu"

    @property
    def decode_any_on_gpu(self) -> bool:
        return self.decode_on_gpu or self.decode_png_on_gpu or self.decode_progressive_on_gpu

    def to_device(self, frame) -> torch.Tensor:
        """A frame as a uint8 [H,W,3] device tensor: decoded there already (--decode gpu, --decode_png gpu, --decode_progressive
        gpu) or uploaded."""
        return frame if torch.is_tensor(frame) else torch.from_numpy(np.ascontiguousarray(frame)).to(self.device)

    def _device_decode(self, named, out, infos, attr, cls, flag, nbytes_of):
        """One device call per batch of at most max_batch parsed files of one format: out[i] becomes a device tensor where the
        status word is 0; a damaged file is named in one warning and left to PIL.  The decoder (self.<attr>) is created for the
        first batch's sizes and re-created when a larger one arrives."""
        import warnings
        idx = [i for i, f in enumerate(infos) if f is not None]
        for lo in range(0, len(idx), max(1, self.model.max_batch)):
            part = idx[lo:lo + max(1, self.model.max_batch)]
            H, W = max(infos[i].height for i in part), max(infos[i].width for i in part)
            nbytes = sum(nbytes_of(infos[i]) + 32 for i in part)
            dec = getattr(self, attr, None)
            if dec is None or H > dec.max_h or W > dec.max_w or len(part) > dec.max_batch or nbytes > dec.max_bytes:
                old = (dec.max_h, dec.max_w, dec.max_bytes) if dec else (0, 0, 0)
                if dec is not None:
                    dec.close()
                dec = cls(self.device, max(H, old[0]), max(W, old[1]), max(1, self.model.max_batch), max(2 * nbytes, old[2], 1 << 20))
                setattr(self, attr, dec)
            tensors, status = dec.decode([infos[i] for i in part], return_status=True)
            for i, t, st in zip(part, tensors, status):
                if st == 0:
                    out[i] = t
                else:
                    warnings.warn(f"{flag}: {named[i][0]} is damaged (status {st}); decoding it with PIL")

    def decode_frames(self, named) -> list:
        """named: [(name, the bytes of an image file)] -> the frames in order, routed by signature: with --decode gpu all baseline
        JPEGs of the list are decoded in ONE device call, with --decode_png gpu all PNGs parse_png accepts in another (uint8
        [H,W,3] device tensors, PIL's pixels), with --decode_progressive gpu all progressive JPEGs parse_progressive_jpeg accepts
        in a third.  A file the parser declines (progressive JPEG without its flag, 16-bit or interlaced PNG ...), a
        format whose flag is not set and an image whose status word comes back non-zero go through PIL (host arrays); the
        latter is named in one warning, and so is a JPEG with more restart intervals than a decoder plans per image.  Any error
        of a decode call is raised.  The decoders are created for the first batch's sizes and re-created when a larger one
        arrives."""
        import io
        import warnings
        from PIL import Image
        out = [None] * len(named)
        if self.decode_on_gpu:
            from .jpeg import SEGS_PER_IMAGE, JpegDecoder, parse_jpeg
            infos = [parse_jpeg(b) if b[:2] == b"\xff\xd8" else None for _, b in named]
            many = [i for i, f in enumerate(infos) if f is not None and len(f.segments) > SEGS_PER_IMAGE]
            if many:                   # checked here, so that every error of the decode call below is a real one and is raised
                warnings.warn(f"--decode gpu: {', '.join(named[i][0] for i in many)}: more than {SEGS_PER_IMAGE} restart intervals, "
                              "which the device decoder does not plan for; decoding with PIL")
                for i in many:
                    infos[i] = None
            self._device_decode(named, out, infos, "_jdec", JpegDecoder, "--decode gpu", lambda f: f.scan_length)
        if self.decode_png_on_gpu:
            from .png import SIGNATURE, PngDecoder, parse_png
            infos = [parse_png(b) if b[:8] == SIGNATURE else None for _, b in named]
            self._device_decode(named, out, infos, "_pdec", PngDecoder, "--decode_png gpu", lambda f: f.stream_length)
        if self.decode_progressive_on_gpu:
            from .jpeg import TABLES_PER_IMAGE, ProgressiveJpegDecoder, _scan_tables, parse_progressive_jpeg
            infos = [parse_progressive_jpeg(b) if b[:2] == b"\xff\xd8" else None for _, b in named]
            many = [i for i, f in enumerate(infos) if f is not None and len(_scan_tables(f)[0]) > TABLES_PER_IMAGE]
            if many:
                warnings.warn(f"--decode_progressive gpu: {', '.join(named[i][0] for i in many)}: more than {TABLES_PER_IMAGE} Huffman "
                              "tables, which the device decoder does not plan for; decoding with PIL")
                for i in many:
                    infos[i] = None
            self._device_decode(named, out, infos, "_jpdec", ProgressiveJpegDecoder, "--decode_progressive gpu",
                                lambda f: f.stream_length)
        for i, (_, b) in enumerate(named):
            if out[i] is None:
                out[i] = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
        return out

    def _save_meshes(self, folder: str, verts: np.ndarray, names):
        from .postproc import write_obj
        for v, n in zip(verts, names):
            write_obj(os.path.join(folder, n + ".obj"), v, self.faces)

    # ---- one batch of detections of one frame ---------------------------------------------------
    def make_batch(self, frame_u8: torch.Tensor, dets: np.ndarray, bbox_scale: float = 1.0) -> Dict[str, torch.Tensor]:
        if self.tta is not None:            # --tta: the K views of every detection, view-major, cut with the dataset crop from its box
            from .tta import frame_batch
            return frame_batch(frame_u8, dets, self.tta.views, self.model_cfg.DATASET.IMG_RES)
        H, W = int(frame_u8.shape[0]), int(frame_u8.shape[1])
        raw = np.asarray(dets)
        # the crop follows the detections' own dtype (float64 tracks stay float64: cv2 sees float32(cx) etc. of THOSE values)
        boxes = torch.from_numpy(np.ascontiguousarray(raw.reshape(-1, 4), np.float64 if raw.dtype == np.float64 else np.float32)).to(self.device)
        dets = raw.astype(np.float32).reshape(-1, 4)
        centers = dets[:, :2]
        scales = np.maximum(dets[:, 2], dets[:, 3]) / 200.0                        # tester.py:196
        info = np.stack([calculate_bbox_info(c, s, (H, W)) for c, s in zip(centers, scales)])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)   # noqa: E731
        return {"img": crop_normalize(frame_u8, boxes, bbox_scale, self.model_cfg.DATASET.IMG_RES),
                "bbox_info": t(info), "focal_length": t(np.full(len(dets), calculate_focal_length(H, W))),
                "scale": t(scales), "center": t(centers), "orig_shape": t(np.tile([[H, W]], (len(dets), 1)))}

    def postprocess(self, output, dets: np.ndarray, W: int, H: int) -> Dict[str, np.ndarray]:
        dets = np.asarray(dets, dtype=np.float32).reshape(-1, 4)
        pred_cam = output["pred_cam"].cpu().numpy()
        res = {"pred_cam": pred_cam, "orig_cam": postproc.convert_crop_cam_to_orig_img(pred_cam, dets, W, H),
               "verts": output["smpl_vertices"].cpu().numpy(), "pose": output["pred_pose"].cpu().numpy(),
               "betas": output["pred_shape"].cpu().numpy(), "joints3d": output["smpl_joints3d"].cpu().numpy(),
               "bboxes": dets}
        j2d = output["smpl_joints2d"].cpu().numpy()
        if self.pair is not None:                                                    # the same two steps, per row by the root's model
            from . import select
            sel = output["select"].cpu().numpy()
            j2d = select.pair_joints2d(j2d, sel, self.pair.backbones, dets, self.model_cfg.DATASET.IMG_RES)
            res["smpl_joints2d"] = np.concatenate([j2d, np.ones((len(dets), 49, 1), np.float32)], -1)
            res["var"], res["var_global"] = select.pair_uncert(output["var_pose"], sel, self.pair.backbones,
                                                               self.model_cfg.POCO.KINEMATIC_UNCERT, clip=True)
            res["select"], res["select_score"] = sel, output["select_score"].cpu().numpy()
            return res
        if "tta_spread" in output:                                                   # --tta: the views' disagreement per joint
            res["tta_spread"] = output["tta_spread"].cpu().numpy()
        if "cliff" not in self.backbone:                                             # tester.py:225-230
            j2d = postproc.convert_crop_coords_to_orig_img(dets, j2d, self.model_cfg.DATASET.IMG_RES)
        res["smpl_joints2d"] = np.concatenate([j2d, np.ones((len(dets), 49, 1), np.float32)], -1)
        res["var"], res["var_global"] = postproc.folder_uncert(output["var_pose"], self.backbone,
                                                               self.model_cfg.POCO.KINEMATIC_UNCERT)   # tester.py:242-245
        if self.calibration is not None:
            res.update(self.calibration.apply(res["var"]))
        return res

    @torch.no_grad()
    def iter_frame_results(self, items, bbox_scale: float = 1.0, keep_frames: bool = False):
        """items: iterable of (frame uint8 [H,W,3] RGB, detections [n,4]); yields one result dict (or None for a frame without
        detections) per item, in order.  The reference runs one forward per image (pocolib/core/tester.py:168-213); crops are
        independent of each other, so here the crops of CONSECUTIVE frames share forwards of up to `batch_size` crops (a photo
        folder with one person per image would otherwise sit in the launch-bound B = 1 regime) and the
        rows are handed back per frame.  At most `batch_size` crops and their frames are held at a time.
        keep_frames (--render): yields (result, the frame's device copy or None) pairs instead, so the picture is drawn on the
        frame the crops were cut from."""
        from collections import deque
        bs = self.model.max_batch
        queue = deque()                    # frames in arrival order: {"dets", "W", "H", "parts", "todo"}
        pieces, batches = [], []           # crops waiting for a forward: (entry, lo, k) + their batch dicts
        npend = 0

        def flush():
            nonlocal npend
            if not pieces:
                return
            if self.tta is not None:           # view-major batches join per view
                from .tta import cat_view_batches
                batch = cat_view_batches(batches, self.tta.K)
            else:
                batch = batches[0] if len(batches) == 1 else {k: torch.cat([b[k] for b in batches], 0) for k in batches[0]}
            out = self.model(batch, want_segm=False)
            if self._pseudo is not None:       # --save_dataset: from the device outputs, before they are copied for the result files
                self._pseudo_offer(out, np.concatenate([e["dets"][lo:lo + k] for e, lo, k in pieces]),
                                   [(e["index"], lo + i) for e, lo, k in pieces for i in range(k)])
            # one D2H per tensor postprocess() reads (not uncert_feat / body_feat2 / pose6d / cam_t: MBs per batch that nothing
            # downstream uses), sliced per frame below
            out = {n: v.cpu() for n, v in out.items() if torch.is_tensor(v) and n not in DEVICE_ONLY_KEYS}
            self.model.check_status()          # (the copies above synchronised the stream) a timed-out in-kernel wait = invalid rows: raise, write nothing
            if self.pair is not None:
                self._select_note(out)
            off = 0
            for e, lo, k in pieces:
                sl = {n: (v[off:off + k] if torch.is_tensor(v) else v) for n, v in out.items()}
                e["parts"].append(self.postprocess(sl, e["dets"][lo:lo + k], e["W"], e["H"]))
                e["todo"] -= k
                off += k
            pieces.clear()
            batches.clear()
            npend = 0

        def drain():
            while queue and queue[0]["todo"] == 0:
                e = queue.popleft()
                res = None if not e["parts"] else {k: np.concatenate([p[k] for p in e["parts"]], 0) for k in e["parts"][0]}
                yield (res, e["frame"]) if keep_frames else res

        for index, (frame, dets) in enumerate(items):
            raw = np.asarray(dets)
            raw = raw.reshape(-1, 4) if raw.size else np.zeros((0, 4), np.float32)
            e = {"dets": raw, "W": frame.shape[1], "H": frame.shape[0], "parts": [], "todo": len(raw), "frame": None, "index": index}
            queue.append(e)
            if len(raw):
                fr = self.to_device(frame)
                if keep_frames:
                    e["frame"] = fr
                lo = 0
                while lo < len(raw):
                    k = min(bs - npend, len(raw) - lo)
                    batches.append(self.make_batch(fr, raw[lo:lo + k], bbox_scale))
                    pieces.append((e, lo, k))
                    npend += k
                    lo += k
                    if npend == bs:
                        flush()
            yield from drain()
        flush()
        yield from drain()

    def run_on_frames(self, frames, detections: List[np.ndarray], bbox_scale: float = 1.0):
        """frames: iterable of uint8 [H,W,3] RGB arrays; detections[i]: [n_i,4].  Returns the per-frame results."""
        return list(self.iter_frame_results(zip(frames, detections), bbox_scale))

    @torch.no_grad()
    def run_on_video(self, tracking_results: dict, frames, orig_width: int, orig_height: int, bbox_scale: float = 1.0,
                     raw: bool = False):
        """Per-track results like pocolib/core/tester.py:362-479.

        tracking_results: {person_id: {'bbox': [T,4] (cx,cy,w,h), 'frames': [T] frame indices}} - what
        multi_person_tracker hands to the reference (tester.py:113-151); a track may carry 'joints2d' [T,K,3], the pose
        tracker's keypoints its boxes were derived from (load_tracking), which are handed back in its result.  frames:
        sequence or callable frame index -> uint8 [H,W,3] RGB.

        The reference walks person by person and re-reads every frame for every person
        (dataset/inference.py:72-135).  Here the stream is frame-major: a frame is decoded and uploaded once,
        all people visible in it are cropped on the GPU, crops of consecutive frames are packed into full
        batches of `batch_size`, and the regressed rows are scattered back to the tracks.
        raw=True: return the un-post-processed per-frame network outputs per track (multi-GPU merge, see
        _merge_rank_results)."""
        get = frames if callable(frames) else (lambda i: frames[i])
        bs = self.model.max_batch
        # (frame, person, slot in that person's track), frame-major
        items = sorted((int(f), pid, k) for pid, tr in tracking_results.items() for k, f in enumerate(tr["frames"]))
        keys = ("pred_cam", "smpl_vertices", "pred_pose", "pred_shape", "smpl_joints3d", "smpl_joints2d", "var_pose")
        if self.pair is not None:
            keys += ("select", "select_score")
        store = {pid: {k: [None] * len(tr["frames"]) for k in keys} for pid, tr in tracking_results.items()}
        pend_batches, pend_meta, pend_dets = [], [], []

        def flush():
            if not pend_meta:
                return
            batch = {k: torch.cat([b[k] for b in pend_batches], 0) for k in pend_batches[0]}
            out = self.model(batch, want_segm=False)
            if self._pseudo is not None:       # --save_dataset: the regressor's raw outputs (smoothing comes later, per track)
                self._pseudo_offer(out, np.concatenate(pend_dets), list(pend_meta))
            host = {k: out[k].cpu().numpy() for k in keys}
            self.model.check_status()          # after the synchronising copies, before the rows are stored
            if self.pair is not None:
                self._select_note(out)
            for row, (pid, slot) in enumerate(pend_meta):
                for k in keys:
                    store[pid][k][slot] = host[k][row]
            pend_batches.clear()
            pend_meta.clear()
            pend_dets.clear()

        i = 0
        while i < len(items):
            f = items[i][0]
            j = i
            while j < len(items) and items[j][0] == f:
                j += 1
            fr = get(f)
            fr = fr if torch.is_tensor(fr) else torch.from_numpy(np.ascontiguousarray(fr)).to(self.device, non_blocking=True)
            group = items[i:j]
            while group:                     # a frame with more people than fit goes out in pieces
                room = bs - len(pend_meta)
                part, group = group[:room], group[room:]
                dets = np.stack([np.asarray(tracking_results[pid]["bbox"][slot]) for _, pid, slot in part])   # keeps the tracks' dtype
                pend_batches.append(self.make_batch(fr, dets, bbox_scale))
                pend_meta.extend((pid, slot) for _, pid, slot in part)
                pend_dets.append(dets.astype(np.float32).reshape(-1, 4))
                if len(pend_meta) == bs:
                    flush()
            i = j
        flush()

        stacked = {pid: {k: np.stack(v) for k, v in store[pid].items()} for pid in tracking_results}
        self.select_summary()
        if raw:
            return stacked
        if getattr(self.args, "track_stitch", False):
            tracking_results, stacked = self._stitch_tracks(tracking_results, stacked, frames, orig_width, orig_height, bbox_scale)
        lam = getattr(self.args, "smooth_uncert", None)
        if getattr(self.args, "kp_refit", None) is not None:
            return self._finish_tracks_refitted(tracking_results, stacked, orig_width, orig_height)
        if getattr(self.args, "infill", None) is not None:
            res = self._finish_tracks_infilled(tracking_results, stacked, orig_width, orig_height)
            return res if lam is None else self._smooth_tracks_uncert(res, lam)
        if lam is not None:
            return self._smooth_tracks_uncert({pid: self._finish_track(tr, stacked[pid], orig_width, orig_height, smooth=False)
                                               for pid, tr in tracking_results.items()}, lam)
        return {pid: self._finish_track(tr, stacked[pid], orig_width, orig_height) for pid, tr in tracking_results.items()}

    def _stitch_tracks(self, tracking_results: dict, stacked: dict, frames, orig_width: int, orig_height: int, bbox_scale: float):
        """--track_stitch: ONE call of stitch.stitch_tracks joins the fragments into chains by their regressed shape and the motion of
        their boxes; unless --stitch_no_fill, the frames of the holes between joined fragments get interpolated boxes and go through
        the forward; chains under 25 frames are dropped.  The finishing branches then see each chain as one long track whose
        uncertain rows sit in the middle: what --infill and --smooth_uncert were written for.  Every raw row gains `stitch` (0 an own
        row, 1 a gap row) and `stitch_frag` (the index of the source fragment in the chain, -1 on a gap row), which _finish_track
        hands on; the merged tracks are kept in self.stitched_tracking."""
        from . import stitch
        fill = not getattr(self.args, "stitch_no_fill", False)
        merged, st, chains = stitch.stitch_tracks(tracking_results, stacked, None, fill=fill, device=self.device,
                                                  **stitch.params_of(self.args))
        gap = stitch.gap_tracks(merged, chains)
        if gap:
            if hasattr(frames, "plan"):
                frames.plan(sorted({int(f) for v in gap.values() for f in v["frames"]}))
            st = stitch.merge_gap_rows(st, self.run_on_video(gap, frames, orig_width, orig_height, bbox_scale, raw=True), chains)
        merged, st, kept, dropped = stitch.drop_short(merged, st, chains)
        for ch in kept:
            st[ch["pid"]] = {**st[ch["pid"]], "stitch": ch["stitch"], "stitch_frag": ch["stitch_frag"]}
        print(stitch.summary_line(len(tracking_results), chains, dropped))
        self.stitched_tracking = merged
        return merged, st

    def _finish_tracks_refitted(self, tracking_results: dict, stacked: dict, orig_width: int, orig_height: int) -> dict:
        """--kp_refit LAMBDA: the tracks are finished unsmoothed, then ONE call of refit.refit_tracks over all of them refits pose and
        orig_cam to the tracks' keypoints and re-poses the fitted frames.  Each result gains `refit_shift` [T,24], `refit_cost` [T,2],
        `refit_flag` [T] and `pose_net` / `betas_net` / `orig_cam_net`, the network's values; var, var_global, pred_cam and
        smpl_joints2d stay those of the raw prediction.  --infill, then --smooth_uncert or --smooth, work on what the refit left."""
        from . import refit
        res = {pid: self._finish_track(tr, stacked[pid], orig_width, orig_height, smooth=False) for pid, tr in tracking_results.items()}
        if self._refit_tables is None:
            self._refit_tables = refit.joint_tables(self.args.smpl)
        a = self.args
        thr = float(getattr(a, "kp_vis_thresh", 0.3))
        fit = refit.refit_tracks(self.model, res, float(a.kp_refit), float(getattr(a, "kp_refit_ref", 0.3)), float(getattr(a, "kp_refit_rho", 0.1)),
                                 thr, int(getattr(a, "kp_refit_iters", 10)), tables=self._refit_tables, img_w=orig_width, img_h=orig_height)
        print(refit.summary_line(fit, res, self._refit_tables, orig_width, orig_height, thr))
        for pid, r in res.items():
            for net, k in (("pose_net", "pose"), ("betas_net", "betas"), ("orig_cam_net", "orig_cam")):
                r.setdefault(net, r[k])
            for k in ("pose", "orig_cam", "verts", "smpl_joints3d", "refit_shift", "refit_cost", "refit_flag"):
                r[k] = fit[pid][k]
        if getattr(a, "infill", None) is not None:
            from . import infill
            filled = infill.infill_tracks(self.model, res, float(a.infill), int(getattr(a, "infill_max_gap", 30)))
            for pid, r in res.items():
                for k in ("pose", "betas", "orig_cam", "verts", "smpl_joints3d", "infill"):
                    r[k] = filled[pid][k]
            print(infill.summary_line(filled))
        if getattr(a, "smooth_uncert", None) is not None:
            return self._smooth_tracks_uncert(res, a.smooth_uncert)
        if getattr(a, "smooth", False):
            from .smooth import smooth_pose
            for r in res.values():
                r["verts"], r["pose"], r["smpl_joints3d"] = smooth_pose(self.model, r["pose"], r["betas"], getattr(a, "min_cutoff", 0.004),
                                                                        getattr(a, "beta", 1.5))
        return res

    def _smooth_tracks_uncert(self, res: dict, lam: float) -> dict:
        """--smooth_uncert LAMBDA on finished, unsmoothed tracks (after --infill where that is given: its output is what is
        smoothed, with the `var` as regressed): ONE call of usmooth.smooth_tracks over all tracks replaces pose, betas and orig_cam
        by the smoothed values and re-poses every frame.  Each result gains `smooth_shift` [T,24] (degrees) and, unless --infill
        put them there already, `pose_net` / `betas_net` / `orig_cam_net`; var, var_global, pred_cam and smpl_joints2d stay those
        of the raw prediction."""
        from . import usmooth
        sm = usmooth.smooth_tracks(self.model, res, float(lam), float(getattr(self.args, "smooth_uncert_ref", 0.3)),
                                   int(getattr(self.args, "smooth_uncert_max_gap", 30)))
        for pid, r in res.items():
            for net, k in (("pose_net", "pose"), ("betas_net", "betas"), ("orig_cam_net", "orig_cam")):
                r.setdefault(net, r[k])
            for k in ("pose", "betas", "orig_cam", "verts", "smpl_joints3d", "smooth_shift"):
                r[k] = sm[pid][k]
        print(usmooth.summary_line(sm, res))
        return res

    def _finish_tracks_infilled(self, tracking_results: dict, stacked: dict, orig_width: int, orig_height: int) -> dict:
        """--infill THRESH: the tracks are finished unsmoothed (video_uncert, convert_crop_cam_to_orig_img), then ONE call of
        infill.infill_tracks over all of them replaces the rotations whose `var` exceeds THRESH (betas and orig_cam follow the root
        joint, the touched frames are re-posed), and only then does --smooth filter the in-filled pose - its LBS call supplies the
        meshes.  Each result gains `infill` [T,24] and `pose_net` / `betas_net` / `orig_cam_net`, the values before in-filling; var,
        var_global, pred_cam and smpl_joints2d stay those of the raw prediction."""
        from . import infill
        res = {pid: self._finish_track(tr, stacked[pid], orig_width, orig_height, smooth=False) for pid, tr in tracking_results.items()}
        filled = infill.infill_tracks(self.model, res, float(self.args.infill), int(getattr(self.args, "infill_max_gap", 30)))
        for pid, r in res.items():
            f = filled[pid]
            r["pose_net"], r["betas_net"], r["orig_cam_net"] = r["pose"], r["betas"], r["orig_cam"]
            for k in ("pose", "betas", "orig_cam", "verts", "smpl_joints3d", "infill"):
                r[k] = f[k]
            if getattr(self.args, "smooth", False):
                from .smooth import smooth_pose
                r["verts"], r["pose"], r["smpl_joints3d"] = smooth_pose(self.model, r["pose"], r["betas"],
                                                                        getattr(self.args, "min_cutoff", 0.004),
                                                                        getattr(self.args, "beta", 1.5))
        print(infill.summary_line(filled))
        return res

    def _finish_track(self, tr: dict, st: Dict[str, np.ndarray], orig_width: int, orig_height: int,
                      smooth: Optional[bool] = None) -> dict:
        """Per-track post-processing of tester.py:416-479 on the raw per-frame network outputs `st` (keys: pred_cam,
        smpl_vertices, pred_pose, pred_shape, smpl_joints3d, smpl_joints2d, var_pose): optional one-euro smoothing
        (meshes / 3-D joints re-derived from the filtered pose; the 2-D joints stay those of the raw prediction, as in
        the reference), uncertainty post-processing, camera / keypoint conversion to the original image.  `joints2d` is the
        track's own input keypoints (original-image pixels, what the reference's run_on_video stores) or None."""
        bboxes = np.asarray(tr["bbox"], np.float32).reshape(-1, 4)
        pose, betas = st["pred_pose"], st["pred_shape"]
        verts, j3d = st["smpl_vertices"], st["smpl_joints3d"]
        if getattr(self.args, "smooth", False) if smooth is None else smooth:               # tester.py:442-447
            from .smooth import smooth_pose
            verts, pose, j3d = smooth_pose(self.model, pose, betas, getattr(self.args, "min_cutoff", 0.004),
                                           getattr(self.args, "beta", 1.5))
        extra = {}
        if "select" in st:                      # --cfg2 / --ckpt2: var_global per row by the rule of the model chosen for the root
            from .select import pair_uncert
            var, var_global = pair_uncert(st["var_pose"], st["select"], self.pair.backbones, self.model_cfg.POCO.KINEMATIC_UNCERT,
                                          clip=False)
            extra = {"select": st["select"], "select_score": st["select_score"]}
        else:
            var, var_global = postproc.video_uncert(st["var_pose"], self.backbone,
                                                    self.model_cfg.POCO.KINEMATIC_UNCERT)    # tester.py:416-419
        if "stitch" in st:                      # --track_stitch: which rows filled a hole, and the fragment each other row came from
            extra = {**extra, "stitch": st["stitch"], "stitch_frag": st["stitch_frag"]}
        return {
            **extra,
            "pred_cam": st["pred_cam"],
            "orig_cam": postproc.convert_crop_cam_to_orig_img(st["pred_cam"], bboxes, orig_width, orig_height),
            "verts": verts, "pose": pose, "betas": betas, "joints2d": tr.get("joints2d"),
            "smpl_joints3d": j3d,
            "smpl_joints2d": postproc.convert_crop_coords_to_orig_img(bboxes, st["smpl_joints2d"],
                                                                      self.model_cfg.DATASET.IMG_RES),
            "var": var, "var_global": var_global,
            "bboxes": bboxes, "frame_ids": np.asarray(tr["frames"]),
        }

    def run_on_image_folder(self, image_folder: str, detections, output_path: str, bbox_scale=1.0):
        """pocolib/core/tester.py:153-245: images are streamed (decode -> regress -> write), every `--skip_frame`-th image of
        the sorted listing (tester.py:171), so host memory does not grow with the folder.  Unlike the reference's one
        forward per image, consecutive images share forwards of up to --batch_size crops (iter_frame_results); what is
        written per image is the same.  The host side is a pipeline: a small thread pool decodes the next images while the
        GPU regresses (PIL releases the GIL while decoding), another one compresses and writes the per-image .npz files (zlib
        releases it too); at most 2 x batch_size decoded images / unwritten results are in flight."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        names_all = sorted(x for x in os.listdir(image_folder) if x.lower().endswith(IMG_EXT))
        skip = max(int(getattr(self.args, "skip_frame", 1) or 1), 1)
        os.makedirs(output_path, exist_ok=True)
        picked = [(pos, names_all[pos]) for pos in range(0, len(names_all), skip)]
        counts = []
        nthreads = max(1, min(8, (os.cpu_count() or 2) // 2))
        # decode look-ahead / unwritten results in flight: about one batch, and bounded in bytes by the first image's size
        # (2 x batch_size 1080p frames were 0.8 GB at batch_size 64)
        ahead = max(4, self.model.max_batch)
        ahead_bytes = 256 << 20

        on_gpu = self.decode_any_on_gpu

        def decode(n):
            if on_gpu:                                   # the file's bytes: routed and decoded per batch (decode_frames)
                with open(os.path.join(image_folder, n), "rb") as f:
                    return f.read()
            return np.asarray(Image.open(os.path.join(image_folder, n)).convert("RGB"))

        def dets_of(pos, n, img):
            d = None
            if isinstance(detections, dict):
                d = detections.get(n)
            elif detections is not None and pos < len(detections):      # reference cache: indexed by image position
                d = detections[pos]
            if d is not None and len(d) > 0:
                d = np.asarray(d).reshape(-1, 4)
                return d if d.dtype in (np.float32, np.float64) else d.astype(np.float32)
            H, W = img.shape[:2]                                        # no detector in scope: one centred square box
            s = float(min(H, W))
            return np.array([[W / 2.0, H / 2.0, s, s]], dtype=np.float32)

        render_on = self.render_on
        render_crop = render_on and bool(getattr(self.args, "render_crop", False))
        first_box = deque()                                          # --render_crop: each image's first detection, as it was cropped
        occ_on = self.occlusion_on
        occ_boxes = deque()                                          # --occlusion_map: each image's detections, as they were cropped
        occ_dir = os.path.join(output_path, "occlusion")
        if occ_on:
            os.makedirs(occ_dir, exist_ok=True)
        img_dir = os.path.join(output_path, "poco_results")          # reference demo.py:95
        if render_on:
            os.makedirs(img_dir, exist_ok=True)

        def write(n, r):
            np.savez_compressed(os.path.join(output_path, os.path.splitext(n)[0] + "_poco.npz"), **r)
            if getattr(self.args, "save_obj", False):          # tester.py:300-303
                self._save_meshes(os.path.join(output_path, "meshes", os.path.splitext(n)[0]), r["verts"],
                                  [f"{i:06d}" for i in range(len(r["verts"]))])

        def listed(pos, n):                                             # the detections dets_of will find, without the image
            d = detections.get(n) if isinstance(detections, dict) else (
                detections[pos] if detections is not None and pos < len(detections) else None)
            return len(d) if d is not None and len(d) > 0 else 1

        self.pseudo_begin(sum(listed(pos, n) for pos, n in picked))       # --save_dataset: every crop is offered once
        t0 = time.time()
        n_img = 0
        with ThreadPoolExecutor(nthreads) as dec_pool, ThreadPoolExecutor(nthreads) as wr_pool:
            def items():
                nonlocal ahead
                q = deque()
                it = iter(picked)
                done = False

                def fill():
                    nonlocal done
                    while not done and len(q) < ahead:
                        nxt = next(it, None)
                        if nxt is None:
                            done = True
                        else:
                            q.append((nxt[0], nxt[1], dec_pool.submit(decode, nxt[1])))

                fill()
                ready = deque()                      # --decode gpu / --decode_png gpu: (pos, name, frame) of the batch decoded last
                while q or ready:
                    if on_gpu and not ready:
                        group = [q.popleft() for _ in range(min(len(q), max(1, self.model.max_batch)))]
                        frames = self.decode_frames([(n, fut.result()) for _, n, fut in group])
                        ready.extend((pos, n, fr) for (pos, n, _), fr in zip(group, frames))
                    if on_gpu:
                        pos, n, img = ready.popleft()
                    else:
                        pos, n, fut = q.popleft()
                        img = fut.result()
                    ahead = max(4, min(ahead, ahead_bytes // max(1, img.shape[0] * img.shape[1] * 3)))   # big images: fewer of them decoded ahead
                    fill()
                    d = dets_of(pos, n, img)
                    counts.append(len(d))
                    if render_crop:
                        first_box.append(d[0])
                    if occ_on:
                        occ_boxes.append(d)
                    yield img, d

            writes = deque()

            def picture(stem, pic):
                if self.image_format == "jpg":
                    return wr_pool.submit(_write_bytes, stem + ".jpg", self.encode_jpeg(pic))
                if self.encode_on_gpu:
                    return wr_pool.submit(_write_bytes, stem + ".png", self.encode_png(pic))
                return wr_pool.submit(_write_png, stem + ".png", pic.cpu().numpy())

            for (pos, n), r in zip(picked, self.iter_frame_results(items(), bbox_scale, keep_frames=render_on or occ_on)):
                n_img += 1
                if render_on or occ_on:
                    r, fr = r
                box0 = first_box.popleft() if render_crop else None
                boxes = occ_boxes.popleft() if occ_on else None
                if occ_on and r is not None:
                    for k, (pic, arrays) in enumerate(self.occlusion_maps(fr, boxes, bbox_scale)):
                        stem = os.path.join(occ_dir, f"{os.path.splitext(n)[0]}_{k}")
                        writes.append(picture(stem, pic))
                        writes.append(wr_pool.submit(_write_npz, stem + ".npz", arrays))
                if r is not None:
                    writes.append(wr_pool.submit(write, n, r))
                    if render_crop:                               # tester.py:256-285: the first detection on its own crop
                        pic = self.render_crop_frame(fr, r, box0, bbox_scale)
                    elif render_on:                               # tester.py:248-345: detection order, white side canvas
                        kp = None
                        if self.draw_keypoints:
                            from .render import folder_keypoints
                            kp = [folder_keypoints(j) for j in r["smpl_joints2d"]]
                        pic = self.render_frame(fr, r["verts"], r["orig_cam"], r["var"], side_bg=255, keypoints=kp)
                    if render_on:
                        writes.append(picture(os.path.join(img_dir, os.path.splitext(n)[0]), pic))
                while len(writes) > ahead:
                    writes.popleft().result()
            for w in writes:
                w.result()                                      # re-raises a failed write
        dataset = self.pseudo_finish(lambda x: picked[x[0]][1], lambda x: x[1])   # imgname = the file name, person_id = detection index
        self.select_summary()
        torch.cuda.synchronize()
        dt = time.time() - t0
        n_crops = int(sum(counts))
        return {"images": n_img, "crops": n_crops, "seconds": dt, "fps": n_img / max(dt, 1e-9),
                "crops_per_s": n_crops / max(dt, 1e-9), **dataset}


def _run_on_video_folder(self, frame_folder: str, tracking_path: Optional[str], output_path: str, bbox_scale=1.0):
    """demo.py --mode video on a folder of extracted frames or a Motion-JPEG .avi (demo.py:60-160): per-track results written
    as <output>/poco_results.npz (the reference joblib-dumps the same dict, demo.py:147-150).  tracking_path: a tracking file
    (load_tracking), what load_tracking returned for one, or None = one centred track over all frames."""
    if os.path.isfile(frame_folder):
        from .jpeg import MjpegReader
        with MjpegReader(frame_folder) as reader:
            return _run_on_frames(self, frame_folder, tracking_path, output_path, bbox_scale, reader)
    return _run_on_frames(self, frame_folder, tracking_path, output_path, bbox_scale, None)


class _GroupLoader:
    """load(i) of video mode when frames are decoded on the device.  One workgroup per image (PNG) or a handful of small launches
    (JPEG) leave a frame-by-frame call with most of the device idle, and the frames a pass will read are known before it starts
    (plan): on a miss, frame i is decoded together with the next wanted frames in ONE decode_frames call - at most batch_size
    frames and at most 256 MiB of decoded pixels.  A group is dropped when the next one is made."""

    def __init__(self, tester, names, read, H: int, W: int):
        self.tester, self.names, self.read = tester, names, read
        self.limit = max(1, min(max(1, tester.model.max_batch), (256 << 20) // max(1, H * W * 3)))
        self.wanted, self.group = [], {}

    def plan(self, frames) -> None:
        self.wanted, self.group = [int(f) for f in frames if 0 <= int(f) < len(self.names)], {}

    def __call__(self, i: int):
        i = int(i)
        if i not in self.group:
            import bisect
            k = bisect.bisect_left(self.wanted, i)
            ids = [i] + [f for f in self.wanted[k:k + self.limit] if f != i][:self.limit - 1]
            frames = self.tester.decode_frames([(self.names[f], self.read(f)) for f in ids])
            self.group = dict(zip(ids, frames))
        return self.group[i]


def _run_on_frames(self, frame_folder: str, tracking_path: Optional[str], output_path: str, bbox_scale, reader):
    import io
    from PIL import Image
    if reader is not None:                             # a Motion-JPEG .avi: frames named as the reference's ffmpeg extraction names them
        names = [f"{i + 1:06d}.jpg" for i in range(len(reader))]
        read = lambda i: reader[i]                                                                 # noqa: E731
    else:
        names = sorted(x for x in os.listdir(frame_folder) if x.lower().endswith(IMG_EXT))

        def read(i):
            with open(os.path.join(frame_folder, names[i]), "rb") as f:
                return f.read()
    if not names:
        raise FileNotFoundError(f"no frames in {frame_folder}")
    if reader is not None:
        first = np.asarray(Image.open(io.BytesIO(read(0))).convert("RGB"))
    else:
        first = np.asarray(Image.open(os.path.join(frame_folder, names[0])).convert("RGB"))
    H, W = first.shape[:2]
    if isinstance(tracking_path, dict):                # already loaded (demo.py checks the file before the engine is built)
        tracking = tracking_path
    elif tracking_path:
        tracking = load_tracking(tracking_path, **tracking_options(self.args))
    else:
        s = float(min(H, W))
        tracking = {"0": {"bbox": np.tile([[W / 2.0, H / 2.0, s, s]], (len(names), 1)).astype(np.float32),
                          "frames": np.arange(len(names))}}
    skip = max(int(getattr(self.args, "skip_frame", 1)), 1)
    if skip > 1:
        tracking = {k: {n: a[::skip] for n, a in v.items()} for k, v in tracking.items()}      # bbox, frames (, joints2d)
    if self.decode_any_on_gpu:
        load = _GroupLoader(self, names, read, H, W)
    elif reader is not None:
        load = lambda i: np.asarray(Image.open(io.BytesIO(read(i))).convert("RGB"))                # noqa: E731
    else:
        load = lambda i: np.asarray(Image.open(os.path.join(frame_folder, names[i])).convert("RGB"))   # noqa: E731
    import torch.distributed as tdist
    world = tdist.get_world_size() if tdist.is_available() and tdist.is_initialized() else 1
    rank = tdist.get_rank() if world > 1 else 0
    t0 = time.time()
    mine = tracking
    dataset = {}
    if world > 1:
        # whole tracks are the unit of sharding (temporal smoothing stays local: the owning rank smooths and
        # finishes its tracks); the only exchange is one all-gather of the packed per-frame SMPL records, from which rank 0
        # - the writer - re-derives the meshes of the tracks regressed elsewhere
        from . import dist as pdist
        mine = pdist.shard_tracks(tracking, rank, world)
        if isinstance(load, _GroupLoader):
            load.plan(sorted({int(f) for v in mine.values() for f in v["frames"]}))
        raw = self.run_on_video(mine, load, W, H, bbox_scale, raw=True) if mine else {}
        results = self._merge_rank_results(raw, tracking, W, H)
    else:
        if isinstance(load, _GroupLoader):
            load.plan(sorted({int(f) for v in tracking.values() for f in v["frames"]}))
        self.pseudo_begin(sum(len(v["frames"]) for v in tracking.values()))
        self.stitched_tracking = None
        results = self.run_on_video(tracking, load, W, H, bbox_scale)
        if self.stitched_tracking is not None:                             # --track_stitch: the chains are the tracks from here on
            from .sort import write_tracking
            os.makedirs(output_path, exist_ok=True)
            write_tracking(os.path.join(output_path, "tracking_results_stitched.json"), self.stitched_tracking)
            tracking = self.stitched_tracking
        order = {pid: i for i, pid in enumerate(tracking)}
        vstem = os.path.splitext(os.path.basename(os.path.normpath(frame_folder)))[0]

        def frame_name(x):              # the frame's file name; a video file has none: <stem>/<frame index>
            f = int(tracking[x[0]]["frames"][x[1]])
            return f"{vstem}/{f:06d}" if reader is not None else (names[f] if 0 <= f < len(names) else f"{f:06d}")

        dataset = self.pseudo_finish(frame_name, lambda x: int(x[0]) if str(x[0]).lstrip("-").isdigit() else order[x[0]])
    if self.calibration is not None:                                   # after everything that changes `var`
        for r in results.values():
            r.update(self.calibration.apply(r["var"]))
    torch.cuda.synchronize()
    dt = time.time() - t0
    if rank != 0:
        tdist.barrier()
        return {"rank": rank, "tracks_local": len(mine), "seconds": dt}
    try:
        os.makedirs(output_path, exist_ok=True)
        flat = {f"{pid}/{k}": v for pid, r in results.items() for k, v in r.items() if v is not None}
        np.savez_compressed(os.path.join(output_path, "poco_results.npz"), **flat)
        if getattr(self.args, "save_obj", False):                      # tester.py:532-535
            for pid, r in results.items():
                sub = f"{int(pid):04d}" if str(pid).lstrip("-").isdigit() else str(pid)
                self._save_meshes(os.path.join(output_path, "meshes", sub), r["verts"], [f"{int(f):06d}" for f in r["frame_ids"]])
        if self.render_on:                                             # demo.py:147-150 -> tester.py:482-580, rank 0 only
            if isinstance(load, _GroupLoader):
                load.plan(list(range(len(names))))
            self._render_video(results, frame_folder, names, load, output_path)
    finally:
        if world > 1:               # the other ranks wait here: release them also when the write fails
            tdist.barrier()
    n_crops = sum(len(v["frames"]) for v in tracking.values())
    n_frames = len({int(f) for v in tracking.values() for f in v["frames"]})
    return {"images": n_frames, "crops": n_crops, "tracks": len(tracking), "seconds": dt, "ranks": world,
            "fps": n_frames / max(dt, 1e-9), "crops_per_s": n_crops / max(dt, 1e-9), **dataset}


def _merge_rank_results(self, local_raw: dict, tracking: dict, W: int, H: int) -> dict:
    """Multi-GPU video mode.  The OWNING rank finishes its tracks (one-euro smoothing included, _finish_track) and packs
    per frame [final pose 216 | betas 10 | cam 3 | raw var_pose 24 | global confidence 1 | raw crop-space 2-D joints 98];
    ONE all-gather (RCCL when the group's backend is nccl) moves 1.4 KB per crop instead of 83 KB of vertices.  Only rank 0
    - the writer - re-derives the meshes / 3-D joints of the tracks regressed elsewhere from the gathered (already
    smoothed) pose with the batched LBS operator; the other ranks return their own tracks (no rank repeats
    another rank's LBS, smoothing or D2H)."""
    import torch.distributed as tdist
    from . import dist as pdist
    dev = pdist.collective_device()
    rank = tdist.get_rank()
    out, recs = {}, {}
    for pid, st in local_raw.items():
        fin = self._finish_track(tracking[pid], st, W, H)
        out[pid] = fin
        t = {"pred_pose": torch.from_numpy(np.ascontiguousarray(fin["pose"], np.float32)), "pred_shape": torch.from_numpy(st["pred_shape"]),
             "pred_cam": torch.from_numpy(st["pred_cam"]), "var_pose": torch.from_numpy(st["var_pose"])}
        rec = pdist.pack_records(t, head=self.backbone, kinematic=self.model_cfg.POCO.KINEMATIC_UNCERT)
        j2 = torch.from_numpy(np.ascontiguousarray(st["smpl_joints2d"], np.float32)).reshape(rec.shape[0], 98)
        recs[str(pid)] = torch.cat([rec, j2], 1).to(dev)
    full = pdist.gather_track_records(recs, device=dev, width=pdist.VIDEO_REC)
    if rank != 0:
        return out
    for pid, tr in tracking.items():
        if pid in out:
            continue
        rec = full[str(pid)].cpu().numpy()
        T = rec.shape[0]
        pose, betas, cam = rec[:, 0:216].reshape(T, 24, 3, 3), rec[:, 216:226], rec[:, 226:229]
        verts = np.empty((T, 6890, 3), np.float32)
        j3d = np.empty((T, 49, 3), np.float32)
        for lo in range(0, T, self.model.max_batch):
            hi = min(T, lo + self.model.max_batch)
            v, j = self.model.smpl_lbs(torch.from_numpy(np.ascontiguousarray(betas[lo:hi])).to(self.device),
                                       torch.from_numpy(np.ascontiguousarray(pose[lo:hi])).to(self.device))
            verts[lo:hi], j3d[lo:hi] = v.cpu().numpy(), j.cpu().numpy()
        st = {"pred_cam": cam, "smpl_vertices": verts, "pred_pose": pose, "pred_shape": betas, "smpl_joints3d": j3d,
              "smpl_joints2d": rec[:, pdist.REC:pdist.VIDEO_REC].reshape(T, 49, 2), "var_pose": rec[:, 229:253]}
        out[pid] = self._finish_track(tr, st, W, H, smooth=False)        # the owner already smoothed this pose
    return {pid: out[pid] for pid in tracking}


def _write_png(path: str, img: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(img).save(path)


def _write_npz(path: str, arrays: dict) -> None:
    np.savez_compressed(path, **arrays)


def _write_bytes(path: str, data: bytes) -> None:
    with open(path, "wb") as f:
        f.write(data)


def _render_video(self, results: dict, frame_folder: str, names, load, output_path: str) -> None:
    """render_results of tester.py:482-580: every frame of the folder with the people the tracks place in it, in ascending
    orig_cam[1] (demo_utils.py:307-313, ties in track order), black side canvas, <output>/tmp_images_output/%06d.png, and the
    lines of <output>/uncertainty.log (tester.py:547-550).  --draw_keypoints stamps each person's 49 model joints green and, for a
    track that came with keypoints, its input keypoints above --kp_vis_thresh black on top.  --image_format jpg writes %06d.jpg, encoded on the device; --encode gpu
    compresses the .png files on the device;
    --save_video adds <output>/<frame folder>_poco_result.avi (Motion-JPEG of the same pictures at --fps: the reference's
    images_to_video, demo.py:148-157)."""
    from concurrent.futures import ThreadPoolExecutor
    from .render import input_keypoints, video_keypoints, video_order
    out_dir = os.path.join(output_path, "tmp_images_output")
    os.makedirs(out_dir, exist_ok=True)
    jpg = self.image_format == "jpg"
    video = None
    per_frame = [[] for _ in names]
    for pid, r in results.items():
        for k, f in enumerate(r["frame_ids"]):
            if 0 <= int(f) < len(names):
                per_frame[int(f)].append((pid, k))
    sideview = bool(getattr(self.args, "sideview", False))
    vis_thresh = float(getattr(self.args, "kp_vis_thresh", 0.3))

    def keypoints_of(pid, k):
        """--draw_keypoints: the 49 model joints green; for a keypoint track the confident input keypoints black on top."""
        kp = video_keypoints(results[pid]["smpl_joints2d"][k])
        if results[pid].get("joints2d") is None:
            return kp
        inp = input_keypoints(results[pid]["joints2d"][k], vis_thresh)
        return np.concatenate([kp[0], inp[0]], 0), np.concatenate([kp[1], inp[1]], 0)

    log_lines = []
    with ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        writes = []
        for fi, name in enumerate(names):
            fr = self.to_device(load(fi))
            people = per_frame[fi]
            if people:
                cams = np.stack([results[pid]["orig_cam"][k] for pid, k in people])
                people = [people[i] for i in video_order(cams)]
                pic = self.render_frame(fr, np.stack([results[pid]["verts"][k] for pid, k in people]),
                                        np.stack([results[pid]["orig_cam"][k] for pid, k in people]),
                                        np.stack([results[pid]["var"][k] for pid, k in people]), side_bg=0,
                                        keypoints=[keypoints_of(pid, k) for pid, k in people] if self.draw_keypoints else None)
                for pid, k in people:
                    g = float(np.clip(results[pid]["var_global"][k], 0, 0.99))
                    who = f"{int(pid):02d}" if str(pid).lstrip("-").isdigit() else str(pid)
                    log_lines.append(f"img_f:{os.path.join(frame_folder, name)} person:{who} var:{g:.3f}")
            else:
                pic = torch.cat([fr, torch.zeros_like(fr)], 1) if sideview else fr
            data = self.encode_jpeg(pic) if jpg or getattr(self.args, "save_video", False) else None
            if getattr(self.args, "save_video", False):
                if video is None:
                    from .jpeg import MjpegWriter
                    avi = os.path.basename(os.path.normpath(frame_folder))
                    avi = (os.path.splitext(avi)[0] if os.path.isfile(frame_folder) else avi) + "_poco_result.avi"
                    video = MjpegWriter(os.path.join(output_path, avi), int(pic.shape[1]), int(pic.shape[0]),
                                        float(getattr(self.args, "fps", 30.0)))
                video.add(data)
            if jpg:
                writes.append(pool.submit(_write_bytes, os.path.join(out_dir, f"{fi:06d}.jpg"), data))
            elif self.encode_on_gpu:
                writes.append(pool.submit(_write_bytes, os.path.join(out_dir, f"{fi:06d}.png"), self.encode_png(pic)))
            else:
                writes.append(pool.submit(_write_png, os.path.join(out_dir, f"{fi:06d}.png"), pic.cpu().numpy()))
            while len(writes) > 16:
                writes.pop(0).result()
        for w in writes:
            w.result()
    if video is not None:
        video.close()
    with open(os.path.join(output_path, "uncertainty.log"), "a") as f:
        for ln in log_lines:
            print(ln, file=f)


POCOTester.run_on_video_folder = _run_on_video_folder
POCOTester._render_video = _render_video
POCOTester._merge_rank_results = _merge_rank_results


def _load_any(path: str):
    """json, or the joblib/pickle caches the reference writes next to its outputs (demo.py:125-131,163-169)."""
    if path.lower().endswith((".pkl", ".pickle", ".joblib")):
        try:
            import joblib
            return joblib.load(path)
        except ImportError:
            import pickle
            with open(path, "rb") as f:
                return pickle.load(f)
    with open(path) as f:
        return json.load(f)


def load_detections(path: Optional[str]):
    """{image name: [[cx,cy,w,h],...]} (json) or the reference's `detection_results.pkl`: a sequence indexed by the
    position of the image in the sorted folder listing (tester.py:153-169).  None = no detector output."""
    return _load_any(path) if path else None


def tracking_options(args) -> dict:
    """load_tracking's keyword arguments from the demo's flags (--tracking_method, --kp_vis_thresh, --smooth_bbox)."""
    return {"method": getattr(args, "tracking_method", "bbox") or "bbox", "vis_thresh": float(getattr(args, "kp_vis_thresh", 0.3)),
            "smooth_bbox": bool(getattr(args, "smooth_bbox", False))}


def load_tracking(path: Optional[str], vis_thresh: float = 0.3, smooth_bbox: bool = False, method: str = "bbox",
                  min_frames: int = 25) -> Optional[dict]:
    """{person_id: {'bbox': [T,4] (cx,cy,w,h), 'frames': [T]}} from json or the reference's
    `tracking_results_<method>.pkl` (demo.py:125-131); tracks shorter than min_frames = MIN_NUM_FRAMES = 25 frames are dropped as in
    tester.py:133-136 (--track_stitch passes --stitch_min_frag: short fragments reach the forward, the rule is applied to the chains).

    The file's content decides how a track is read.  A track with `bbox` is read as it is; a `joints2d` array of the same length
    next to it is kept.  A track with `joints2d` [T,K,3] and no `bbox` - a pose tracker's output, the reference's
    --tracking_method pose - goes through tracks.boxes_from_keypoints (vis_thresh; smooth_bbox = median + Gaussian filter of the
    box parameters): its `bbox`, `frames` and `joints2d` are the derived, trimmed ones, the 25-frame rule applies to the trimmed
    length, and a track without a usable frame is dropped with one line on stderr.  method = 'pose' (--tracking_method pose):
    a track without `joints2d` is a ValueError that names it."""
    if not path:
        return None
    raw = _load_any(path)
    is_json = path.lower().endswith(".json")
    out = {}
    for k, v in raw.items():
        if method == "pose" and v.get("joints2d") is None:
            raise ValueError(f"--tracking_method pose: track {k!r} of {path} has no joints2d")
        frames = np.asarray(v["frames"], np.int64).reshape(-1)
        if v.get("bbox") is None and v.get("joints2d") is not None:
            from .tracks import boxes_from_keypoints
            tr = boxes_from_keypoints(v["joints2d"], frames, vis_thresh, smooth=smooth_bbox)
            if not len(tr["frames"]):
                import sys
                print(f"load_tracking: track {k!r} of {path} has no frame with a keypoint above {vis_thresh}: dropped", file=sys.stderr)
            elif is_json or len(tr["frames"]) >= min_frames:
                out[str(k)] = tr
        elif is_json or frames.shape[0] >= min_frames:
            out[str(k)] = {"bbox": np.asarray(v["bbox"], np.float32).reshape(-1, 4), "frames": frames}
            if v.get("joints2d") is not None and len(v["joints2d"]) == frames.shape[0]:
                try:
                    j = np.asarray(v["joints2d"], np.float64 if is_json else None)
                except (TypeError, ValueError):          # ragged, or None entries: not an array of keypoints
                    j = None
                if j is not None and j.ndim == 3 and j.dtype.kind == "f":
                    out[str(k)]["joints2d"] = j
    return out
