"""The reference's DATASET crop on the device (eval.py --crop dataset): BaseDataset.augm_params / rgb_processing and the
ground-truth transforms that go with them (pocolib/dataset/base_dataset.py:172-262, pocolib/utils/image_utils.py:21-45,111-118,
189-206,236-278, pocolib/utils/vibe_image_utils.py:49-91).

The pixels are made by ONE launch per batch (poco_dataset_crop, csrc/dataset_crop.hip): crops of mixed image sizes with rotation,
flip, scale and per-channel noise.  The host states gen_trans_from_patch_cv up to its three float32 source points (crop_params);
everything after that runs on the device.  The ground truth - 72 or 24 x 3 numbers per sample - is transformed on the host in
float64 numpy: dataset loading, not a hot path.  DESIGN.md section 22; tests/datacrop_np.py restates the contract.

Synthetic occluders (eval.py --aug_occlude): occlusion_params restates the draws of
occlude_with_pascal_objects_kp (pocolib/dataset/occlusion.py:109-149) on the host; the resize of the cut-outs and the alpha blend run
inside the same launch (poco_dataset_crop_occ), from an atlas of the cut-outs that is uploaded once."""
from __future__ import annotations

import ctypes as C
import random as pyrandom
from dataclasses import dataclass, field
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, lib

# pocolib/core/constants.py:104-111 (data, like the joint maps of evaluate.py)
SMPL_JOINTS_FLIP_PERM = [0, 2, 1, 3, 5, 4, 6, 8, 7, 9, 11, 10, 12, 14, 13, 15, 17, 16, 19, 18, 21, 20, 23, 22]
SMPL_POSE_FLIP_PERM = [3 * i + k for i in SMPL_JOINTS_FLIP_PERM for k in range(3)]
J24_FLIP_PERM = [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22]

# poco_dataset_crop_param_t (include/poco_hip.h): 48 bytes
PARAM_DTYPE = np.dtype([("img", np.int32), ("flip", np.int32), ("src", np.float32, (6,)), ("pn", np.float32, (3,)), ("bb", np.int32)])
assert PARAM_DTYPE.itemsize == 48

# poco_occluder_t, poco_occ_object_t, poco_occ_record_t (include/poco_hip.h)
OCCLUDER_DTYPE = np.dtype([("offset", np.int32), ("h", np.int32), ("w", np.int32)])
OCC_OBJECT_DTYPE = np.dtype([("id", np.int32), ("dst_w", np.int32), ("dst_h", np.int32), ("cx", np.int32), ("cy", np.int32)])
OCC_MAX_OBJECTS = 7
OCC_DTYPE = np.dtype([("count", np.int32), ("obj", OCC_OBJECT_DTYPE, (OCC_MAX_OBJECTS,))])
assert OCC_DTYPE.itemsize == 144 and OCCLUDER_DTYPE.itemsize == 12
OCC_MAX_RES = 256                                       # above it resize_by_factor could upscale: INTER_LINEAR is not built
OCC_MAX_SIDE = 4096

upload_count = 0                                        # images sent to the device by upload_image since import
upload_hook: Optional[Callable[[np.ndarray], None]] = None    # called with every image upload_image sends (tests count with it)


# ---- augmentation parameters ---------------------------------------------------------------------------------------------------
def augm_params(rng_state: np.random.RandomState, cfg, is_train: bool) -> Tuple[int, np.ndarray, float, float]:
    """BaseDataset.augm_params (base_dataset.py:172-199): flip, pn [3], rot (degrees), sc, drawn from rng_state in the reference's
    call order - the first uniform is drawn even when FLIP is off - so that RandomState(seed) gives the sequence the reference
    draws after np.random.seed(seed).  cfg: FLIP, NOISE_FACTOR, ROT_FACTOR, SCALE_FACTOR as attributes or keys."""
    g = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
    flip, pn, rot, sc = 0, np.ones(3), 0, 1
    if is_train:
        if rng_state.uniform() <= 0.5 and g("FLIP"):
            flip = 1
        pn = rng_state.uniform(1 - g("NOISE_FACTOR"), 1 + g("NOISE_FACTOR"), 3)
        rot = min(2 * g("ROT_FACTOR"), max(-2 * g("ROT_FACTOR"), rng_state.randn() * g("ROT_FACTOR")))
        sc = min(1 + g("SCALE_FACTOR"), max(1 - g("SCALE_FACTOR"), rng_state.randn() * g("SCALE_FACTOR") + 1))
        if rng_state.uniform() <= 0.6:
            rot = 0
    return flip, pn, rot, sc


@dataclass
class AugSpec:
    """What eval.py's augmentation flags ask for.  random=False: the fixed perturbation (rot degrees, scale, flip, noise) on every
    sample; random=True: per sample from augm_params with the config's factors under RandomState(seed), in dataset order."""
    rot: float = 0.0
    scale: float = 1.0
    flip: bool = False
    noise: Sequence[float] = (1.0, 1.0, 1.0)
    random: bool = False
    seed: int = 0
    cfg: object = None

    def draw(self, n: int):
        """flip int32 [n], pn float64 [n,3], rot float64 [n], sc float64 [n]."""
        flip, pn, rot, sc = np.zeros(n, np.int32), np.ones((n, 3)), np.zeros(n), np.ones(n)
        if self.random:
            rng = np.random.RandomState(self.seed)
            for i in range(n):
                flip[i], pn[i], rot[i], sc[i] = augm_params(rng, self.cfg, True)
        else:
            flip[:], pn[:], rot[:], sc[:] = int(bool(self.flip)), np.asarray(self.noise, np.float64).reshape(3), float(self.rot), float(self.scale)
        return flip, pn, rot, sc

    def describe(self) -> str:
        if self.random:
            g = (lambda k: self.cfg[k]) if isinstance(self.cfg, dict) else (lambda k: getattr(self.cfg, k))
            return (f"per sample from augm_params (ROT_FACTOR {g('ROT_FACTOR')}, SCALE_FACTOR {g('SCALE_FACTOR')}, NOISE_FACTOR "
                    f"{g('NOISE_FACTOR')}, FLIP {g('FLIP')}), seed {self.seed}")
        return f"rot {float(self.rot):g} deg, scale {float(self.scale):g}, flip {int(bool(self.flip))}, noise {tuple(float(x) for x in self.noise)}"


# ---- the crop --------------------------------------------------------------------------------------------------------------------
def _rotate_2d(x32, y32, rot_rad):
    """vibe_image_utils.py:49-55 on a float32 point: numpy's sin / cos in float64, float64 products, float32 result."""
    sn, cs = np.float64(np.sin(rot_rad)), np.float64(np.cos(rot_rad))
    x, y = np.float64(np.float32(x32)), np.float64(np.float32(y32))
    return np.float32(x * cs - y * sn), np.float32(x * sn + y * cs)


def crop_params(center, scale, rot, flip, pn, sc, res) -> np.ndarray:
    """One poco_dataset_crop_param_t record (img = 0) for crop_cv2(img, center, sc * scale, [res, res], rot) -> flip -> noise pn:
    c = int(round(center)), bb = int(round(sc * scale * 200)) and gen_trans_from_patch_cv(c_x, c_y, bb, bb, res, res, 1.0, rot) up to
    its float32 `src` (vibe_image_utils.py:58-79), with the dtype chain of the reference's numpy: float32 half extents, float64 sin /
    cos and products, float32 directions, float64 centre + direction, float32 points.  A non-finite input is a ValueError; a box
    side that rounds to 0 is left for poco_dataset_crop to refuse."""
    vals = [float(center[0]), float(center[1]), float(scale), float(rot), float(sc)] + [float(x) for x in pn]
    if not np.all(np.isfinite(vals)) or len(pn) != 3:
        raise ValueError(f"crop_params: centre, scale, rot, sc and the three noise factors must be finite, got {vals}")
    c_x, c_y = int(round(vals[0])), int(round(vals[1]))
    bb = int(round(vals[4] * vals[2] * 200.))
    if abs(bb) > 2 ** 30:
        raise ValueError(f"crop_params: box side {bb} is out of range")
    src_w = src_h = bb * 1.0
    rot_rad = np.pi * vals[3] / 180
    down = _rotate_2d(np.float32(0), np.float32(src_h * 0.5), rot_rad)
    right = _rotate_2d(np.float32(src_w * 0.5), np.float32(0), rot_rad)
    cx, cy = np.float64(c_x), np.float64(c_y)
    rec = np.zeros((), PARAM_DTYPE)
    rec["flip"] = int(bool(flip))
    rec["src"] = (cx, cy, cx + np.float64(down[0]), cy + np.float64(down[1]), cx + np.float64(right[0]), cy + np.float64(right[1]))
    rec["pn"] = vals[5:8]
    rec["bb"] = bb
    return rec


def batch_params(centers, scales, rots, flips, pns, scs, res) -> np.ndarray:
    """crop_params per sample, stacked: PARAM_DTYPE [N]."""
    out = np.zeros(len(centers), PARAM_DTYPE)
    for n in range(len(out)):
        out[n] = crop_params(centers[n], scales[n], rots[n], flips[n], pns[n], scs[n], res)
    return out


def upload_image(img_u8: np.ndarray, device) -> torch.Tensor:
    """uint8 [H,W,3] RGB to the device.  Counted in `upload_count` and reported to `upload_hook`."""
    global upload_count
    a = np.ascontiguousarray(img_u8, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"upload_image: need uint8 [H,W,3], got {a.shape}")
    upload_count += 1
    if upload_hook is not None:
        upload_hook(a)
    return torch.from_numpy(a).to(device)


def _bind():
    L = lib()
    if not getattr(L, "_datacrop_bound", False):
        L.poco_dataset_crop.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p]
        L._datacrop_bound = True
    return L


def _bind_occ():
    L = _bind()
    if not getattr(L, "_datacrop_occ_bound", False):
        L.poco_dataset_crop_occ.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]
        L.poco_dataset_crop_occ_mask.argtypes = L.poco_dataset_crop_occ.argtypes[:-1] + [C.c_void_p, C.c_void_p]
        L._datacrop_occ_bound = True
    return L


# ---- synthetic occluders: the host side --------------------------------------------------------------------------------------------
def _check_cutout(a, where: str) -> np.ndarray:
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4 and 1 <= a.shape[0] <= OCC_MAX_SIDE
            and 1 <= a.shape[1] <= OCC_MAX_SIDE):
        what = f"{a.dtype} {a.shape}" if isinstance(a, np.ndarray) else type(a).__name__
        raise ValueError(f"{where} is not a uint8 [h, w, 4] RGBA cut-out with sides in 1..{OCC_MAX_SIDE}: {what}")
    return np.ascontiguousarray(a)


def load_occluders(path: str) -> list:
    """The reference's pascal_occluders.pkl (joblib: a list of uint8 [h, w, 4] RGBA cut-outs, occlusion.py:43-98) or an .npz whose
    arrays are such cut-outs, taken in sorted key order.  Anything else is a ValueError that names the offending entry."""
    import os
    if not os.path.isfile(path):
        raise ValueError(f"occluder file not found: {path}")
    if path.endswith(".npz"):
        try:
            with np.load(path, allow_pickle=False) as z:
                items = [(f"{path}: array {k!r}", z[k]) for k in sorted(z.files)]
        except ValueError:
            raise
        except Exception as e:
            raise ValueError(f"{path}: not a readable .npz ({e})")
    else:
        import joblib
        try:
            obj = joblib.load(path)
        except Exception as e:
            raise ValueError(f"{path}: not a joblib file of cut-outs ({type(e).__name__}: {e})")
        if not isinstance(obj, (list, tuple)):
            raise ValueError(f"{path}: a list of cut-outs is expected, got {type(obj).__name__}")
        items = [(f"{path}: entry {i}", a) for i, a in enumerate(obj)]
    if not items:
        raise ValueError(f"{path}: no cut-out in the file")
    return [_check_cutout(a, where) for where, a in items]


def occlusion_params(np_rng: np.random.RandomState, py_rng: pyrandom.Random, kp24, scale, occluder_hw, res: int = 224) -> dict:
    """The draws of occlude_with_pascal_objects_kp (occlusion.py:109-149) for one sample, up to the two calls that touch pixels, with
    the reference's draw order and dtype chain: count = randint(1, 8); per object random.choice (Python's generator), choice among the
    visible keypoints, two randn, one uniform(0.2, 1.0).  kp24: the 24 ground-truth keypoints after j2d_processing (normalised crop
    coordinates, float32; the reference's kp2d[25:]), brought to pixels with the reference's literal 224; scale = sc * scale;
    occluder_hw: (h, w) per cut-out.  Returns dict(count = the count drawn, objects = [(id, dst_w, dst_h, cx, cy)] kept, skipped,
    no_visible).  Where the reference raises: no keypoint with confidence > 0.3 -> the sample stays unoccluded after its count draw;
    a new size with a zero side -> that object is skipped after its draws."""
    res = int(res)
    if not 1 <= res <= OCC_MAX_RES:
        raise ValueError(f"occlusion_params: res must be in 1..{OCC_MAX_RES} (above it a cut-out could be upscaled: INTER_LINEAR is not built)")
    if len(occluder_hw) < 1:
        raise ValueError("occlusion_params: no cut-out")
    im_w = im_h = res
    im_scale_factor = min(im_w, im_h) / 256
    count = int(np_rng.randint(1, 8))
    kp = np.array(kp24, np.float32).reshape(24, 3)
    kp[:, :-1] = np.float32(0.5 * 224) * (kp[:, :-1] + np.float32(1))
    visible = kp[kp[..., -1] > 0.3]
    if len(visible) == 0:
        return dict(count=count, objects=[], skipped=0, no_visible=True)
    objects, skipped = [], 0
    for _ in range(count):
        oid = py_rng.choice(range(len(occluder_hw)))
        x, y = visible[np_rng.choice(range(len(visible)), 1)[0]][:2]
        delta_x = np.float64((np_rng.randn() * 0.1) * scale)
        delta_y = np.float64((np_rng.randn() * 0.1) * scale)
        cx = int(np.clip(np.float64(x) + delta_x, 0, im_w))           # truncates, does not round
        cy = int(np.clip(np.float64(y) + delta_y, 0, im_h))
        factor = np_rng.uniform(0.2, 1.0) * im_scale_factor + 1e-8
        h, w = occluder_hw[oid]
        new = np.round(np.array([int(w), int(h)]) * factor).astype(int)   # resize_by_factor
        if new[0] < 1 or new[1] < 1:
            skipped += 1
            continue
        objects.append((int(oid), int(new[0]), int(new[1]), cx, cy))
    return dict(count=count, objects=objects, skipped=skipped, no_visible=False)


def occ_records(objects) -> np.ndarray:
    """OCC_DTYPE [N] from per-sample lists of (id, dst_w, dst_h, cx, cy)."""
    rec = np.zeros(len(objects), OCC_DTYPE)
    for n, objs in enumerate(objects):
        if len(objs) > OCC_MAX_OBJECTS:
            raise ValueError(f"occ_records: sample {n} has {len(objs)} objects, at most {OCC_MAX_OBJECTS} fit a record")
        rec["count"][n] = len(objs)
        for k, o in enumerate(objs):
            rec["obj"][n, k] = tuple(int(v) for v in o)
    return rec


class OccluderAtlas:
    """All cut-outs as one packed uint8 RGBA buffer on the device with the (offset, h, w) table: uploaded once, read by every batch."""

    def __init__(self, occluders, device):
        cut = [_check_cutout(a, f"cut-out {i}") for i, a in enumerate(occluders)]
        if not cut:
            raise ValueError("OccluderAtlas: no cut-out")
        self.table = np.zeros(len(cut), OCCLUDER_DTYPE)
        off = 0
        for i, a in enumerate(cut):
            self.table[i] = (off, a.shape[0], a.shape[1])
            off += a.shape[0] * a.shape[1]
        if off >= 2 ** 31:
            raise ValueError(f"OccluderAtlas: {off} texels do not fit the table's int32 offsets")
        self.texels = off
        self.device = torch.device(device)
        self.d_atlas = torch.from_numpy(np.concatenate([a.reshape(-1) for a in cut])).to(self.device)
        self.d_table = torch.from_numpy(self.table.view(np.uint8).copy()).to(self.device)


@dataclass
class OcclusionSpec:
    """What eval.py --aug_occlude asks for: the cut-outs and the seed of the two generators (numpy's and Python's, as the reference
    uses both).  draw() makes every sample's objects once, in dataset order; atlas() uploads the cut-outs once per device."""
    occluders: Sequence[np.ndarray]
    seed: int = 0
    source: str = ""
    _atlas: dict = field(default_factory=dict, repr=False)

    def __post_init__(self):
        self.occluders = [_check_cutout(a, f"cut-out {i}") for i, a in enumerate(self.occluders)]
        if not self.occluders:
            raise ValueError("OcclusionSpec: no cut-out")

    @property
    def sizes(self):
        return [(a.shape[0], a.shape[1]) for a in self.occluders]

    def atlas(self, device) -> OccluderAtlas:
        key = str(torch.device(device))
        if key not in self._atlas:
            self._atlas[key] = OccluderAtlas(self.occluders, device)
        return self._atlas[key]

    def draw(self, aug: "AugSpec", part, center, scale, res: int = 224):
        """Per sample, in dataset order and from ONE RandomState(seed) as BaseDataset.__getitem__ draws: augm_params first (only a
        random AugSpec draws anything), then the sample's occlusion draws on its keypoints after j2d_processing with sc * scale, rot
        and flip.  part [N,24,3], center [N,2], scale [N] (the file's).  Returns (flip, pn, rot, sc) as AugSpec.draw does and a dict:
        objects (per-sample lists), count int32 [N] (objects kept), skipped and no_visible (totals)."""
        part = np.asarray(part, np.float64).reshape(-1, 24, 3)
        n = len(part)
        if aug.random and int(aug.seed) != int(self.seed):
            raise ValueError(f"OcclusionSpec.draw: one generator makes the augmentation and the occlusion draws, but the seeds differ "
                             f"({aug.seed} and {self.seed})")
        np_rng, py_rng = np.random.RandomState(self.seed), pyrandom.Random(self.seed)
        flip, pn, rot, sc = aug.draw(n) if not aug.random else (np.zeros(n, np.int32), np.ones((n, 3)), np.zeros(n), np.ones(n))
        objects, skipped, no_visible = [], 0, 0
        sizes = self.sizes
        for i in range(n):
            if aug.random:
                flip[i], pn[i], rot[i], sc[i] = augm_params(np_rng, aug.cfg, True)
            s_eff = np.float64(sc[i]) * np.float64(scale[i])
            kp = j2d_processing(part[i], center[i], float(s_eff), float(rot[i]), int(flip[i]), res)
            d = occlusion_params(np_rng, py_rng, kp, s_eff, sizes, res)
            objects.append(d["objects"])
            skipped += d["skipped"]
            no_visible += int(d["no_visible"])
        return (flip, pn, rot, sc), dict(objects=objects, count=np.asarray([len(o) for o in objects], np.int32), skipped=skipped,
                                         no_visible=no_visible)

    def describe(self) -> str:
        return f"{len(self.occluders)} cut-outs{' from ' + self.source if self.source else ''}, seed {self.seed}"


def dataset_crop(images: Sequence[torch.Tensor], img_index, params: np.ndarray, res: int = 224, normalize: bool = True,
                 out: Optional[torch.Tensor] = None, occlusion=None, want_mask: bool = False):
    """images: uint8 [H_i,W_i,3] RGB tensors on one device; img_index [N]: which of them crop n is cut from (an index outside the
    list is clamped into it by the kernel); params: PARAM_DTYPE [N] (crop_params / batch_params) -> fp32 [N,3,res,res] on that
    device: the normalised crop, or with normalize=False the raw float crop after noise and clamp.
    One small upload (pointer table, image sizes and records in one buffer) and one launch on the current stream.
    occlusion = (OccluderAtlas on the same device, OCC_DTYPE [N] records from occ_records): the synthetic occluders are pasted between
    flip and noise in the same launch (poco_dataset_crop_occ), the records travel in the same upload, and the result is (crops,
    cover) with cover int32 [N] on the device = the crop's pixels that a pasted texel with alpha > 0 touched.  want_mask=True (with
    occlusion): the launch is poco_dataset_crop_occ_mask and the result (crops, cover, mask) with mask uint8 [N,res,res] on the device =
    1 at exactly those pixels."""
    if len(images) < 1:
        raise ValueError("dataset_crop: no image")
    if want_mask and occlusion is None:
        raise ValueError("dataset_crop: want_mask needs occlusion (the mask marks the pixels the occluders touched)")
    dev = images[0].device
    for im in images:
        if not (torch.is_tensor(im) and im.is_cuda and im.device == dev and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3
                and im.is_contiguous() and 1 <= im.shape[0] <= 32767 and 1 <= im.shape[1] <= 32767):
            raise ValueError("dataset_crop: images must be contiguous uint8 [H,W,3] tensors on one device, up to 32767 x 32767")
    params = np.array(params, dtype=PARAM_DTYPE).reshape(-1)
    N, n_img = int(params.shape[0]), len(images)
    idx = np.asarray(img_index, np.int64).reshape(-1)
    if idx.shape[0] != N:
        raise ValueError(f"dataset_crop: {idx.shape[0]} image indices for {N} records")
    params["img"] = np.clip(idx, -2 ** 31, 2 ** 31 - 1)
    occ = None
    if occlusion is not None:
        atlas, occ = occlusion
        occ = np.array(occ, dtype=OCC_DTYPE).reshape(-1)
        if not isinstance(atlas, OccluderAtlas) or atlas.device != dev:
            raise ValueError("dataset_crop: occlusion needs an OccluderAtlas on the images' device")
        if occ.shape[0] != N:
            raise ValueError(f"dataset_crop: {occ.shape[0]} occlusion records for {N} crops")
    # [pointers 8 n_img | (H, W) 8 n_img | records 48 N | occlusion records 144 N]: every part starts on a multiple of 8 bytes
    host = np.zeros(16 * n_img + 48 * N + (144 * N if occ is not None else 0), np.uint8)
    host[:8 * n_img].view(np.int64)[:] = [im.data_ptr() for im in images]
    host[8 * n_img:16 * n_img].view(np.int32)[:] = [v for im in images for v in (im.shape[0], im.shape[1])]
    host[16 * n_img:16 * n_img + 48 * N] = params.view(np.uint8)
    if occ is not None:
        host[16 * n_img + 48 * N:] = occ.view(np.uint8)
    if out is None:
        out = torch.empty((N, 3, res, res), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, 3, res, res)):
        raise ValueError(f"dataset_crop: out must be a contiguous float32 [{N},3,{res},{res}] tensor on the images' device")
    if occ is not None:
        groups = (int(res) + 31) // 32
        with torch.cuda.device(dev):
            d = torch.from_numpy(host).to(dev)
            base = d.data_ptr()
            cover = torch.empty((N, groups * groups), dtype=torch.int32, device=dev)
            if want_mask:
                mask = torch.empty((N, int(res), int(res)), dtype=torch.uint8, device=dev)
                check(_bind_occ().poco_dataset_crop_occ_mask(
                    C.c_void_p(base), C.c_void_p(base + 8 * n_img), n_img, C.c_void_p(base + 16 * n_img), C.c_void_p(params.ctypes.data), N,
                    int(res), int(bool(normalize)), C.c_void_p(atlas.d_atlas.data_ptr()), atlas.texels, C.c_void_p(atlas.d_table.data_ptr()),
                    C.c_void_p(atlas.table.ctypes.data), len(atlas.table), C.c_void_p(base + 16 * n_img + 48 * N), C.c_void_p(occ.ctypes.data),
                    C.c_void_p(out.data_ptr()), C.c_void_p(cover.data_ptr()), C.c_void_p(mask.data_ptr()),
                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "poco_dataset_crop_occ_mask")
                return out, cover.sum(dim=1, dtype=torch.int32), mask
            check(_bind_occ().poco_dataset_crop_occ(
                C.c_void_p(base), C.c_void_p(base + 8 * n_img), n_img, C.c_void_p(base + 16 * n_img), C.c_void_p(params.ctypes.data), N, int(res),
                int(bool(normalize)), C.c_void_p(atlas.d_atlas.data_ptr()), atlas.texels, C.c_void_p(atlas.d_table.data_ptr()),
                C.c_void_p(atlas.table.ctypes.data), len(atlas.table), C.c_void_p(base + 16 * n_img + 48 * N), C.c_void_p(occ.ctypes.data),
                C.c_void_p(out.data_ptr()), C.c_void_p(cover.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                "poco_dataset_crop_occ")
            return out, cover.sum(dim=1, dtype=torch.int32)
    with torch.cuda.device(dev):
        d = torch.from_numpy(host).to(dev)
        base = d.data_ptr()
        check(_bind().poco_dataset_crop(C.c_void_p(base), C.c_void_p(base + 8 * n_img), n_img, C.c_void_p(base + 16 * n_img),
                                        C.c_void_p(params.ctypes.data), N, int(res), int(bool(normalize)), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "poco_dataset_crop")
    return out


# ---- ground truth (host, float64) -------------------------------------------------------------------------------------------------
def _aa_to_rotmat(aa) -> np.ndarray:
    a = np.asarray(aa, np.float64).reshape(3)
    th = float(np.linalg.norm(a))
    if th < 1e-12:
        return np.eye(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _rotmat_to_aa(R) -> np.ndarray:
    """Through the unit quaternion (largest component first, so angles near pi are stable), angle in [0, pi]."""
    R = np.asarray(R, np.float64)
    q = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    i = int(np.argmax(q))
    if i == 0:
        q = np.array([q[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        q = np.array([R[2, 1] - R[1, 2], q[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], q[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], q[3]])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    s = float(np.linalg.norm(q[1:]))
    if s < 1e-12:
        return 2.0 * q[1:]
    return q[1:] * (2.0 * np.arctan2(s, q[0]) / s)


def rot_aa(aa, rot) -> np.ndarray:
    """image_utils.py:236-247: Rodrigues -> Rz(-rot) . R -> axis-angle (the reference goes through cv2.Rodrigues twice)."""
    a = np.deg2rad(-float(rot))
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return _rotmat_to_aa(Rz @ _aa_to_rotmat(aa))


def flip_pose(pose) -> np.ndarray:
    """image_utils.py:269-278."""
    p = np.asarray(pose)[SMPL_POSE_FLIP_PERM].copy()
    p[1::3] = -p[1::3]
    p[2::3] = -p[2::3]
    return p


def flip_kp(kp) -> np.ndarray:
    """image_utils.py:258-266 for 24 keypoints."""
    k = np.asarray(kp)
    if len(k) != 24:
        raise ValueError(f"flip_kp: 24 keypoints expected, got {len(k)}")
    k = k[J24_FLIP_PERM].copy()
    k[:, 0] = -k[:, 0]
    return k


def pose_processing(pose, r, f) -> np.ndarray:
    """base_dataset.py:253-262: float32 [72].  At r = 0 the reference's rot_aa is a Rodrigues round trip - the identity up to its
    rounding - and is not made here, so that unperturbed ground truth stays bit for bit what the file holds."""
    p = np.array(pose, np.float64).reshape(72)
    if not r == 0:
        p[:3] = rot_aa(p[:3], r)
    if f:
        p = flip_pose(p)
    return p.astype(np.float32)


def j3d_processing(S, r, f) -> np.ndarray:
    """base_dataset.py:237-251 on S [24,3] or [24,4] (x, y, z[, confidence]): float32, same shape."""
    S = np.array(S, np.float64)
    rot_mat = np.eye(3)
    if not r == 0:
        rot_rad = -r * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
    S[:, :3] = np.einsum("ij,kj->ki", rot_mat, S[:, :3])
    if f:
        S = flip_kp(S)
    return S.astype(np.float32)


def get_transform(center, scale, res, rot=0) -> np.ndarray:
    """image_utils.py:21-45."""
    h = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0] = float(res[1]) / h
    t[1, 1] = float(res[0]) / h
    t[0, 2] = res[1] * (-float(center[0]) / h + .5)
    t[1, 2] = res[0] * (-float(center[1]) / h + .5)
    t[2, 2] = 1
    if not rot == 0:
        rot = -rot                                      # to match the direction of the crop's rotation
        rot_mat = np.zeros((3, 3))
        rot_rad = rot * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
        rot_mat[2, 2] = 1
        t_mat = np.eye(3)
        t_mat[0, 2] = -res[1] / 2
        t_mat[1, 2] = -res[0] / 2
        t_inv = t_mat.copy()
        t_inv[:2, 2] *= -1
        t = np.dot(t_inv, np.dot(rot_mat, np.dot(t_mat, t)))
    return t


def transform(pt, center, scale, res, rot=0) -> np.ndarray:
    """image_utils.py:111-118 (invert = 0): truncates toward zero, then adds 1."""
    t = get_transform(center, scale, res, rot=rot)
    new_pt = np.dot(t, np.array([pt[0] - 1, pt[1] - 1, 1.]).T)
    return new_pt[:2].astype(int) + 1


def j2d_processing(kp, center, scale, r, f, res: int = 224) -> np.ndarray:
    """base_dataset.py:223-235 on 24 keypoints (x, y, confidence) in image pixels; scale = sc * scale: float32 [24,3] in normalised
    crop coordinates."""
    kp = np.array(kp, np.float64)
    for i in range(kp.shape[0]):
        kp[i, 0:2] = transform(kp[i, 0:2] + 1, center, scale, [res, res], rot=r)
    kp[:, :-1] = 2. * kp[:, :-1] / res - 1.
    if f:
        kp = flip_kp(kp)
    return kp.astype(np.float32)


def crop_keypoints24(part, center, scale, rot, flip, res: int = 224) -> np.ndarray:
    """j2d_processing per sample followed by trainer.py:231-234 (back to crop pixels, float32): `part` [N,24,3] -> float32 [N,24,3].
    scale = sc * scale per sample."""
    p = np.asarray(part, np.float64).reshape(-1, 24, 3)
    out = np.stack([j2d_processing(p[i], center[i], float(scale[i]), float(rot[i]), int(flip[i]), res) for i in range(len(p))])
    out[:, :, :-1] = np.float32(0.5) * np.float32(res) * (out[:, :, :-1] + np.float32(1))
    return out
