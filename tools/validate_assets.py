"""Opt-in validation against the REAL, licence-gated assets.  Nothing here can run in
the build / CI image (no smplx, no SMPL_NEUTRAL.pkl, no data/poco_*.pt); it is the path by which a user who holds the licences
turns the two "parity unpinned" rows (a10 SMPL-LBS, f2 real-asset loaders) into pinned ones on their own machine.

    python tools/validate_assets.py [--smpl-pkl data/smpl/SMPL_NEUTRAL.pkl] [--extra data/J_regressor_extra.npy]
                                    [--smpl-npz data/smpl/SMPL_NEUTRAL.npz]
                                    [--ckpt data/poco_cliff.pt --cfg configs/demo_poco_cliff.yaml] [--device cuda:0]

Every stage whose inputs are missing is reported as SKIPPED (exit code 0); a stage that runs and disagrees is FAILED (exit 1).
  1. SMPL file: convert the licensed pickle with tools/convert_smpl.py (or take --smpl-npz) and check shapes / sparsity /
     kinematic tree against what pocolib/models/head/smpl_head.py:12-34 expects (6890 vertices, 24 joints, 207 pose-blend rows).
  2. LBS parity (needs `smplx` importable + the model directory): smplx.SMPL.forward(pose2rot=False) on random betas / rotations
     against oracle/smpl_np.py (float64) and - with a GPU - against poco_smpl_lbs; also the 21 extra-vertex ids and the 49-joint map
     against smplx's own VertexJointSelector / the reference's constants.  Gate: 1e-5 m (oracle), 1e-4 m (HIP fp32).
  3. Checkpoint: strict load of data/poco_{pare,cliff}.pt through poco_amd.checkpoint (pocolib/models/poco.py:131-154,
     train_utils.py:69-136): reports missing / unexpected / tolerated-unused keys and shape mismatches without needing a GPU;
     with a GPU it finalises the engine and runs one forward on a synthetic crop (finite outputs, orthonormal rotations).
  4. Crop (needs `cv2` importable; licence-free): the reference's per-detection crop - cv2.getAffineTransform +
     cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT) on uint8 exactly as pocolib/utils/vibe_image_utils.py:58-107 calls them - against
     the fixed-point restatement oracle/crop_np.py (uint8, byte for byte; the transform matrix bit for bit) and, with a GPU, against
     poco_crop_normalize.  `--crop` runs only this stage.
  5. Keypoint stamp (needs `cv2` importable; licence-free; opt-in): cv2.circle(img, (x, y), r, colour, -1) as
     pocolib/core/tester.py:324-328,552-554 calls it against the half-width table of include/poco_hip.h
     (POCO_DISC_HALF_WIDTHS, restated in tests/render_overlay_np.py) for every radius of the table, at the centre and clipped at the
     borders.  Runs only with `--keypoints`.
  6. Dataset crop (needs `cv2` importable; licence-free; opt-in): cv2.warpAffine on the FLOAT32 image as crop_cv2 calls it
     (pocolib/utils/image_utils.py:189-206) against the restatement tests/datacrop_np.py, bit for bit, and rot_aa's cv2.Rodrigues
     round trip (:236-247) against its scipy restatement.  Runs only with `--dataset-crop`.
  7. the synthetic occluders: the restated cv2.resize(INTER_AREA) on uint8 RGBA and whole occluded crops
     against the real cv2; prints the number of differing bytes.  Runs only with `--occlusion`.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SKIP, OK, FAIL = "SKIPPED", "OK", "FAILED"


def check_smpl_npz(smpl: dict) -> list:
    """Structural checks of an engine-format body model.  Returns a list of problems (empty = fine)."""
    from poco_amd import synth
    bad = []
    V = smpl["v_template"].shape[0]
    want = {"v_template": (V, 3), "shapedirs": (V, 3, 10), "posedirs": (207, V * 3), "J_regressor": (24, V),
            "J_regressor_extra": (9, V), "lbs_weights": (V, 24), "parents": (24,), "extra_vertex_ids": (21,), "joint_map": (49,)}
    for k, shp in want.items():
        if k not in smpl:
            bad.append(f"missing array {k}")
        elif tuple(smpl[k].shape) != shp:
            bad.append(f"{k}: shape {tuple(smpl[k].shape)}, expected {shp}")
    if bad:
        return bad
    if not np.array_equal(np.asarray(smpl["parents"], np.int64), synth.SMPL_PARENTS.astype(np.int64)):
        bad.append("kinematic tree differs from the SMPL tree (pocolib/utils/kp_utils.py:881-908)")
    if np.abs(smpl["lbs_weights"].sum(1) - 1).max() > 1e-4:
        bad.append("skinning weights do not sum to 1 per vertex")
    if np.abs(smpl["J_regressor"].sum(1) - 1).max() > 1e-3:
        bad.append("J_regressor rows do not sum to 1")
    if int(np.asarray(smpl["extra_vertex_ids"]).max()) >= V or int(np.asarray(smpl["joint_map"]).max()) >= 54:
        bad.append("extra_vertex_ids / joint_map out of range")
    return bad


def stage_smpl_file(args):
    npz = args.smpl_npz
    if args.smpl_pkl and os.path.isfile(args.smpl_pkl) and args.extra and os.path.isfile(args.extra):
        from tools import convert_smpl
        npz = npz or str(Path(args.smpl_pkl).with_suffix(".npz"))
        convert_smpl.main(args.smpl_pkl, args.extra, npz)
    if not npz or not os.path.isfile(npz):
        return SKIP, "no SMPL model (--smpl-pkl + --extra, or --smpl-npz)", None
    smpl = dict(np.load(npz))
    bad = check_smpl_npz(smpl)
    if bad:
        return FAIL, "; ".join(bad), None
    return OK, f"{npz}: {smpl['v_template'].shape[0]} vertices, tree / weights / regressors consistent", smpl


def lbs_against(fn_ref, smpl: dict, n: int = 8, seed: int = 0):
    """max |oracle - ref| over vertices and the 49 joints for random (betas, rotations); fn_ref(betas, rotmat) -> (verts, joints49)."""
    import torch
    from oracle import poco_ref, smpl_np
    r = np.random.default_rng(seed)
    betas = r.standard_normal((n, 10)).astype(np.float32)
    R = poco_ref.rot6d_to_rotmat(torch.from_numpy(r.standard_normal((n * 24, 6)).astype(np.float32))).reshape(n, 24, 3, 3).numpy()
    v64, j64 = smpl_np.smpl_lbs_np(smpl, betas, R)
    v, j = fn_ref(betas, R)
    return float(np.abs(np.asarray(v) - v64).max()), float(np.abs(np.asarray(j) - j64).max()), betas, R, v64, j64


def stage_lbs(args, smpl):
    if smpl is None:
        return SKIP, "no SMPL model"
    try:
        import smplx  # noqa: F401
        import torch
    except ImportError:
        return SKIP, "smplx is not importable (pip install smplx==0.1.28, requirements.txt:7)"
    model_dir = args.smpl_dir or (str(Path(args.smpl_pkl).parent) if args.smpl_pkl else None)
    if not model_dir or not os.path.isdir(model_dir):
        return SKIP, "no smplx model directory (--smpl-dir)"
    from smplx import SMPL as _SMPL
    from smplx.lbs import vertices2joints
    m = _SMPL(model_dir, create_transl=False)
    msgs = []
    # data the product keeps as constants: extra vertex ids (smplx VertexJointSelector) and the 49-joint map
    sel = getattr(getattr(m, "vertex_joint_selector", None), "extra_joints_idxs", None)
    if sel is not None and not np.array_equal(sel.cpu().numpy().astype(np.int64), np.asarray(smpl["extra_vertex_ids"], np.int64)):
        return FAIL, "extra_vertex_ids differ from smplx's VertexJointSelector: " + str(sel.cpu().numpy().tolist())
    Jx = torch.from_numpy(np.asarray(smpl["J_regressor_extra"], np.float32))
    jm = torch.from_numpy(np.asarray(smpl["joint_map"], np.int64))

    def ref(betas, R):                                    # pocolib/models/head/smpl_head.py:22-34 on the real smplx layer
        Rt = torch.from_numpy(R)
        o = m(betas=torch.from_numpy(betas), body_pose=Rt[:, 1:].contiguous(), global_orient=Rt[:, :1].contiguous(), pose2rot=False)
        joints = torch.cat([o.joints, vertices2joints(Jx, o.vertices)], 1)[:, jm]
        return o.vertices.detach().numpy(), joints.detach().numpy()

    dv, dj, betas, R, v64, j64 = lbs_against(ref, smpl)
    msgs.append(f"oracle (float64 restatement) vs smplx.SMPL.forward: vertices {dv:.2e} m, joints49 {dj:.2e} m")
    status = OK if max(dv, dj) < 1e-5 else FAIL
    if torch.cuda.is_available():
        from poco_amd.model import POCO
        eng = POCO(backbone="resnet50-cliff", num_flow_layers=1, max_batch=len(betas), smpl=smpl, device=args.device)
        # LBS only needs the body model; finalize() wants the network too: use the seeded synthetic weights
        from tests import util
        eng.load_state_dict(util.synth_weights("resnet50-cliff"), strict=True)
        eng.finalize()
        v, j = eng.smpl_lbs(torch.from_numpy(betas).to(args.device), torch.from_numpy(R).to(args.device))
        dvh, djh = float(np.abs(v.cpu().numpy() - v64).max()), float(np.abs(j.cpu().numpy() - j64).max())
        msgs.append(f"poco_smpl_lbs (HIP fp32) vs float64: vertices {dvh:.2e} m, joints49 {djh:.2e} m")
        if max(dvh, djh) >= 1e-4:
            status = FAIL
    else:
        msgs.append("no GPU: HIP LBS operator not exercised")
    return status, " | ".join(msgs)


def checkpoint_report(engine_tensors, loaded: dict) -> dict:
    """Strict comparison of a checkpoint's tensors with what the engine declares (names, shapes after dropping size-1 dims)."""
    want = {n: (tuple(s), req) for n, s, req in engine_tensors if not n.startswith("smpl.")}
    squeeze = lambda s: tuple(int(d) for d in s if int(d) != 1)   # noqa: E731
    rep = {"missing": sorted(n for n, (_, req) in want.items() if req and n not in loaded),
           "tolerated_unused_present": sorted(n for n, (_, req) in want.items() if not req and n in loaded),
           "unexpected": sorted(n for n in loaded if n not in want),
           "shape_mismatch": sorted(f"{n}: checkpoint {tuple(loaded[n].shape)} vs engine {want[n][0]}" for n in loaded
                                    if n in want and squeeze(loaded[n].shape) != squeeze(want[n][0]))}
    rep["ok"] = not (rep["missing"] or rep["unexpected"] or rep["shape_mismatch"])
    return rep


def stage_checkpoint(args, smpl):
    if not args.ckpt or not os.path.exists(args.ckpt):
        return SKIP, "no checkpoint (--ckpt data/poco_cliff.pt | data/poco_pare.pt)"
    if not args.cfg or not os.path.isfile(args.cfg):
        return SKIP, "no --cfg yaml for the checkpoint"
    import torch
    from poco_amd.checkpoint import read_checkpoint
    from poco_amd.config import model_kwargs, update_hparams
    from poco_amd.model import POCO
    kw = model_kwargs(update_hparams(args.cfg))
    sd = read_checkpoint(args.ckpt, args.inf_model)
    eng = POCO(**kw, max_batch=2, device=args.device)
    rep = checkpoint_report(eng.expected_tensors(), sd)
    msg = (f"{len(sd)} tensors; missing {len(rep['missing'])}, unexpected {len(rep['unexpected'])}, shape mismatches "
           f"{len(rep['shape_mismatch'])}, tolerated-unused present {len(rep['tolerated_unused_present'])}")
    for k in ("missing", "unexpected", "shape_mismatch"):
        if rep[k]:
            msg += f"\n      {k}: " + ", ".join(rep[k][:6]) + (" ..." if len(rep[k]) > 6 else "")
    if not rep["ok"]:
        return FAIL, msg
    eng.load_state_dict(sd, strict=True)
    if smpl is None or not torch.cuda.is_available():
        return OK, msg + " | strict load OK (no GPU or no SMPL model: forward not run)"
    from poco_amd import synth
    eng.load_smpl(smpl)
    eng.finalize()
    batch = {k: torch.from_numpy(v).to(args.device) for k, v in synth.synth_batch(2, 1).items()}
    out = eng(batch)
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(v).all()) for v in out.values() if torch.is_tensor(v))
    Rm = out["pred_pose"].reshape(-1, 3, 3)
    ortho = float((Rm @ Rm.transpose(1, 2) - torch.eye(3, device=Rm.device)).abs().max())
    ok = finite and ortho < 1e-4 and 0 < float(out["var_pose"].min()) and float(out["var_pose"].max()) < 1
    return (OK if ok else FAIL), msg + f" | forward on 2 synthetic crops: finite={finite}, |RR^T-I|={ortho:.1e}"


def crop_against_cv2(cv2, n: int = 64, seed: int = 0, device=None):
    """Random frames / boxes through the real cv2 calls the reference makes vs oracle/crop_np.py (and the HIP kernel on `device`).
    `cv2` is passed in so that the CPU test can hand over a stand-in built from the oracle itself (logic check only)."""
    from oracle import crop_np
    r = np.random.default_rng(seed)
    frame = r.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    boxes = np.stack([r.uniform(-60, 1340, n), r.uniform(-60, 780, n), r.uniform(8, 900, n), r.uniform(8, 900, n)], 1)
    boxes[0] = (112, 112, 224, 224)
    worst = {"matrix_bits": 0, "u8_pixels": 0, "u8_maxdiff": 0, "gpu_values": 0}
    for dt in (np.float32, np.float64):
        for scale in (1.0, 1.1, 1.2):
            bx = boxes.astype(dt).astype(np.float64)                 # numpy 1.18: float32 box * Python float promotes to float64
            crops = []
            for (cx, cy, w, h) in bx:
                src, dst = crop_np.patch_points(cx, cy, w, h, 224, scale)
                M = cv2.getAffineTransform(np.float32(src), np.float32(dst))
                worst["matrix_bits"] += int((np.asarray(M, np.float64) != crop_np.get_affine_transform_cv(src, dst)).sum())
                crops.append(cv2.warpAffine(frame.copy(), M, (224, 224), flags=cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT))
            ref = np.stack(crops)
            mine = crop_np.crop_u8_np(frame, bx, scale)
            d = np.abs(ref.astype(np.int32) - mine.astype(np.int32))
            worst["u8_pixels"] += int((d > 0).sum())
            worst["u8_maxdiff"] = max(worst["u8_maxdiff"], int(d.max()))
            if device is not None:
                import torch
                from poco_amd.tester import crop_normalize
                out = crop_normalize(torch.from_numpy(frame).to(device), torch.from_numpy(boxes.astype(dt)).to(device), scale)
                worst["gpu_values"] += int((out.cpu().numpy() != crop_np.normalize_np(ref)).sum())
    return worst


def stage_crop(args):
    try:
        import cv2
    except Exception as e:                                     # noqa: BLE001
        return SKIP, f"cv2 is not importable ({type(e).__name__}); the reference pins opencv-python==4.5.5.64"
    dev = None
    try:
        import torch
        if torch.cuda.is_available():
            dev = args.device
    except Exception:                                          # noqa: BLE001
        pass
    w = crop_against_cv2(cv2, device=dev)
    msg = (f"cv2 {cv2.__version__}: 384 crops; getAffineTransform entries differing {w['matrix_bits']}, uint8 pixels differing "
           f"{w['u8_pixels']} (max {w['u8_maxdiff']} grey levels)" + (f", HIP kernel values differing {w['gpu_values']}" if dev else " (no GPU: HIP kernel not compared)"))
    ok = w["u8_pixels"] == 0 and w["gpu_values"] == 0
    if not ok and not cv2.__version__.startswith("4.5"):
        msg += " - note: OpenCV >= 4.11 ships a different (floating-point) warpAffine; the reference pins 4.5.5.64"
    return (OK if ok else FAIL), msg


def dataset_crop_against_cv2(cv2, n: int = 48, seed: int = 0):
    """The reference's crop_cv2 arithmetic on the real cv2 (float32 image, image_utils.py:189-206) and rot_aa (cv2.Rodrigues, :236-247)
    vs tests/datacrop_np.py.  `cv2` is passed in, as for crop_against_cv2."""
    from tests import datacrop_np as dn
    from oracle import crop_np
    r = np.random.default_rng(seed)
    frame = r.integers(0, 256, (270, 480, 3), dtype=np.uint8)
    worst = {"values": 0, "maxdiff": 0.0, "rot_aa": 0.0}
    for i in range(n):
        center, scale = (r.uniform(-30, 510), r.uniform(-30, 300)), r.uniform(0.1, 2.0)
        rot, res = [0.0, 30.0, -47.5, 90.0, 180.0, r.uniform(-60, 60)][i % 6], (32, 224)[i % 2]
        c_x, c_y, bb = dn.py_round(center[0]), dn.py_round(center[1]), dn.py_round(scale * 200.0)
        src, dst = dn.patch_points(c_x, c_y, bb, res, rot)
        M = cv2.getAffineTransform(np.float32(src), np.float32(dst))
        ref = cv2.warpAffine(frame.astype(np.float32), M, (res, res), flags=cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT)
        mine = dn.warp_affine_f32(frame, crop_np.get_affine_transform_cv(src, dst), res)
        worst["values"] += int((ref != mine).sum())
        worst["maxdiff"] = max(worst["maxdiff"], float(np.abs(ref - mine).max()))
        aa = 0.8 * r.standard_normal(3)
        a = np.deg2rad(-rot)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        want = cv2.Rodrigues(np.dot(R, cv2.Rodrigues(aa)[0]))[0].T[0]
        worst["rot_aa"] = max(worst["rot_aa"], float(np.abs(want - dn.rot_aa_np(aa, rot)).max()))
    return worst


def stage_dataset_crop(args):
    try:
        import cv2
    except Exception as e:                                     # noqa: BLE001
        return SKIP, f"cv2 is not importable ({type(e).__name__}); the dataset crop stays pinned to the restatement only"
    w = dataset_crop_against_cv2(cv2)
    msg = (f"cv2 {cv2.__version__}: 48 float crops; values differing {w['values']} (max {w['maxdiff']:.3g}), rot_aa max deviation "
           f"{w['rot_aa']:.2e}")
    ok = w["values"] == 0 and w["rot_aa"] < 1e-9
    if not ok and not cv2.__version__.startswith("4.5"):
        msg += " - note: OpenCV >= 4.11 ships a different (floating-point) warpAffine; the reference pins 4.5.5.64"
    return (OK if ok else FAIL), msg


def occlusion_against_cv2(cv2, seed: int = 0):
    """The restated cv2.resize(uint8 RGBA, INTER_AREA) of tests/occlude_np.py against the real one over every path (copy, integer
    blocks, generic, mixed axes), and whole occluded crops against the reference's arithmetic on the real cv2: crop_cv2's warp on
    float32, then resize_by_factor and paste_over per drawn object (pocolib/dataset/occlusion.py:247-288, restated call for call so
    that the reference tree is not needed).  Returns the numbers of differing bytes / float values."""
    from tests import datacrop_np as dn, occlude_cases, occlude_np as on
    from oracle import crop_np
    r = np.random.default_rng(seed)
    cuts = occlude_cases.cutouts() + [r.integers(0, 256, (int(h), int(w), 4), dtype=np.uint8) for h, w in r.integers(20, 200, (6, 2))]
    out = {"resizes": 0, "resize_bytes": 0, "resize_max": 0, "crops": 0, "crop_values": 0}
    for c in cuts:
        h, w = c.shape[:2]
        sizes = {(w, h), (max(w // 2, 1), max(h // 2, 1)), (max(w // 3, 1), max(h // 3, 1)), (max(w // 2, 1), max(int(h / 3.2), 1)), (1, 1)}
        sizes |= {(max(int(round(w * f)), 1), max(int(round(h * f)), 1)) for f in r.uniform(0.175, 0.875, 12)}
        for dw, dh in sorted(sizes):
            ref, mine = cv2.resize(c, (dw, dh), interpolation=cv2.INTER_AREA), on.resize_area(c, (dw, dh))
            d = np.abs(ref.astype(np.int32) - mine.astype(np.int32))
            out["resizes"] += 1
            out["resize_bytes"] += int((d != 0).sum())
            out["resize_max"] = max(out["resize_max"], int(d.max()))
    frame = r.integers(0, 256, (270, 480, 3), dtype=np.uint8)
    kp = np.concatenate([r.uniform(-0.8, 0.8, (24, 2)), np.ones((24, 1))], 1).astype(np.float32)
    for i in range(8):
        res = (224, 32)[i % 2]
        src, dst = dn.patch_points(240, 135, 200, res, 30.0 * (i % 3))
        crop = cv2.warpAffine(frame.astype(np.float32), cv2.getAffineTransform(np.float32(src), np.float32(dst)), (res, res),
                              flags=cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT)
        np.random.seed(i)
        __import__("random").seed(i)
        objs = on.occlusion_draws_np(kp, 1.0, [c.shape[:2] for c in cuts], res)["objects"]
        ref = crop.copy()
        for oid, dw, dh, cx, cy in objs:
            on.paste_over_np(cv2.resize(cuts[oid], (dw, dh), interpolation=cv2.INTER_AREA), ref, np.array([cx, cy]))
        mine, _ = on.apply_objects_np(dn.warp_affine_f32(frame, crop_np.get_affine_transform_cv(src, dst), res), cuts, objs)
        out["crops"] += 1
        out["crop_values"] += int((ref.view(np.uint32) != mine.view(np.uint32)).sum())
    return out


def stage_occlusion(args):
    try:
        import cv2
    except Exception as e:                                     # noqa: BLE001
        return SKIP, f"cv2 is not importable ({type(e).__name__}); the occluder resize stays pinned to the restatement only"
    w = occlusion_against_cv2(cv2)
    msg = (f"cv2 {cv2.__version__}: {w['resizes']} INTER_AREA resizes, bytes differing {w['resize_bytes']} (max {w['resize_max']} grey "
           f"levels); {w['crops']} occluded crops, float values differing {w['crop_values']}")
    if w["resize_bytes"] and w["resize_max"] <= 1:
        msg += " - one grey level at rounding ties is what a build that fuses the row accumulation (FMA dispatch) gives"
    return (OK if w["resize_bytes"] == 0 and w["crop_values"] == 0 else FAIL), msg


def stage_keypoints(args):
    try:
        import cv2
    except Exception as e:                                     # noqa: BLE001
        return SKIP, f"cv2 is not importable ({type(e).__name__}); the stamp of --draw_keypoints stays unpinned"
    from tests import render_overlay_np as ov
    H, W = 40, 48
    bad = []
    for r in range(ov.disc_table().shape[0]):
        for cx, cy in ((24, 20), (0, 0), (W - 1, H - 1), (2, H - 2), (-3, 7), (W + 2, 5)):
            ref = np.zeros((H, W, 3), np.uint8)
            cv2.circle(ref, (cx, cy), r, (255, 255, 255), -1)
            got = ov.draw_discs_np(np.zeros((H, W, 3), np.uint8), [[cx, cy]], [[255, 255, 255]], r)
            if not np.array_equal(ref, got):
                bad.append((r, cx, cy, int((ref != got).any(-1).sum())))
    r4 = [b for b in bad if b[0] == 4]
    msg = f"cv2 {cv2.__version__}: {len(bad)} of {6 * ov.disc_table().shape[0]} stamps differ" + \
          (f" (radius, cx, cy, pixels): {bad[:6]}" if bad else "") + f"; radius 4 (the demo's): {'differs' if r4 else 'equal'}"
    return (FAIL if r4 else OK), msg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--smpl-pkl", default="data/smpl/SMPL_NEUTRAL.pkl")
    ap.add_argument("--extra", default="data/J_regressor_extra.npy")
    ap.add_argument("--smpl-npz", default=None)
    ap.add_argument("--smpl-dir", default=None, help="directory smplx.SMPL loads from (default: the folder of --smpl-pkl)")
    ap.add_argument("--ckpt", default="data/poco_cliff.pt")
    ap.add_argument("--cfg", default="configs/demo_poco_cliff.yaml")
    ap.add_argument("--inf_model", default="best")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--crop", action="store_true", help="only stage 4: the crop against the real cv2")
    ap.add_argument("--keypoints", action="store_true", help="only stage 5: the keypoint stamp against the real cv2.circle")
    ap.add_argument("--dataset-crop", dest="dataset_crop", action="store_true",
                    help="only stage 6: the dataset crop's restatement (tests/datacrop_np.py) against the real cv2.warpAffine on float32 "
                         "images and cv2.Rodrigues")
    ap.add_argument("--occlusion", action="store_true",
                    help="only stage 7: the synthetic occluders' restatement (tests/occlude_np.py) against the real cv2.resize(INTER_AREA) "
                         "and whole occluded crops; prints the number of differing bytes")
    args = ap.parse_args(argv)
    results = []
    if args.occlusion:
        st, msg = stage_occlusion(args)
        print(f"[{st:7s}] 7 occluders vs cv2: {msg}")
        return 1 if st == FAIL else 0
    if args.dataset_crop:
        st, msg = stage_dataset_crop(args)
        print(f"[{st:7s}] 6 dataset crop vs cv2: {msg}")
        return 1 if st == FAIL else 0
    if args.keypoints:
        st, msg = stage_keypoints(args)
        print(f"[{st:7s}] 5 keypoint stamp vs cv2: {msg}")
        return 1 if st == FAIL else 0
    if args.crop:
        st, msg = stage_crop(args)
        print(f"[{st:7s}] 4 crop vs cv2: {msg}")
        return 1 if st == FAIL else 0
    st, msg, smpl = stage_smpl_file(args)
    results.append(("1 SMPL file", st, msg))
    results.append(("2 LBS vs smplx", *stage_lbs(args, smpl)))
    results.append(("3 checkpoint", *stage_checkpoint(args, smpl)))
    results.append(("4 crop vs cv2", *stage_crop(args)))
    for name, st, msg in results:
        print(f"[{st:7s}] {name}: {msg}")
    return 1 if any(st == FAIL for _, st, _ in results) else 0


if __name__ == "__main__":
    sys.exit(main())
