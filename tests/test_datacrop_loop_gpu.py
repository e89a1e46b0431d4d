"""GPU: the dataset crop in a closed loop, and under eval.py --segm.

Closed loop (resnet50-cliff, synthetic weights): demo.py --save_dataset exports its own predictions as ground truth; eval.py --crop demo
on that file scores zero up to the axis-angle round trip, as tests/test_demo_dataset_gpu.py shows; eval.py --crop dataset cuts the float
crops instead (same integer boxes, no byte rounding), so its error is NOT zero - and how large it is comes from an independent side: the
restatement's two crops (oracle/crop_np.py, tests/datacrop_np.py) through the CPU oracle on the same weights.

--segm (hrnet_w32-pare, synthetic weights): segm.run_eval on EvalDataset(crop='dataset') under rot 30 + flip rasterises the labels from
the host-transformed pose and the `part` keypoints sent through j2d_processing; they equal the labels made by hand from the
restatement's keypoints (datacrop_np.j2d_processing_np) and tests/segm_np.py, and under a pure rotation the rotated ground-truth joints
reproject onto the rotated keypoints."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import crop_np
from poco_amd import datacrop, evaluate, ops, segm, synth
from tests import datacrop_np, eval_np, segm_np, util

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = "configs/demo_poco_cliff_resnet50.yaml"
NAMES = ["im0.png", "im1.png", "im2.png"]
# square boxes whose side is a multiple of 25 at integer centres: scale * 200 is exact and the dataset crop's rounding changes nothing,
# so the two crops differ by the byte rounding of cv2's uint8 path alone
DETS = {"im0.png": [[160, 120, 150, 150]], "im1.png": [[200, 110, 125, 125]], "im2.png": [[150, 100, 200, 200]]}


def _cli(name):
    spec = importlib.util.spec_from_file_location(f"poco_{name}_cli_datacrop_loop", ROOT / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def oracle_mpjpe(ds, frames, crops, dtype):
    """Per-joint MPJPE [N,14] of the CPU oracle (resnet50-cliff, the synthetic weights) on `crops` [N,3,224,224] against the SMPL ground
    truth of the dataset arrays `ds`, everything in `dtype`: the model inputs as EvalDataset.batch builds them."""
    from oracle import poco_ref
    from oracle.smpl_np import smpl_lbs_np
    from poco_amd.tester import calculate_bbox_info, calculate_focal_length
    n = len(ds["imgname"])
    shapes = np.array([frames[str(nm)].shape[:2] for nm in ds["imgname"]], np.float32)
    center, scale = np.asarray(ds["center"], np.float32), np.asarray(ds["scale"], np.float32)
    batch = {"img": crops, "bbox_info": np.stack([calculate_bbox_info(c, s, hw) for c, s, hw in zip(center, scale, shapes)]),
             "focal_length": np.array([calculate_focal_length(h, w) for h, w in shapes], np.float32), "scale": scale, "center": center,
             "orig_shape": shapes}
    cast = lambda d: {k: np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else np.asarray(v) for k, v in d.items()}   # noqa: E731
    smpl = synth.synth_smpl(7)
    sd = poco_ref.to_torch(cast(util.synth_weights("resnet50-cliff")))
    with torch.no_grad():
        out = poco_ref.poco_forward("resnet50-cliff", sd, poco_ref.to_torch(cast(smpl)), poco_ref.to_torch(cast(batch)))
    gt_rot = eval_np.rodrigues(np.asarray(ds["pose"], np.float32).reshape(-1, 3), dtype).reshape(n, 24, 3, 3)
    gt_verts, _ = smpl_lbs_np(smpl, np.asarray(ds["shape"], np.float32), gt_rot)
    y = eval_np.evaluate(out["smpl_vertices"].numpy().astype(dtype), out["pred_pose"].numpy().astype(dtype), out["var_pose"].numpy().astype(dtype),
                         np.asarray(ds["pose"], np.float32), synth.synth_j_regressor_h36m(11), eval_np.joint_map("3dpw"),
                         gt_vertices=gt_verts.astype(dtype), dtype=dtype)
    return np.asarray(y["mpjpe"], np.float64)


def two_crops(ds, frames):
    """The restatement's demo crop and dataset crop of every row: float32 [N,3,224,224] each."""
    side = np.asarray(ds["scale"], np.float32).astype(np.float64) * 200.0
    demo = np.concatenate([crop_np.crop_normalize_np(frames[str(nm)], np.array([[c[0], c[1], s, s]], np.float32))
                           for nm, c, s in zip(ds["imgname"], ds["center"], side)])
    n = len(side)
    data = datacrop_np.dataset_crop_np([frames[str(nm)] for nm in ds["imgname"]], range(n), ds["center"], np.asarray(ds["scale"], np.float64),
                                       np.zeros(n), np.zeros(n, int), np.ones((n, 3)), 224, True)
    return demo, data


def test_closed_loop_demo_crop_scores_zero_dataset_crop_scores_what_the_oracle_says(tmp_path, cuda, capsys):
    """The tolerance is 8 x the oracle's own float32 error on the quantity compared (its float32 result against its float64 result),
    the margin of the other evaluation tests; the reference value is the oracle's float64 result.  Measured on an MI355X: difference up to
    7.6e-05 m, device vs oracle 1.9e-07 m, oracle float32 error 2.3e-07 m (tolerance 1.9e-06 m).  The figures are printed."""
    from PIL import Image
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp_path / "ckpt.pt")
    np.savez(tmp_path / "smpl.npz", **synth.synth_smpl(7))
    np.save(tmp_path / "J.npy", synth.synth_j_regressor_h36m(11))
    (tmp_path / "imgs").mkdir()
    r = np.random.default_rng(0)
    frames = {n: r.integers(0, 256, (240, 320, 3), dtype=np.uint8) for n in NAMES}
    for n in NAMES:
        Image.fromarray(frames[n]).save(tmp_path / "imgs" / n)
    (tmp_path / "dets.json").write_text(json.dumps(DETS))
    demo, ev = _cli("demo"), _cli("eval")
    path = tmp_path / "pseudo.npz"
    # 1. export pseudo ground truth
    demo.main(demo.parse_args(["--cfg", CFG, "--ckpt", str(tmp_path / "ckpt.pt"), "--mode", "folder", "--image_folder", str(tmp_path / "imgs"),
                               "--output_folder", str(tmp_path / "out"), "--batch_size", "8", "--smpl", str(tmp_path / "smpl.npz"),
                               "--detections", str(tmp_path / "dets.json"), "--no_render", "--save_dataset", str(path)]))
    ds = dict(np.load(path, allow_pickle=False))
    assert len(ds["imgname"]) == 3
    common = ["--cfg", CFG, "--ckpt", str(tmp_path / "ckpt.pt"), "--smpl", str(tmp_path / "smpl.npz"), "--j_regressor", str(tmp_path / "J.npy"),
              "--dataset", str(path), "--img_dir", str(tmp_path / "imgs"), "--batch_size", "8"]
    # 2. --crop demo: zero up to the axis-angle round trip, as today
    res_demo = ev.main(ev.parse_args(common + ["--output_folder", str(tmp_path / "e_demo"), "--crop", "demo"]))
    assert res_demo["N"] == 3 and res_demo["val_mpjpe"] < 1e-2 and res_demo["val_v2v"] < 1e-2                  # mm
    # 3. --crop dataset: not zero, and as large as the oracle says
    res_data = ev.main(ev.parse_args(common + ["--output_folder", str(tmp_path / "e_data"), "--crop", "dataset"]))
    capsys.readouterr()
    d_gpu = res_data["mpjpe"].astype(np.float64) - res_demo["mpjpe"].astype(np.float64)
    crops_demo, crops_data = two_crops(ds, frames)
    assert 0 < np.abs(crops_demo - crops_data).max() <= (0.5 + 255 * 6 * 2.0 ** -16) / 255 / 0.224 * (1 + 1e-6)   # the byte rounding alone
    d_or = {dt: oracle_mpjpe(ds, frames, crops_data, dt) - oracle_mpjpe(ds, frames, crops_demo, dt) for dt in (np.float32, np.float64)}
    e_ref = np.abs(d_or[np.float32] - d_or[np.float64]).max()
    dev = np.abs(d_gpu - d_or[np.float64]).max()
    with capsys.disabled():
        print(f"\nclosed loop, per-joint MPJPE(--crop dataset) - MPJPE(--crop demo) in metres: device max {np.abs(d_gpu).max():.3e}, oracle "
              f"float64 max {np.abs(d_or[np.float64]).max():.3e}; device vs oracle {dev:.3e}; the oracle's own float32 error {e_ref:.3e} "
              f"(tolerance 8 x = {8 * e_ref:.3e}); val_mpjpe demo {res_demo['val_mpjpe']:.3e} mm, dataset {res_data['val_mpjpe']:.3e} mm")
    assert np.abs(d_gpu).max() > 0 and res_data["val_mpjpe"] > res_demo["val_mpjpe"]
    assert e_ref > 0 and dev <= 8 * e_ref


# ---- --segm ------------------------------------------------------------------------------------------------------------------------
def _faces():
    """Three large triangles of the synthetic body model, one inside each of the parts 3, 15 and 21 (tests/test_demo_segm_gpu.py)."""
    vp = segm.vertex_parts_from_weights(synth.synth_smpl(7)["lbs_weights"])
    return np.array([np.nonzero(vp == p)[0][:3] for p in (3, 15, 21)], np.int32)


@pytest.fixture(scope="module")
def pare(tmp_path_factory, cuda):
    """A PARE engine, a body model with triangles, and a 3-row dataset whose `part` keypoints are the ground-truth joints seen by a
    camera 40 m in front of the crop (focal 5000, as the reference's crop camera), mapped from crop pixels back into the image."""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("datacrop_segm")
    model = util.make_engine("hrnet_w32-pare", max_batch=4)
    smpl = dict(synth.synth_smpl(7))
    smpl["faces"] = _faces()
    np.savez(tmp / "smpl.npz", **smpl)
    (tmp / "imgs").mkdir()
    r = np.random.default_rng(5)
    names = ["p0.png", "p1.png", "p0.png"]
    for n in set(names):
        Image.fromarray(r.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(tmp / "imgs" / n)
    base = dict(imgname=np.array(names), center=np.array([[160, 120], [140, 110], [170, 100]], np.float32), scale=np.array([0.75, 0.625, 1.0], np.float32),
                pose=(0.3 * r.standard_normal((3, 72))).astype(np.float32), shape=(0.5 * r.standard_normal((3, 10))).astype(np.float32))
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)   # noqa: E731
    _, j49 = model.smpl_lbs(tt(base["shape"]), ops.rodrigues(tt(base["pose"])))
    j = j49[:, 25:49].cpu().numpy().astype(np.float64) + np.array([0.05, -0.03, 40.0])
    crop_px = 5000.0 * j[:, :, :2] / j[:, :, 2:3] + 112.0
    h = 200.0 * base["scale"].astype(np.float64)[:, None, None]
    img_px = (crop_px - 112.0) * h / 224.0 + base["center"].astype(np.float64)[:, None, :]
    base["part"] = np.concatenate([img_px, np.ones((3, 24, 1))], 2).astype(np.float32)
    np.savez(tmp / "ds.npz", **base)
    return tmp, model, smpl, base


def _by_hand(model, smpl, pose, shape, part_px, cuda):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)   # noqa: E731
    gt_verts, gt_j49 = model.smpl_lbs(tt(shape), ops.rodrigues(tt(pose)))
    j24 = gt_j49[:, 25:49].contiguous()
    cam_t = segm.estimate_translation(j24, tt(part_px))
    fparts = segm.face_parts(segm.vertex_parts_from_weights(smpl["lbs_weights"]), smpl["faces"])
    labels = segm_np.part_labels(gt_verts.cpu().numpy(), cam_t.cpu().numpy(), smpl["faces"], fparts)
    return labels, j24.cpu().numpy().astype(np.float64), cam_t.cpu().numpy().astype(np.float64)


def _restated_keypoints(base, rot, flip, sc=1.0):
    k = np.stack([datacrop_np.j2d_processing_np(p, c, sc * float(s), rot, flip) for p, c, s in zip(base["part"], base["center"], base["scale"])])
    k[:, :, :-1] = np.float32(0.5) * np.float32(224) * (k[:, :, :-1] + np.float32(1))          # trainer.py:231-234
    return k


@pytest.mark.parametrize("rot,flip", [(30.0, 1), (30.0, 0), (0.0, 1)])
def test_segm_run_eval_on_the_dataset_crop(pare, cuda, rot, flip):
    tmp, model, smpl, base = pare
    J = synth.synth_j_regressor_h36m(11)
    ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=datacrop.AugSpec(rot=rot, flip=bool(flip)))
    res = segm.run_eval(model, ds, str(tmp / "ds.npz"), J, str(tmp / "smpl.npz"), batch_size=2, return_labels=True)
    assert res["segm_N"] == 3 and res["segm_labels"].shape == (3, 224, 224) and np.isfinite(res["val_segm_ce"])
    # the keypoints: EvalDataset.part_keypoints == the restatement's j2d_processing, bit for bit
    kp = _restated_keypoints(base, rot, flip)
    assert np.array_equal(ds.part_keypoints(base["part"]).view(np.uint32), kp.view(np.uint32))
    # the pose: the restatement's pose_processing up to the float32 rounding of a float64 result
    want_pose = np.stack([datacrop_np.pose_processing_np(p, rot, flip) if rot else datacrop_np.flip_pose_np(p) for p in base["pose"]])
    assert np.abs(ds.pose - want_pose).max() <= 2.0 ** -22 and not np.array_equal(ds.pose, base["pose"])
    # the labels: by hand from the restated keypoints and the transformed pose, rasterised by tests/segm_np.py
    labels, j24, cam_t = _by_hand(model, smpl, ds.pose, base["shape"], kp, cuda)
    assert np.array_equal(res["segm_labels"], labels)
    assert (labels != 0).mean() > 0.005 and len(np.unique(labels)) > 2                      # the mesh is in the picture
    plain, _, _ = _by_hand(model, smpl, base["pose"], base["shape"], _restated_keypoints(base, 0.0, 0), cuda)
    assert not np.array_equal(labels, plain)
    if not flip:
        # geometry: rot_aa turns the body the way get_transform turns the keypoints.  The rotated joints, seen from the estimated
        # camera, land on the rotated keypoints up to transform()'s truncation (+1, then at most one pixel down) and the least-squares
        # fit over 24 of them; a wrong sign at 30 degrees would be tens of pixels.  (The flip cannot be checked this way: the synthetic
        # body is not mirror-symmetric.)
        p = j24 + cam_t[:, None, :]
        reproj = 5000.0 * p[:, :, :2] / p[:, :, 2:3] + 112.0
        d = np.abs(reproj - kp[:, :, :2].astype(np.float64)).max()
        print(f"rot {rot}: reprojection of the rotated joints vs the rotated keypoints: max {d:.3f} px")
        assert d <= 2.0
