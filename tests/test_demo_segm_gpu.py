"""GPU: eval.py --segm and demo.py --save_segm end to end on synthetic PARE weights and a synthetic body model (as
tests/test_demo_dataset_gpu.py builds them, plus a few triangles): the dataset demo.py --save_dataset wrote is scored with the same
weights, so the ground-truth mesh is the predicted mesh up to the axis-angle round trip and the keypoint rounding of the reference's
crop transform; the printed numbers equal a SegmAccumulator fed by hand; the pictures equal the restatement's."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import evaluate, ops, segm, synth
from tests import segm_np, util

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = "configs/demo_poco_pare.yaml"
NAMES = ["im0.png", "im1.png"]
# square boxes whose side is a multiple of 25: scale = side / 200 and scale * 200 are exact, so eval.py cuts the very same crops
DETS = {"im0.png": [[160, 120, 150, 150], [90, 100, 100, 100]], "im1.png": [[200, 110, 125, 125]]}
N = 3


def _faces():
    """Three large triangles of the synthetic body model (a cloud of 6890 points), one inside each of the parts 3, 15 and 21: the
    first three vertices whose largest skinning weight is that part's.  Why so few: the reference's crop transform truncates every
    ground-truth keypoint and adds 1 (image_utils.py:111-118), so gt_cam_t puts the ground-truth mesh about half a pixel right of
    and below the predicted one (measured: cam_t - pred_cam_t = +0.0046 m in x and y at Z = 45.4 m, 0.51 pixels).  A half-pixel
    diagonal shift changes about half a pixel per pixel of label boundary, so the agreement the test asserts (>= 0.99 of 50176 pixels)
    needs a fixture whose label boundaries stay under roughly a thousand pixels.  Twelve seeded random triangles of this cloud have
    more (0.988 measured on the device, 0.984 when the shift is applied to the template mesh in numpy); these three have about 700
    (0.995 in the same numpy model, 0.9974 to 0.9976 measured on the device)."""
    from poco_amd import segm as _segm
    vp = _segm.vertex_parts_from_weights(synth.synth_smpl(7)["lbs_weights"])
    return np.array([np.nonzero(vp == p)[0][:3] for p in (3, 15, 21)], np.int32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("segm")
    w = util.synth_weights("hrnet_w32-pare")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "ckpt.pt")
    smpl = dict(synth.synth_smpl(7))
    smpl["faces"] = _faces()
    np.savez(tmp / "smpl.npz", **smpl)
    np.save(tmp / "J.npy", synth.synth_j_regressor_h36m(11))
    (tmp / "imgs").mkdir()
    r = np.random.default_rng(0)
    for n in NAMES:
        Image.fromarray(r.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(tmp / "imgs" / n)
    (tmp / "dets.json").write_text(json.dumps(DETS))
    return tmp


def _cli(name):
    spec = importlib.util.spec_from_file_location(f"poco_{name}_cli_segm_gpu", ROOT / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _demo_args(files, *extra):
    return ["--cfg", CFG, "--ckpt", str(files / "ckpt.pt"), "--mode", "folder", "--image_folder", str(files / "imgs"),
            "--output_folder", str(files / "out"), "--batch_size", "4", "--smpl", str(files / "smpl.npz"),
            "--detections", str(files / "dets.json"), "--no_render", *extra]


def test_save_segm_and_eval_segm_end_to_end(files, cuda, capsys):
    from PIL import Image
    from poco_amd.tester import POCOTester
    demo = _cli("demo")
    path = files / "pseudo.npz"
    demo.main(demo.parse_args(_demo_args(files, "--save_dataset", str(path), "--save_segm")))
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["segm_pictures"] == N and line["dataset_kept"] == N

    # ---- the pictures: one per detection, two 224 x 224 panels; both equal the restatement's ----
    pics = sorted((files / "out" / "imgs_" / "segm").glob("*.png"))
    assert [p.name for p in pics] == ["im0_0.png", "im0_1.png", "im1_0.png"]
    t = POCOTester(demo.parse_args(_demo_args(files)))
    smpl = dict(np.load(files / "smpl.npz"))
    fparts = segm.face_parts(segm.vertex_parts_from_weights(smpl["lbs_weights"]), smpl["faces"])
    pal = segm.palette()
    pred_labels = []
    for name in NAMES:                                                # the forwards the demo made: all detections of an image together
        fr = t.to_device(np.asarray(Image.open(files / "imgs" / name).convert("RGB")))
        boxes = np.asarray(DETS[name], np.float32)
        out = t.model(t.make_batch(fr, boxes), want_segm=True)
        args_ = segm_np.segm_score(out["pred_segm_mask"].cpu().numpy(), np.zeros((len(boxes), 224, 224), np.uint8))[2]
        labs = segm_np.part_labels(out["smpl_vertices"].cpu().numpy(), out["pred_cam_t"].cpu().numpy(), smpl["faces"], fparts)
        for k in range(len(boxes)):
            crop = t.crop_canvas(fr, boxes[k]).cpu().numpy().astype(np.int32)
            pred_labels.append(labs[k])
            got = np.asarray(Image.open(files / "out" / "imgs_" / "segm" / f"{name[:-4]}_{k}.png"))
            assert got.shape == (224, 448, 3) and got.dtype == np.uint8
            assert np.array_equal(got[:, :224], ((crop + pal[args_[k]] + 1) >> 1).astype(np.uint8)), (name, k, "left panel")
            assert np.array_equal(got[:, 224:], ((crop + pal[labs[k]] + 1) >> 1).astype(np.uint8)), (name, k, "right panel")
    pred_labels = np.stack(pred_labels)
    assert (pred_labels != 0).mean() > 0.02 and len(np.unique(pred_labels)) > 3     # the mesh is in the picture, with several parts

    # ---- eval.py --segm on the exported dataset, same weights ----
    ev = _cli("eval")
    args = ev.parse_args(["--cfg", CFG, "--ckpt", str(files / "ckpt.pt"), "--smpl", str(files / "smpl.npz"), "--j_regressor",
                          str(files / "J.npy"), "--dataset", str(path), "--img_dir", str(files / "imgs"), "--batch_size", "2",
                          "--output_folder", str(files / "eval_out"), "--segm", "--save_results"])
    res = ev.main(args)
    printed = capsys.readouterr().out
    for k, word in (("val_segm_ce", "Segm CE"), ("val_segm_pixel_acc", "Segm pixel acc"), ("val_segm_miou", "Segm mIoU")):
        assert f"{word}: {res[k]}" in printed, word
    saved = dict(np.load(files / "eval_out" / "evaluation_results_3dpw.npz"))
    assert saved["segm_counts"].shape == (N, 1 + 3 * 25) and saved["segm_ce"].shape == (N,) and saved["val_segm_iou"].shape == (25,)
    assert np.array_equal(saved["segm_summary"][:3], [res["val_segm_ce"], res["val_segm_pixel_acc"], res["val_segm_miou"]])

    # by hand: the same steps from the operators, in the batches eval.py made
    ds = evaluate.EvalDataset(str(path), str(files / "imgs"))
    dev = t.model.device
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    part = segm_np.crop_keypoints24(np.load(path)["part"], ds.center, ds.scale)
    mesh = segm.PartMesh(smpl["faces"], fparts, dev)
    acc = segm.SegmAccumulator(N)
    gt_labels, cams, pred_cams = [], [], []
    for lo, hi in ((0, 2), (2, 3)):
        out = t.model(ds.batch(lo, hi, dev), want_segm=True)
        gt_verts, gt_j49 = t.model.smpl_lbs(tt(ds.shape[lo:hi]), ops.rodrigues(tt(ds.pose[lo:hi])))
        cam_t = segm.estimate_translation(gt_j49[:, 25:49].contiguous(), tt(part[lo:hi]))
        labels = segm.part_labels(gt_verts, cam_t, mesh)
        acc.step(out["pred_segm_mask"], labels)
        gt_labels.append(labels.cpu().numpy())
        cams.append(cam_t.cpu().numpy())
        pred_cams.append(out["pred_cam_t"].cpu().numpy())
    gt_labels, cams, pred_cams = np.concatenate(gt_labels), np.concatenate(cams), np.concatenate(pred_cams)
    hand = acc.finish(return_records=True)
    for k in ("val_segm_ce", "val_segm_pixel_acc", "val_segm_miou", "val_segm_miou_fg"):
        assert hand[k] == res[k] or (np.isnan(hand[k]) and np.isnan(res[k])), k
    assert np.array_equal(hand["val_segm_iou"], res["val_segm_iou"], equal_nan=True)
    assert np.array_equal(hand["segm_counts"], res["segm_counts"]) and np.array_equal(hand["segm_ce"], res["segm_ce"])

    # the ground-truth labels are the predicted mesh's labels up to the axis-angle round trip
    agree = (gt_labels == pred_labels).mean(axis=(1, 2))
    with capsys.disabled():
        print(f"pixel agreement, ground-truth labels vs labels of the predicted mesh: {agree}; cam_t {cams.tolist()} "
              f"vs pred_cam_t {pred_cams.tolist()}")
    assert np.all(agree >= 0.99), agree


def test_cliff_config_is_refused(files, cuda):
    ev = _cli("eval")
    np.savez(files / "ds_cliff.npz", imgname=np.array(["im0.png"]), center=np.zeros((1, 2)), scale=np.ones(1), pose=np.zeros((1, 72)),
             shape=np.zeros((1, 10)), part=np.zeros((1, 24, 3)))
    args = ev.parse_args(["--cfg", "configs/demo_poco_cliff.yaml", "--ckpt", str(files / "ckpt.pt"), "--smpl", str(files / "smpl.npz"),
                          "--j_regressor", str(files / "J.npy"), "--dataset", str(files / "ds_cliff.npz"), "--segm"])
    with pytest.raises(SystemExit) as e:
        ev.main(args)
    assert e.value.code not in (0, None) and "PARE" in str(e.value.code)
