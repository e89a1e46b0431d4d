"""GPU: eval.py --visibility end to end on the small synthetic dataset and mesh of tests/test_demo_segm_gpu.py (synthetic PARE weights, a
synthetic body model with three triangles, the dataset demo.py --save_dataset wrote), built again here: run_eval with the visibility
step on the demo crop, on the flipped dataset crop and under synthetic occluders gives the counts of the numpy restatement
(tests/visibility_np.py) run on the same ground truth and masks, and the statistics of its restatement; without the step the result
is what it was; an occluder placed over one part lowers that joint's vis_obj and leaves the others at 1; the command line runs once."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import datacrop, evaluate, ops, segm, synth, visibility
from tests import occlude_cases, occlude_np, segm_np, util, visibility_np

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = "configs/demo_poco_pare.yaml"
NAMES = ["im0.png", "im1.png"]
# square boxes whose side is a multiple of 25: scale = side / 200 and scale * 200 are exact (tests/test_demo_segm_gpu.py)
DETS = {"im0.png": [[160, 120, 150, 150], [90, 100, 100, 100]], "im1.png": [[200, 110, 125, 125]]}
N = 3
VIS_KEYS = set(visibility.NPZ_KEYS) | {"vis_stats", "vis_margin"}


def _faces():
    """Three large triangles of the synthetic body model, one inside each of the parts 3, 15 and 21 (tests/test_demo_segm_gpu.py)."""
    vp = segm.vertex_parts_from_weights(synth.synth_smpl(7)["lbs_weights"])
    return np.array([np.nonzero(vp == p)[0][:3] for p in (3, 15, 21)], np.int32)


def _cli(name):
    spec = importlib.util.spec_from_file_location(f"poco_{name}_cli_visibility_gpu", ROOT / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _demo_args(files, *extra):
    return ["--cfg", CFG, "--ckpt", str(files / "ckpt.pt"), "--mode", "folder", "--image_folder", str(files / "imgs"),
            "--output_folder", str(files / "out"), "--batch_size", "4", "--smpl", str(files / "smpl.npz"),
            "--detections", str(files / "dets.json"), "--no_render", *extra]


@pytest.fixture(scope="module")
def world(tmp_path_factory, cuda):
    """(folder, engine, body-model arrays, face parts, J regressor): the dataset is written by demo.py --save_dataset once."""
    from PIL import Image
    from poco_amd.tester import POCOTester
    tmp = tmp_path_factory.mktemp("visibility")
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
    np.savez(tmp / "occ.npz", **{f"c{i}": c for i, c in enumerate(occlude_cases.cutouts())})
    demo = _cli("demo")
    demo.main(demo.parse_args(_demo_args(tmp, "--save_dataset", str(tmp / "pseudo.npz"))))
    model = POCOTester(demo.parse_args(_demo_args(tmp))).model
    fparts = segm.face_parts(segm.vertex_parts_from_weights(smpl["lbs_weights"]), smpl["faces"])
    return tmp, model, smpl, fparts, synth.synth_j_regressor_h36m(11)


def _dataset(tmp, **kw):
    return evaluate.EvalDataset(str(tmp / "pseudo.npz"), str(tmp / "imgs"), **kw)


def _ground_truth(model, ds, tmp):
    """(gt_verts [N,V,3], cam_t [N,3]) as numpy, by hand from the operators, in batches of 2 as the runs below."""
    dev = model.device
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
    raw = np.load(tmp / "pseudo.npz")["part"]
    part = ds.part_keypoints(raw) if ds.crop == "dataset" else segm_np.crop_keypoints24(raw, ds.center, ds.scale)
    verts, cams = [], []
    for lo, hi in ((0, 2), (2, 3)):
        gv, gj = model.smpl_lbs(tt(ds.shape[lo:hi]), ops.rodrigues(tt(ds.pose[lo:hi])))
        cams.append(ops.estimate_translation(gj[:, 25:49].contiguous(), tt(part[lo:hi])).cpu().numpy())
        verts.append(gv.cpu().numpy())
    return np.concatenate(verts), np.concatenate(cams)


def _masks(ds):
    """The restatement's alpha > 0 maps of the dataset's occluder records."""
    cuts, zero = ds.occlude.occluders, np.zeros((224, 224, 3), np.float32)
    objs = [[tuple(int(v) for v in ds.occ_records["obj"][n, k].tolist()) for k in range(int(ds.occ_records["count"][n]))] for n in range(len(ds))]
    return np.stack([occlude_np.apply_objects_np(zero, cuts, o)[1] for o in objs]).astype(np.uint8)


def _run(world, ds, with_visibility=True, margin=None):
    tmp, model, smpl, fparts, J = world
    vs = visibility.prepare(model, ds, str(tmp / "pseudo.npz"), str(tmp / "smpl.npz"), batch_size=2, margin=margin) if with_visibility else None
    return evaluate.run_eval(model, ds, J, batch_size=2, visibility=vs) if with_visibility else evaluate.run_eval(model, ds, J, batch_size=2)


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("variant", ["demo_crop", "flip", "occlude"])
def test_run_eval_counts_equal_the_restatement(world, variant):
    tmp, model, smpl, fparts, J = world
    kw = {"demo_crop": {}, "flip": dict(crop="dataset", augment=datacrop.AugSpec(flip=True)),
          "occlude": dict(crop="dataset", occlude=datacrop.OcclusionSpec(occlude_cases.cutouts(), seed=5))}[variant]
    ds = _dataset(tmp, **kw)
    res = _run(world, ds)
    assert VIS_KEYS <= set(res) and res["vis_counts"].shape == (N, 24, 4) and res["vis_counts"].dtype == np.int32
    gt_verts, cam_t = _ground_truth(model, ds, tmp)
    mask = _masks(ds) if variant == "occlude" else None
    want = visibility_np.part_visibility(gt_verts, cam_t, smpl["faces"], fparts, 5000.0, 224, 112, mask)
    assert np.array_equal(res["vis_counts"], want), np.argwhere(res["vis_counts"] != want)[:6]
    c = res["vis_counts"]
    assert c[:, :, 0].any(axis=1).all() and not np.delete(c, [3, 15, 21], 1).any()             # the three triangles, and nothing else
    if variant == "occlude":
        assert mask.any() and ds.last_occ_mask is not None
        assert np.array_equal(np.rint(ds.occ_cover * 224 * 224), mask.reshape(N, -1).sum(1))
    else:
        assert np.array_equal(c[:, :, 3], c[:, :, 2]) and ds.last_occ_mask is None
    # the statistics are those of the restatement, from the evaluator's own per-joint uncertainty and error
    st, ref = res["vis_stats"], visibility_np.statistics(want, res["corr_y"].reshape(N, 24), res["corr_x"].reshape(N, 24))
    assert np.array_equal(res["vis"], visibility_np.ratios(want)["vis"], equal_nan=True) and res["vis"].shape == (N, 24)
    assert (st["valid"], st["invalid"]) == (ref["valid"], ref["invalid"]) and N <= st["valid"] <= 3 * N and st["valid"] + st["invalid"] == 24 * N
    assert st["mean_all"] == pytest.approx(ref["mean_all"], abs=1e-12)
    for k in visibility.COMPONENTS:
        assert np.allclose(st["corr"][k], ref["corr"][k], rtol=0, atol=1e-9, equal_nan=True), k
    assert np.allclose(st["corr_joint"], ref["corr_joint"], rtol=0, atol=1e-9, equal_nan=True)
    assert np.allclose(st["bins"], ref["bins"], rtol=0, atol=1e-12, equal_nan=True) and st["bins"][:, 0].sum() == st["valid"]
    assert res["vis_summary"].shape == (len(visibility.SUMMARY_NAMES),) and res["vis_margin"] == 112
    # without the step the result is what it was: the same keys, the same bits
    plain = _run(world, _dataset(tmp, **kw), with_visibility=False)
    assert set(res) - VIS_KEYS == set(plain) and all(_same(plain[k], res[k]) for k in plain), [k for k in plain if not _same(plain[k], res[k])]


def test_an_occluder_over_one_part_lowers_that_joints_vis_obj_only(world):
    tmp, model, smpl, fparts, J = world
    opaque = np.full((16, 16, 4), 255, np.uint8)
    ds = _dataset(tmp, crop="dataset", occlude=datacrop.OcclusionSpec([opaque], seed=0))
    gt_verts, cam_t = _ground_truth(model, ds, tmp)
    labels = segm_np.part_labels(gt_verts[:1], cam_t[:1], smpl["faces"], fparts)[0]
    target = max((3, 15, 21), key=lambda p: int((labels == p + 1).sum()))
    # an 8 x 8 paste (the 2 x 2 block average of the opaque cut-out: alpha 255) at the place where it covers most of the target's
    # pixels and none of another part's
    best, where = 0, None
    for y in range(0, 224 - 8):
        for x in range(0, 224 - 8):
            blk = labels[y:y + 8, x:x + 8]
            n = int((blk == target + 1).sum())
            if n > best and not ((blk != 0) & (blk != target + 1)).any():
                best, where = n, (x, y)
    assert where is not None and best > 0, "no place where the paste touches the target part alone"
    ds.occ_records = datacrop.occ_records([[(0, 8, 8, where[0] + 4, where[1] + 4)], [], []])   # paste_over starts at centre - size // 2
    res = _run(world, ds)
    want = visibility_np.part_visibility(gt_verts, cam_t, smpl["faces"], fparts, 5000.0, 224, 112, _masks(ds))
    assert np.array_equal(res["vis_counts"], want)
    vo = res["vis_stats"]["vis_obj"]
    c = res["vis_counts"]
    assert c[0, target, 2] - c[0, target, 3] == best and vo[0, target] == (c[0, target, 2] - best) / c[0, target, 2] < 1
    others = np.isfinite(vo)
    others[0, target] = False
    assert others.sum() >= 2 and (vo[others] == 1).all()


def test_command_line_runs_once(world, capsys):
    """eval.py --visibility --segm --aug_occlude --vis_margin 64 --vis_bins 4: the report lines and the .npz keys are there and carry
    the numbers of the result."""
    tmp = world[0]
    ev = _cli("eval")
    capsys.readouterr()
    args = ev.parse_args(["--cfg", CFG, "--ckpt", str(tmp / "ckpt.pt"), "--smpl", str(tmp / "smpl.npz"), "--j_regressor", str(tmp / "J.npy"),
                          "--dataset", str(tmp / "pseudo.npz"), "--img_dir", str(tmp / "imgs"), "--batch_size", "2", "--output_folder",
                          str(tmp / "eval_out"), "--visibility", "--vis_margin", "64", "--vis_bins", "4", "--segm", "--aug_occlude",
                          str(tmp / "occ.npz"), "--aug_seed", "5"])
    res = ev.main(args)
    printed = capsys.readouterr().out.splitlines()
    lines = visibility.report_lines(res)
    assert len(lines) == 10 + 4 and all(line in printed for line in lines)
    assert any(p.startswith("Visibility (window margin 64 px): mean ") for p in printed) and any(p.startswith("Segm mIoU: ") for p in printed)
    assert printed[-1].startswith("Corr(cover, uncertainty): ")                                 # the occluder lines stay last
    z = dict(np.load(tmp / "eval_out" / "evaluation_results_3dpw.npz"))
    assert set(visibility.NPZ_KEYS) <= set(z) and "vis_stats" not in z
    assert z["vis_counts"].shape == (N, 24, 4) and z["vis_counts"].dtype == np.int32 and z["vis"].shape == (N, 24)
    assert np.array_equal(z["vis_counts"], res["vis_counts"]) and z["vis_bins"].shape == (4, 3) and z["vis_joint"].shape == (24, 3)
    assert np.array_equal(z["vis_summary"], res["vis_summary"], equal_nan=True) and z["vis_summary"][-2:].tolist() == [64, 4]
    assert (z["vis_counts"][:, :, 3] <= z["vis_counts"][:, :, 2]).all() and "segm_summary" in z and "occ_cover" in z
