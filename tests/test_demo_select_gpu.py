"""GPU: demo.py --cfg2 --ckpt2 end to end with synthetic weights and body model (as tests/test_demo_infill_gpu.py builds them).

(a) folder mode, two resnet50-cliff checkpoints (seeds 0 and 1) on five 96 x 128 noise images with two boxes each: model 1 alone,
    model 2 alone and the pair; --select_scale is the median of the solo runs' score ratio, so both choices occur.
(b) folder mode with hrnet_w32-pare as the second model: the mean rule scores its rows, their 2-D joints are converted per row.
(c) video mode, --select joint, on a 12-frame clip with two tracks: mixed rows are re-posed, unmixed rows are a solo run's; the scale
    is chosen so that both kinds of row occur, and every rotation is compared with its joint's model as well.
(d) of the issue, eval.py with a second model, is tests/test_eval_select_gpu.py.
Rows of the pair's file equal the rows of the solo file its `select` names bit for bit (the engine is bitwise
repeatable), and `select` equals tests/select_np.py applied to the solo files' own var_pose-derived inputs."""
import json

import numpy as np
import pytest
import torch

from poco_amd import postproc, synth
from tests import select_np as snp, util

pytestmark = pytest.mark.gpu
H, W, NIMG, T = 96, 128, 5, 12
NEW_KEYS = ("select", "select_score")
LBS_TOL = 2e-5                # tests/test_model_gpu.py::test_smpl_lbs_op: the LBS operator against its float64 restatement
CFG = {"resnet50-cliff": "configs/demo_poco_cliff_resnet50.yaml", "hrnet_w32-pare": "configs/demo_poco_pare.yaml"}
ROW_KEYS = ("pred_cam", "orig_cam", "verts", "pose", "betas", "joints3d", "smpl_joints2d", "bboxes")


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("select")
    for name, variant, seed in (("m1", "resnet50-cliff", 0), ("m2", "resnet50-cliff", 1), ("pare", "hrnet_w32-pare", 0)):
        w = util.synth_weights(variant, seed)
        torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / f"{name}.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    r = np.random.default_rng(6)
    (tmp / "imgs").mkdir()
    (tmp / "frames").mkdir()
    dets = {}
    for i in range(NIMG):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp / "imgs" / f"{i:03d}.png")
        dets[f"{i:03d}.png"] = [[40.0 + 3 * i, 48.0, 60.0, 60.0], [84.0 - 2 * i, 50.0, 56.0, 64.0]]
    for i in range(T):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp / "frames" / f"{i:06d}.png")
    (tmp / "dets.json").write_text(json.dumps(dets))
    f = np.arange(T)
    box = lambda cx: np.stack([cx + 0.5 * f, 48 + 0.2 * f, 60 + 0 * f, 60 + 0 * f], 1).tolist()            # noqa: E731
    (tmp / "tracks.json").write_text(json.dumps({"0": {"bbox": box(36.0), "frames": f.tolist()}, "1": {"bbox": box(80.0), "frames": f.tolist()}}))
    cache = {}

    def run(name, model, flags=(), video=False):
        """model: (variant, checkpoint name); the result of a run is kept by name."""
        if name not in cache:
            import demo
            src = ["--mode", "video", "--vid_file", str(tmp / "frames"), "--tracking", str(tmp / "tracks.json")] if video else \
                  ["--mode", "folder", "--image_folder", str(tmp / "imgs"), "--detections", str(tmp / "dets.json")]
            demo.main(demo.parse_args(["--cfg", CFG[model[0]], "--ckpt", str(tmp / f"{model[1]}.pt"), "--batch_size", "8", "--smpl",
                                       str(tmp / "smpl.npz"), "--no_render", "--output_folder", str(tmp / name), *src, *flags]))
            if video:
                cache[name] = dict(np.load(tmp / name / "frames_" / "poco_results.npz"))
            else:
                files = [dict(np.load(tmp / name / "imgs_" / f"{i:03d}_poco.npz")) for i in range(NIMG)]
                cache[name] = {k: np.concatenate([f[k] for f in files]) for k in files[0]}
        return cache[name]
    run.second = lambda model: ["--cfg2", CFG[model[0]], "--ckpt2", str(tmp / f"{model[1]}.pt")]
    return run


M1, M2, PARE = ("resnet50-cliff", "m1"), ("resnet50-cliff", "m2"), ("hrnet_w32-pare", "pare")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _scale(a, b, kinds):
    """The median ratio of the two solo runs' crop scores: about half of the crops go to either model."""
    s = lambda v, k: np.array([snp.crop_score(row, k, 0.40) for row in v])                         # noqa: E731
    return float(np.median(s(a["var"], kinds[0]) / s(b["var"], kinds[1])))


def _expected_select(a, b, kinds, scale, mode):
    """tests/select_np.py on the solo files' own inputs: their `var` is the processed uncertainty, so kinematic is off here."""
    z = np.zeros((len(a["var"]), 24, 3, 3), np.float32)
    return snp.select(z, a["var"], kinds[0], z, b["var"], kinds[1], False, 0.40, scale, mode)


def test_a_run_without_the_flags_has_none_of_the_new_keys(case):
    solo = case("solo1", M1)
    assert not any(k in solo for k in NEW_KEYS) and solo["pose"].shape == (2 * NIMG, 24, 3, 3)


def test_folder_mode_rows_are_the_rows_of_the_model_select_names(case):
    a, b = case("solo1", M1), case("solo2", M2)
    scale = _scale(a, b, (1, 1))
    p = case("pair", M1, case.second(M2) + ["--select_scale", repr(scale)])
    sel = p["select"]
    assert sel.dtype == np.uint8 and sel.shape == (2 * NIMG, 24) and p["select_score"].shape == (2 * NIMG, 2)
    root = sel[:, 0] == 1
    assert root.any() and not root.all() and (sel == sel[:, :1]).all()                 # both choices occur; crop mode never mixes
    ref = _expected_select(a, b, (1, 1), scale, 0)
    assert np.array_equal(sel, ref["choice"]) and np.array_equal(_bits(p["select_score"]), _bits(ref["score"]))
    assert set(p) == set(a) | set(NEW_KEYS)
    for k in a:
        assert np.array_equal(_bits(p[k]), _bits(np.where(root.reshape((-1,) + (1,) * (a[k].ndim - 1)), b[k], a[k]))), k


def test_folder_mode_with_a_pare_second_model_follows_its_rules_per_row(case):
    a, b = case("solo1", M1), case("solo_pare", PARE)
    scale = _scale(a, b, (1, 0))
    p = case("pair_pare", M1, case.second(PARE) + ["--select_scale", repr(scale)])
    root = p["select"][:, 0] == 1
    assert root.any() and not root.all()
    ref = _expected_select(a, b, (1, 0), scale, 0)                                       # the mean rule scores model 2's rows
    assert np.array_equal(p["select"], ref["choice"]) and np.array_equal(_bits(p["select_score"]), _bits(ref["score"]))
    for k in ROW_KEYS + ("var",):
        assert np.array_equal(_bits(p[k]), _bits(np.where(root.reshape((-1,) + (1,) * (a[k].ndim - 1)), b[k], a[k]))), k
    # the PARE rows' 2-D joints are the PARE solo run's converted ones (pixels of the original image, not crop coordinates)
    assert np.array_equal(_bits(p["smpl_joints2d"][root]), _bits(b["smpl_joints2d"][root])) and np.abs(b["smpl_joints2d"][..., :2]).max() > 2
    # var_global follows the chosen model's rule per row
    want = np.where(root, postproc.global_uncert(p["var"], PARE[0]), postproc.global_uncert(p["var"], M1[0]))
    assert np.array_equal(_bits(p["var_global"]), _bits(want))
    assert np.array_equal(_bits(p["var_global"]), _bits(np.where(root, b["var_global"], a["var_global"])))


def test_video_mode_joint_selection_reposes_the_mixed_rows(case, cuda):
    a, b = case("v1", M1, video=True), case("v2", M2, video=True)
    # entry (t, j) takes model 2 iff scale < u_1[t,j] / u_2[t,j]: with the median over the 24 rows of the row's smallest ratio, half of
    # the rows lie wholly above the scale (all 24 joints from model 2, unmixed) and the others have joints on both sides (mixed)
    ratio = np.concatenate([a[f"{pid}/var"].astype(np.float64) / b[f"{pid}/var"] for pid in ("0", "1")])
    scale = float(np.median(ratio.min(axis=1)))
    p = case("vpair", M1, case.second(M2) + ["--select", "joint", "--select_scale", repr(scale)], video=True)
    model = util.make_engine("resnet50-cliff", max_batch=T)
    nmixed = nwhole = 0
    for pid in ("0", "1"):
        g = lambda k: p[f"{pid}/{k}"]                                                    # noqa: E731
        sa = {k.split("/")[1]: v for k, v in a.items() if k.startswith(pid + "/")}
        sb = {k.split("/")[1]: v for k, v in b.items() if k.startswith(pid + "/")}
        sel = g("select")
        assert sel.shape == (T, 24) and sel.dtype == np.uint8 and g("select_score").shape == (T, 2)
        ref = _expected_select(sa, sb, (1, 1), scale, 1)
        assert np.array_equal(sel, ref["choice"]) and np.array_equal(_bits(g("select_score")), _bits(ref["score"]))
        mixed = ref["mixed"].astype(bool)
        nmixed += int(mixed.sum())
        nwhole += int((~mixed).sum())
        root = sel[:, 0] == 1
        for k in sa:                                                                     # unmixed rows: a solo run's, bit for bit
            if sa[k].dtype.kind != "f" or k in ("var", "var_global"):
                continue
            want = np.where(root.reshape((-1,) + (1,) * (sa[k].ndim - 1)), sb[k], sa[k])
            assert np.array_equal(_bits(g(k))[~mixed], _bits(want)[~mixed]), k
        # every rotation from the model chosen for its joint; shape and camera from the root's model, also in mixed rows
        assert np.array_equal(_bits(g("pose")), _bits(np.where(sel[:, :, None, None] == 1, sb["pose"], sa["pose"])))
        for k in ("betas", "pred_cam", "orig_cam", "smpl_joints2d"):
            assert np.array_equal(_bits(g(k)), _bits(np.where(root.reshape((-1,) + (1,) * (sa[k].ndim - 1)), sb[k], sa[k]))), k
        v, j = model.smpl_lbs(torch.from_numpy(g("betas")).to(cuda), torch.from_numpy(g("pose")).to(cuda))
        assert np.abs(g("verts") - v.cpu().numpy())[mixed].max(initial=0) <= LBS_TOL
        assert np.abs(g("smpl_joints3d") - j.cpu().numpy())[mixed].max(initial=0) <= LBS_TOL
    assert nmixed > 0 and nwhole > 0                         # else the mesh check / the unmixed rows' comparison shows nothing
