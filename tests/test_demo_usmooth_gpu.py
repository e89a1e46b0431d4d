"""GPU: demo.py --mode video --smooth_uncert end to end on the smallest variant (resnet50-cliff, synthetic weights and body model as
in tests/test_demo_infill_gpu.py): a clip of 70 noise frames of 96 x 128 with two box tracks, one of 70 rows and one of 20 rows on
every second frame (holes in the frame indices).

The smoothed file is checked against usmooth.smooth_tracks applied to the file's own pose_net / betas_net / orig_cam_net / var /
frame_ids (the same operator on the same rows: the same bits) and against tests/usmooth_np.py, its meshes against the LBS operator,
and everything the smoother must not touch against the run without the flag."""
import json

import numpy as np
import pytest
import torch

from poco_amd import synth, usmooth
from tests import usmooth_np as unp, util

pytestmark = pytest.mark.gpu
T, H, W = 70, 96, 128
LAM = 10.0
NEW_KEYS = ("smooth_shift", "pose_net", "betas_net", "orig_cam_net")
LBS_TOL = 2e-5                # tests/test_model_gpu.py::test_smpl_lbs_op: the LBS operator against its float64 restatement


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("usmooth")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    fr = tmp / "frames"
    fr.mkdir()
    r = np.random.default_rng(4)
    for i in range(T):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(fr / f"{i:06d}.png")
    f0, f1 = np.arange(T), np.arange(6, 46, 2)                                   # 70 rows; 20 rows with holes
    box = lambda cx, f: np.stack([cx + 0.25 * f, 48 + 0.1 * f, 60 + 0 * f, 60 + 0 * f], 1)        # noqa: E731
    tracks = {"0": {"bbox": box(36.0, f0).tolist(), "frames": f0.tolist()}, "1": {"bbox": box(80.0, f1).tolist(), "frames": f1.tolist()}}
    (tmp / "tracks.json").write_text(json.dumps(tracks))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video", "--vid_file", str(fr),
              "--batch_size", "32", "--smpl", str(tmp / "smpl.npz"), "--tracking", str(tmp / "tracks.json"), "--no_render"]

    def run(name, flags=()):
        import demo
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp / name), *flags]))
        return dict(np.load(tmp / name / "frames_" / "poco_results.npz"))
    return run


@pytest.fixture(scope="module")
def plain(case):
    return case("plain")


@pytest.fixture(scope="module")
def u_ref(plain):
    return float(np.median(np.concatenate([plain["0/var"].ravel(), plain["1/var"].ravel()])))


@pytest.fixture(scope="module")
def smoothed(case, u_ref):
    return case("smoothed", ["--smooth_uncert", repr(LAM), "--smooth_uncert_ref", repr(u_ref)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_run_without_the_flag_gives_what_it_gives_today(plain):
    assert {k.split("/")[0] for k in plain} == {"0", "1"} and not any(k.split("/")[1] in NEW_KEYS for k in plain)
    assert plain["0/pose"].shape == (T, 24, 3, 3) and plain["1/pose"].shape == (20, 24, 3, 3)


def test_smoothed_file_is_smooth_tracks_on_its_own_net_values(plain, smoothed, u_ref, cuda):
    model = util.make_engine("resnet50-cliff", max_batch=T)
    tracks = {}
    for pid in ("0", "1"):
        g = lambda k: smoothed[f"{pid}/{k}"]                                     # noqa: E731
        for k in NEW_KEYS:
            assert f"{pid}/{k}" in smoothed, k
        n = len(g("frame_ids"))
        assert g("smooth_shift").shape == (n, 24) and g("smooth_shift").dtype == np.float32
        # what the smoother starts from is the raw prediction, and what it must not touch stays raw
        for net, raw in (("pose_net", "pose"), ("betas_net", "betas"), ("orig_cam_net", "orig_cam")):
            assert np.array_equal(_bits(g(net)), _bits(plain[f"{pid}/{raw}"])), net
        for k in ("var", "var_global", "pred_cam", "smpl_joints2d", "bboxes", "frame_ids"):
            assert np.array_equal(g(k), plain[f"{pid}/{k}"]), k
        tracks[pid] = {"pose": g("pose_net"), "betas": g("betas_net"), "orig_cam": g("orig_cam_net"), "var": g("var"),
                       "frame_ids": g("frame_ids"), "verts": plain[f"{pid}/verts"], "smpl_joints3d": plain[f"{pid}/smpl_joints3d"]}
    again = usmooth.smooth_tracks(model, tracks, LAM, u_ref, 30)
    for pid in ("0", "1"):
        g = lambda k: smoothed[f"{pid}/{k}"]                                     # noqa: E731
        for k in ("pose", "betas", "orig_cam", "smooth_shift"):
            assert np.array_equal(_bits(g(k)), _bits(again[pid][k])), k
        # ... and the restatement on the same rows, to the tolerance of tests/test_usmooth_gpu.py
        n = len(g("frame_ids"))
        lin = np.concatenate([g("betas_net"), g("orig_cam_net")], 1)
        ref = unp.smooth(g("pose_net"), g("var"), g("frame_ids"), np.array([0, n], np.int32), lin, LAM, u_ref, 30)
        got = {"pose": g("pose"), "lin": np.concatenate([g("betas"), g("orig_cam")], 1), "shift": g("smooth_shift")}
        for k in got:
            d_ref = float(np.abs(ref[k + "64"] - ref[k].astype(np.float64)).max())
            assert np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64)).max() <= 8 * d_ref, k
        assert g("smooth_shift").max() > 0.0 and np.abs(g("pose") - g("pose_net")).max() > 0.0        # it did move
        # meshes: every frame re-posed from the smoothed pose and shape
        v, j = model.smpl_lbs(torch.from_numpy(g("betas")).to(cuda), torch.from_numpy(g("pose")).to(cuda))
        assert np.abs(g("verts") - v.cpu().numpy()).max() <= LBS_TOL and np.abs(g("smpl_joints3d") - j.cpu().numpy()).max() <= LBS_TOL
    print(usmooth.summary_line(again, tracks))


def test_after_infill_the_smoother_works_on_the_infilled_pose(case, plain, u_ref, cuda):
    thr = float(np.median(np.concatenate([plain["0/var"][:, 0], plain["1/var"][:, 0]])))
    filled = case("filled", ["--infill", repr(thr), "--infill_max_gap", "8"])
    both = case("both", ["--infill", repr(thr), "--infill_max_gap", "8", "--smooth_uncert", repr(LAM), "--smooth_uncert_ref", repr(u_ref)])
    model = util.make_engine("resnet50-cliff", max_batch=T)
    tracks = {pid: {"pose": filled[f"{pid}/pose"], "betas": filled[f"{pid}/betas"], "orig_cam": filled[f"{pid}/orig_cam"],
                    "var": filled[f"{pid}/var"], "frame_ids": filled[f"{pid}/frame_ids"], "verts": filled[f"{pid}/verts"],
                    "smpl_joints3d": filled[f"{pid}/smpl_joints3d"]} for pid in ("0", "1")}
    want = usmooth.smooth_tracks(model, tracks, LAM, u_ref, 30)
    for pid in ("0", "1"):
        assert np.array_equal(both[f"{pid}/infill"], filled[f"{pid}/infill"])
        for k in ("pose_net", "betas_net", "orig_cam_net", "var"):                # the values before in-filling; var as regressed
            assert np.array_equal(_bits(both[f"{pid}/{k}"]), _bits(filled[f"{pid}/{k}"])), k
        for k in ("pose", "betas", "orig_cam", "smooth_shift"):
            assert np.array_equal(_bits(both[f"{pid}/{k}"]), _bits(want[pid][k])), k
