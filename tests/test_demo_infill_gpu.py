"""GPU: demo.py --mode video --infill end to end on the smallest variant (resnet50-cliff, synthetic weights and body model as in
tests/test_demo_pose_tracks_gpu.py): a clip of 70 noise frames of 96 x 128 with two box tracks, one of 70 rows (more than one
64-row chunk of the in-fill kernel) and one of 20 rows on every second frame (holes in the frame indices).

The threshold is the median of var[:, 0] of a run without the flag, so reliable and unreliable root entries both exist.  The
in-filled file is then checked against tests/infill_np.py applied to the file's own pose_net / betas_net / orig_cam_net / var /
frame_ids under the conditions of tests/test_infill_gpu.py, its meshes against the LBS operator, everything the in-fill must not
touch against the plain run, and --smooth against smooth.one_euro_rotmats of the in-filled pose."""
import json

import numpy as np
import pytest
import torch

from poco_amd import smooth, synth
from tests import infill_np as inp, util

pytestmark = pytest.mark.gpu
T, H, W = 70, 96, 128
GAP = 8
NEW_KEYS = ("infill", "pose_net", "betas_net", "orig_cam_net")
ULP1 = 2.0 ** -23
LBS_TOL = 2e-5                # tests/test_model_gpu.py::test_smpl_lbs_op: the LBS operator against its float64 restatement


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("infill")
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
def thresh(plain):
    return float(np.median(np.concatenate([plain["0/var"][:, 0], plain["1/var"][:, 0]])))


@pytest.fixture(scope="module")
def filled(case, thresh):
    return case("filled", ["--infill", repr(thresh), "--infill_max_gap", str(GAP)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_run_without_the_flag_has_none_of_the_new_keys(plain):
    assert {k.split("/")[0] for k in plain} == {"0", "1"} and not any(k.split("/")[1] in NEW_KEYS for k in plain)
    assert plain["0/pose"].shape == (T, 24, 3, 3) and plain["1/pose"].shape == (20, 24, 3, 3)


def test_infilled_file_matches_the_restatement_on_its_own_inputs(plain, filled, thresh, cuda):
    flags = np.concatenate([filled["0/infill"], filled["1/infill"]])
    assert flags.dtype == np.uint8 and (flags == 0).any() and ((flags == 1) | (flags == 2)).any()      # else this test shows nothing
    assert (flags[:, 0] == 0).any() and (flags[:, 0] != 0).any()                 # the median splits the root entries
    model = util.make_engine("resnet50-cliff", max_batch=T)
    worst = 0.0
    for pid in ("0", "1"):
        g = lambda k: filled[f"{pid}/{k}"]                                       # noqa: E731
        n = len(g("frame_ids"))
        lin = np.concatenate([g("betas_net"), g("orig_cam_net")], 1)
        assert lin.dtype == np.float32 and lin.shape == (n, 14)
        ref = inp.infill(g("pose_net"), g("var"), g("frame_ids"), np.array([0, n], np.int32), lin, np.float32(thresh), GAP)
        f = ref["flags"]
        assert np.array_equal(g("infill"), f)
        exact = f != 1                                                           # flags 0, 3: the input; 2: the anchor row (as the restatement copies it)
        assert np.array_equal(_bits(g("pose"))[exact], _bits(ref["pose"])[exact])
        keep = (f == 0) | (f == 3)
        assert np.array_equal(_bits(g("pose"))[keep], _bits(g("pose_net"))[keep])
        dev = np.abs(g("pose").astype(np.float64) - ref["pose"].astype(np.float64))[f == 1]
        worst = max(worst, float(dev.max()) if dev.size else 0.0)
        assert dev.size == 0 or dev.max() <= ULP1, dev.max()
        got_lin = np.concatenate([g("betas"), g("orig_cam")], 1)
        f0 = f[:, 0]
        assert np.array_equal(_bits(got_lin)[f0 != 1], _bits(ref["lin"])[f0 != 1])
        assert np.array_equal(_bits(got_lin)[(f0 == 0) | (f0 == 3)], _bits(lin)[(f0 == 0) | (f0 == 3)])
        dl = np.abs(got_lin.astype(np.float64) - ref["lin"].astype(np.float64))[f0 == 1]
        assert dl.size == 0 or (dl <= np.spacing(np.abs(ref["lin"][f0 == 1]))).all()
        # what the in-fill starts from is the raw prediction, and what it must not touch stays raw
        for net, raw in (("pose_net", "pose"), ("betas_net", "betas"), ("orig_cam_net", "orig_cam")):
            assert np.array_equal(_bits(g(net)), _bits(plain[f"{pid}/{raw}"])), net
        for k in ("var", "var_global", "pred_cam", "smpl_joints2d", "bboxes", "frame_ids"):
            assert np.array_equal(g(k), plain[f"{pid}/{k}"]), k
        # meshes: touched frames re-posed from the in-filled pose and shape, untouched frames bitwise those of the raw prediction
        touched = ref["touched"].astype(bool)
        assert touched.any() and not touched.all()
        v, j = model.smpl_lbs(torch.from_numpy(g("betas")).to(cuda), torch.from_numpy(g("pose")).to(cuda))
        v, j = v.cpu().numpy(), j.cpu().numpy()
        assert np.abs(g("verts")[touched] - v[touched]).max() <= LBS_TOL and np.abs(g("smpl_joints3d")[touched] - j[touched]).max() <= LBS_TOL
        assert np.abs(g("verts")[touched] - plain[f"{pid}/verts"][touched]).max() > 1e-3              # they did move
        for k in ("verts", "smpl_joints3d"):
            assert np.array_equal(_bits(g(k))[~touched], _bits(plain[f"{pid}/{k}"])[~touched]), k
    print(f"demo --infill {thresh:.6g}: flags {np.bincount(flags.ravel(), minlength=4).tolist()}, largest deviation {worst / ULP1:.3f} ulp(1.0)")


def test_smooth_filters_the_infilled_pose(case, filled, thresh):
    both = case("smooth", ["--infill", repr(thresh), "--infill_max_gap", str(GAP), "--smooth"])
    for pid in ("0", "1"):
        assert np.array_equal(both[f"{pid}/infill"], filled[f"{pid}/infill"])
        assert np.array_equal(_bits(both[f"{pid}/pose"]), _bits(smooth.one_euro_rotmats(filled[f"{pid}/pose"], 0.004, 1.5)))
        for k in ("pose_net", "betas", "orig_cam", "var", "smpl_joints2d"):
            assert np.array_equal(_bits(both[f"{pid}/{k}"]), _bits(filled[f"{pid}/{k}"])), k
