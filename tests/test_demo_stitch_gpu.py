"""GPU: demo.py --mode video --tracker sort --track_stitch end to end on the smallest variant (resnet50-cliff, synthetic weights and
body model as in tests/test_demo_sort_gpu.py): 60 frames of 96 x 128 with two moving people written as a detections file, the second
one missing for 5 frames.  SORT with --track_max_age 1 forgets her and starts a new id when she is back; --track_stitch joins the two
fragments on motion alone (--stitch_shape 0: the synthetic weights' betas carry no identity), the 5 frames of the hole go through the
forward with interpolated boxes, and the written tracking_results_stitched.json gives the same results through --tracking.

Bit for bit: the boxes are float32 on a quarter-pixel lattice (a pickled detections file keeps the dtype, the interpolated rows are
cast to it, the json holds float32 values exactly), and --batch_size 5 divides the 115 own rows, the 5 gap rows and the 120 rows of
the second run, so every forward of both runs has the same batch size; a crop's result does not depend on its neighbours
(tests/test_model_gpu.py), but the tuned conv tiles do depend on the batch size."""
import contextlib
import io
import json
import pickle

import numpy as np
import pytest
import torch

from poco_amd import synth
from tests import util

pytestmark = pytest.mark.gpu
T, H, W = 60, 96, 128
GONE = range(27, 32)                                                            # the frames in which the second person is not detected


def _boxes():
    f = np.arange(T)
    a = np.stack([30 + 0.5 * f, 46 + 0.25 * f, 36 + 0 * f, 60 + 0 * f], 1).astype(np.float32)
    b = np.stack([100 - 0.25 * f, 50 - 0.25 * f, 32 + 0 * f, 56 + 0.25 * (f % 2)], 1).astype(np.float32)
    return a, b


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("demo_stitch")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    fr = tmp / "frames"
    fr.mkdir()
    r = np.random.default_rng(9)
    for i in range(T):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(fr / f"{i:06d}.png")
    a, b = _boxes()
    dets = {f"{i:06d}.png": np.stack([a[i]] + ([b[i]] if i not in GONE else [])) for i in range(T)}
    with open(tmp / "dets.pkl", "wb") as f:
        pickle.dump(dets, f)
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video", "--vid_file", str(fr),
              "--batch_size", "5", "--smpl", str(tmp / "smpl.npz"), "--no_render"]

    def run(name, flags):
        import demo
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            demo.main(demo.parse_args(common + ["--output_folder", str(tmp / name), *flags]))
        return dict(np.load(tmp / name / "frames_" / "poco_results.npz")), out.getvalue()
    run.tmp = tmp
    run.sort = ["--detections", str(tmp / "dets.pkl"), "--tracker", "sort", "--track_max_age", "1", "--track_backfill"]
    return run


@pytest.fixture(scope="module")
def built(case):
    return case("stitch", case.sort + ["--track_stitch", "--stitch_shape", "0"])


def test_two_chains_cover_every_frame(case, built):
    res, log = built
    a, b = _boxes()
    assert {k.split("/")[0] for k in res} == {"0", "1"}
    assert np.array_equal(res["0/frame_ids"], np.arange(T)) and np.array_equal(res["1/frame_ids"], np.arange(T))
    gap = np.isin(np.arange(T), list(GONE))
    assert res["1/stitch"].dtype == np.uint8 and np.array_equal(res["1/stitch"] == 1, gap) and not res["0/stitch"].any()
    assert res["1/stitch_frag"].dtype == np.int32 and res["1/stitch_frag"].tolist() == [0] * 27 + [-1] * 5 + [1] * 28
    assert np.array_equal(res["0/bboxes"], a) and np.array_equal(res["1/bboxes"][~gap], b[~gap])
    assert np.abs(res["1/bboxes"][gap] - b[gap]).max() <= 0.25                    # interpolated between frames 26 and 32 (h alternates)
    assert res["1/pose"].shape == (T, 24, 3, 3) and res["1/verts"].shape == (T, 6890, 3) and np.isfinite(res["1/verts"]).all()
    assert "track_stitch: 3 fragments, 1 links, 2 chains, 5 gap rows, 0 chains dropped" in log
    tr = json.loads((case.tmp / "stitch" / "frames_" / "tracking_results_stitched.json").read_text())
    assert list(tr) == ["0", "1"] and tr["1"]["frames"] == list(range(T)) and tr["1"]["bbox"] == res["1/bboxes"].astype(np.float64).tolist()


def test_without_the_flag_there_are_three_tracks(case):
    res, log = case("plain", case.sort)
    assert {k.split("/")[0] for k in res} == {"0", "1", "2"} and "track_stitch" not in log and "0/stitch" not in res
    assert np.array_equal(res["1/frame_ids"], np.arange(27)) and np.array_equal(res["2/frame_ids"], np.arange(32, T))
    assert not (case.tmp / "plain" / "frames_" / "tracking_results_stitched.json").exists()


def test_the_written_chains_give_the_same_results(case, built):
    res, _ = built
    again, _ = case("reread", ["--tracking", str(case.tmp / "stitch" / "frames_" / "tracking_results_stitched.json")])
    assert set(again) == {k for k in res if not k.endswith(("/stitch", "/stitch_frag"))}
    for pid in ("0", "1"):
        for k in ("pose", "betas", "verts", "var", "orig_cam", "pred_cam"):
            x, y = np.ascontiguousarray(again[f"{pid}/{k}"]), np.ascontiguousarray(res[f"{pid}/{k}"])
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (pid, k)


def test_no_fill_leaves_the_hole(case, built):
    res, log = case("nofill", case.sort + ["--track_stitch", "--stitch_shape", "0", "--stitch_no_fill"])
    keep = np.array([f for f in range(T) if f not in GONE])
    assert {k.split("/")[0] for k in res} == {"0", "1"} and np.array_equal(res["1/frame_ids"], keep) and not res["1/stitch"].any()
    assert res["1/stitch_frag"].tolist() == [0] * 27 + [1] * 28 and "1 links, 2 chains, 0 gap rows" in log
    assert np.array_equal(res["1/pose"], built[0]["1/pose"][keep])                # the own rows are the same forward's


def test_post_processing_sees_one_long_track(case, built):
    res, _ = case("post", case.sort + ["--track_stitch", "--stitch_shape", "0", "--infill", "0.3", "--smooth_uncert", "10"])
    assert res["1/infill"].shape == (T, 24) and res["1/smooth_shift"].shape == (T, 24) and np.isfinite(res["1/pose"]).all()
    assert np.array_equal(res["1/pose_net"], built[0]["1/pose"]) and np.array_equal(res["1/stitch"], built[0]["1/stitch"])


def test_conflicts_end_before_anything_is_written(case):
    with pytest.raises(SystemExit, match="--kp_refit"):
        case("refused", case.sort + ["--track_stitch", "--kp_refit", "1.0"])
    with pytest.raises(SystemExit, match="needs --track_stitch"):
        case("refused", case.sort + ["--stitch_shape", "0"])
    assert not (case.tmp / "refused").exists()
