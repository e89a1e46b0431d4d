"""GPU: demo.py --mode folder --tta (resnet50-cliff, synthetic weights, five synthetic images with two detections each).  At batch size 8
and K = 2 a forward takes the views of four crops, so detections of consecutive images share forwards and the view-major batches of
several images are joined per view.  The result files carry tta_spread; their rows are what TTAModel computes from the views of that
image's detections alone (within the project's parity gate of 1e-3: the batch composition differs); var / var_global come from the
fused var_pose; camera and 2-D joints are the base view's, whose crop is the DATASET crop of the box.  Without the flag every array
of every result file is bit for bit what the commit before this feature wrote on the same input (tests/golden/demo_plain_folder.json,
recorded by tools/gen_demo_plain_golden.py)."""
import json

import numpy as np
import pytest
import torch

from poco_amd import postproc, tta
from tests import util
from tools import gen_demo_plain_golden as gold

pytestmark = pytest.mark.gpu
NIMG = gold.NIMG
OLD_KEYS = {"pred_cam", "orig_cam", "verts", "pose", "betas", "joints3d", "bboxes", "smpl_joints2d", "var", "var_global"}
GOLDEN = util.GOLD / "demo_plain_folder.json"


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("demo_tta")
    w, frames, dets = gold.make_inputs(tmp)
    cache = {}

    def run(name, flags=()):
        if name not in cache:
            import demo
            demo.main(demo.parse_args(gold.demo_args(tmp, name, flags)))
            cache[name] = [dict(np.load(tmp / name / "imgs_" / f"{i:03d}_poco.npz")) for i in range(NIMG)]
        return cache[name]
    run.tmp, run.weights, run.frames, run.dets = tmp, w, frames, dets
    return run


def test_without_the_flag_the_files_hold_the_parent_commits_arrays_bit_for_bit(case):
    """tests/golden/demo_plain_folder.json: the sha256 of every array (key, dtype, shape, bytes) of the five result files, recorded
    by tools/gen_demo_plain_golden.py from the commit before --tta existed, on this input.  (The .npz container is not compared: its
    zip entries carry the time of writing.)"""
    files = case("plain_a")
    assert all(set(f) == OLD_KEYS for f in files)
    want = json.loads(GOLDEN.read_text())
    assert sorted(want) == [f"{i:03d}_poco.npz" for i in range(NIMG)]
    assert gold.result_digests(case.tmp, "plain_a") == want


def test_two_runs_without_the_flag_write_the_same_arrays(case):
    case("plain_a"), case("plain_b")
    assert gold.result_digests(case.tmp, "plain_a") == gold.result_digests(case.tmp, "plain_b")


@pytest.mark.parametrize("weight", ["uncert", "uniform"])
def test_folder_mode_writes_the_fused_rows_and_their_spread(case, weight, cuda):
    files = case(f"tta_{weight}", ["--tta", "flip", "--tta_weight", weight])
    plain = case("plain_a")
    model = tta.TTAModel(util.make_engine("resnet50-cliff", max_batch=8, weights=case.weights), tta.parse_views("flip"), weight)
    for i, f in enumerate(files):
        assert set(f) == OLD_KEYS | {"tta_spread"}
        assert f["tta_spread"].shape == (2, 24) and f["tta_spread"].dtype == np.float32 and (f["tta_spread"] > 0).all()
        d = np.float32(case.dets[f"{i:03d}.png"])
        per_view, fused = model.forward_all(tta.frame_batch(torch.from_numpy(case.frames[i]).to(cuda), d, model.views, 224))
        for key, name in (("pose", "pred_pose"), ("betas", "pred_shape"), ("verts", "smpl_vertices"), ("joints3d", "smpl_joints3d"),
                          ("tta_spread", "tta_spread"), ("pred_cam", "pred_cam")):
            assert np.abs(f[key] - fused[name].cpu().numpy()).max() <= 1e-3, (i, key)
        var, var_global = postproc.folder_uncert(fused["var_pose"].cpu(), "resnet50-cliff", True)
        assert np.abs(f["var"] - var).max() <= 1e-3 and np.abs(f["var_global"] - var_global).max() <= 1e-3
        assert np.abs(f["pred_cam"] - per_view[0]["pred_cam"].cpu().numpy()).max() <= 1e-3        # the camera is the base view's
        # every fused rotation is a rotation; the fused rows are not the demo crop's rows
        R = f["pose"].astype(np.float64).reshape(-1, 3, 3)
        assert np.abs(np.einsum("nij,nik->njk", R, R) - np.eye(3)).max() <= 2.0 ** -20 and (np.linalg.det(R) > 0).all()
        assert np.array_equal(f["bboxes"], plain[i]["bboxes"]) and np.abs(f["pose"] - plain[i]["pose"]).max() > 1e-4
