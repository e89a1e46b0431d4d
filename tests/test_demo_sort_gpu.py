"""GPU: demo.py --mode video --detections FILE --tracker sort end to end on the smallest variant (resnet50-cliff, synthetic weights
and body model as in tests/test_demo_pose_tracks_gpu.py): 40 frames of 96 x 128 with two moving people written as a detections json,
the second entering at frame 6 and listed first.  The tracks are built on the device (poco_amd/sort.py, csrc/sort_tracks.hip) and go
through the unchanged run_on_video: the results equal, bit for bit, a second run that reads the written tracking_results_sort.json
through --tracking, and --infill / --smooth_uncert take the built tracks as they take a file's."""
import json

import numpy as np
import pytest
import torch

from poco_amd import synth
from tests import util

pytestmark = pytest.mark.gpu
T, H, W, LATE = 40, 96, 128, 6


def _boxes():
    """Boxes on a quarter-pixel lattice: exact in float32, so the json's float64 rows and the tracking file's float32 rows are
    the same numbers."""
    f = np.arange(T)
    a = np.stack([30 + 0.5 * f, 46 + 0.25 * f, 36 + 0 * f, 60 + 0 * f], 1).astype(np.float64)
    b = np.stack([100 - 0.25 * f, 50 - 0.25 * f, 32 + 0 * f, 56 + 0.25 * (f % 2)], 1).astype(np.float64)
    return a, b


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("demo_sort")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    fr = tmp / "frames"
    fr.mkdir()
    r = np.random.default_rng(9)
    for i in range(T):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(fr / f"{i:06d}.png")
    a, b = _boxes()
    dets = {f"{i:06d}.png": ([b[i].tolist() + [0.9]] if i >= LATE else []) + [a[i].tolist() + [0.8]] for i in range(T)}
    (tmp / "dets.json").write_text(json.dumps(dets))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video", "--vid_file", str(fr),
              "--batch_size", "32", "--smpl", str(tmp / "smpl.npz"), "--no_render"]

    def run(name, flags):
        import demo
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp / name), *flags]))
        return dict(np.load(tmp / name / "frames_" / "poco_results.npz"))
    run.tmp = tmp
    return run


@pytest.fixture(scope="module")
def built(case):
    return case("sort", ["--detections", str(case.tmp / "dets.json"), "--tracker", "sort", "--track_backfill"])


def test_two_tracks_from_a_detections_file(case, built):
    a, b = _boxes()
    assert {k.split("/")[0] for k in built} == {"0", "1"}
    assert np.array_equal(built["0/frame_ids"], np.arange(T)) and np.array_equal(built["1/frame_ids"], np.arange(LATE, T))   # backfilled
    assert np.array_equal(built["0/bboxes"], a.astype(np.float32)) and np.array_equal(built["1/bboxes"], b[LATE:].astype(np.float32))
    assert built["0/pose"].shape == (T, 24, 3, 3) and built["1/verts"].shape == (T - LATE, 6890, 3)
    assert np.abs(built["0/pose"][LATE:] - built["1/pose"]).max() > 1e-3           # two different people were regressed
    tr = json.loads((case.tmp / "sort" / "frames_" / "tracking_results_sort.json").read_text())
    assert list(tr) == ["0", "1"] and tr["1"]["frames"] == list(range(LATE, T)) and tr["1"]["bbox"] == b[LATE:].tolist()
    # without --track_backfill the late entrant is reported from her fourth frame on
    plain = case("sort_plain", ["--detections", str(case.tmp / "dets.json"), "--tracker", "sort"])
    assert np.array_equal(plain["1/frame_ids"], np.arange(LATE + 3, T)) and np.array_equal(plain["0/frame_ids"], np.arange(T))


def test_the_written_tracking_file_gives_the_same_results(case, built):
    again = case("reread", ["--tracking", str(case.tmp / "sort" / "frames_" / "tracking_results_sort.json")])
    assert set(again) == set(built)
    for k in built:
        assert again[k].dtype == built[k].dtype and again[k].shape == built[k].shape, k
    for pid in ("0", "1"):
        for k in ("pose", "betas", "var"):
            assert np.array_equal(np.ascontiguousarray(again[f"{pid}/{k}"]).view(np.uint32),
                                  np.ascontiguousarray(built[f"{pid}/{k}"]).view(np.uint32)), (pid, k)


def test_post_processing_takes_the_built_tracks(case, built):
    out = case("post", ["--detections", str(case.tmp / "dets.json"), "--tracker", "sort", "--track_backfill", "--infill", "0.3",
                        "--smooth_uncert", "10"])
    for pid, n in (("0", T), ("1", T - LATE)):
        assert out[f"{pid}/infill"].shape == (n, 24) and out[f"{pid}/smooth_shift"].shape == (n, 24)
        assert np.array_equal(out[f"{pid}/pose_net"], built[f"{pid}/pose"]) and np.isfinite(out[f"{pid}/pose"]).all()
        assert np.array_equal(out[f"{pid}/frame_ids"], built[f"{pid}/frame_ids"])


def test_conflicts_end_before_anything_is_written(case):
    with pytest.raises(SystemExit, match="--tracking"):
        case("refused", ["--detections", str(case.tmp / "dets.json"), "--tracker", "sort", "--tracking", str(case.tmp / "dets.json")])
    with pytest.raises(SystemExit, match="--detections"):
        case("refused", ["--tracker", "sort"])
    assert not (case.tmp / "refused").exists()
