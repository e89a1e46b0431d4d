"""GPU: demo.py --mode video on 2-D pose tracks ({'joints2d', 'frames'}: the reference's --tracking_method pose).  The boxes are
derived on the host (poco_amd/tracks.py, checked against the reference in tests/test_tracks_cpu.py); what is checked here is the
hand-over: a keypoint file and a box file that holds exactly the derived boxes give bit-equal results (the box path adds no
arithmetic on the device), the result carries the trimmed keypoints, --draw_keypoints stamps them, and two ranks merge them.

Synthetic checkpoint and body model of tests/test_demo_gpu.py (resnet50-cliff, whose own 2-D joints video mode sends off the
frame: tests/test_render_overlay_gpu.py::test_demo_video_keypoints - so every disc on these pictures is an input keypoint's), 12
frames of 96 x 128, two people standing apart."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import synth, tracks
from tests import render_overlay_np as ov, util

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
T, H, W, K = 12, 96, 128, 25
LOW = (6, 13, 17)                 # joints below the threshold in every frame: inside the lattice, so the box does not move
THRESH = 0.3


def _people():
    """{person: [T,K,3] float64}: a 5 x 5 lattice of joints per person, 10 px apart in x and 12 in y (the r = 4 stamps of two
    joints never touch), at sub-pixel positions, drifting half a pixel per frame; person 0 on the left, person 1 on the right."""
    r = np.random.default_rng(7)
    out = {}
    for pid, (x0, y0) in (("0", (8.25, 20.5)), ("1", (78.5, 24.25))):
        gx, gy = np.meshgrid(np.arange(5) * 10.0, np.arange(5) * 12.0)
        xy = np.stack([gx.ravel() + x0, gy.ravel() + y0], 1)[None] + r.uniform(-0.4, 0.4, (T, K, 2))
        xy[..., 0] += 0.5 * np.arange(T)[:, None] * (1 if pid == "0" else -1)
        conf = r.uniform(0.6, 1.0, (T, K))
        conf[:, LOW] = 0.1
        out[pid] = np.concatenate([xy, conf[..., None]], -1)
    return out


def _write_pose(path, people):
    """people: {pid: list of [K,3] arrays or None} over frames 0 .. T-1."""
    path.write_text(json.dumps({pid: {"joints2d": [None if k is None else np.asarray(k).tolist() for k in kps],
                                      "frames": list(range(len(kps)))} for pid, kps in people.items()}))


def _write_boxes(path, derived):
    path.write_text(json.dumps({pid: {"bbox": tr["bbox"].tolist(), "frames": tr["frames"].tolist()} for pid, tr in derived.items()}))


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("pose_tracks")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
    smpl = synth.synth_smpl(7)
    smpl["faces"] = np.stack([np.arange(0, 3000), np.arange(1, 3001), np.arange(2, 3002)], 1).astype(np.int32)
    np.savez(tmp / "smpl.npz", **smpl)
    fr = tmp / "frames"
    fr.mkdir()
    r = np.random.default_rng(2)
    frames = [r.integers(1, 256, (H, W, 3), dtype=np.uint8) for _ in range(T)]              # no black pixel of their own
    for i, f in enumerate(frames):
        Image.fromarray(f).save(fr / f"{i:06d}.png")
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video",
              "--vid_file", str(fr), "--batch_size", "5", "--smpl", str(tmp / "smpl.npz")]
    return tmp, common, frames


def _demo(tmp, common, name, tracking, flags=()):
    import demo
    demo.main(demo.parse_args(common + ["--tracking", str(tracking), "--output_folder", str(tmp / name), *flags]))
    return tmp / name / "frames_"


def _same_except_joints2d(pose_npz, box_npz):
    a, b = dict(np.load(pose_npz)), dict(np.load(box_npz))
    assert {k for k in a if not k.endswith("/joints2d")} == set(b) and not any(k.endswith("/joints2d") for k in b)
    for k in b:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    return a


@pytest.fixture(scope="module")
def clean(case):
    """The clean keypoint file and the box file of its derived boxes, both run once."""
    tmp, common, _ = case
    people = {pid: list(kp) for pid, kp in _people().items()}
    derived = {pid: tracks.boxes_from_keypoints(kps, np.arange(T), THRESH) for pid, kps in people.items()}
    _write_pose(tmp / "pose.json", people)
    _write_boxes(tmp / "boxes.json", derived)
    return people, derived, _demo(tmp, common, "clean_pose", tmp / "pose.json", ["--no_render"]), \
        _demo(tmp, common, "clean_box", tmp / "boxes.json", ["--no_render"])


@pytest.fixture(scope="module")
def gappy(case):
    """Person 0: frames 0 and 1 below the threshold, frame 6 missing.  Both files rendered with --draw_keypoints."""
    tmp, common, _ = case
    people = {pid: list(kp.copy()) for pid, kp in _people().items()}
    people["0"][0][:, 2] = people["0"][1][:, 2] = 0.1
    people["0"][6] = None
    derived = {pid: tracks.boxes_from_keypoints(kps, np.arange(T), THRESH) for pid, kps in people.items()}
    _write_pose(tmp / "gappy_pose.json", people)
    _write_boxes(tmp / "gappy_boxes.json", derived)
    flags = ["--render", "--draw_keypoints"]
    return people, derived, _demo(tmp, common, "gappy_pose", tmp / "gappy_pose.json", flags), \
        _demo(tmp, common, "gappy_box", tmp / "gappy_boxes.json", flags)


def test_same_boxes_same_results(case, clean):
    tmp, common, _ = case
    people, derived, out_pose, out_box = clean
    a = _same_except_joints2d(out_pose / "poco_results.npz", out_box / "poco_results.npz")
    for pid, kps in people.items():
        assert np.array_equal(a[f"{pid}/frame_ids"], np.arange(T)) and a[f"{pid}/verts"].shape == (T, 6890, 3)
        assert np.array_equal(a[f"{pid}/bboxes"], derived[pid]["bbox"])
        assert a[f"{pid}/joints2d"].shape == (T, K, 3) and np.array_equal(a[f"{pid}/joints2d"], np.stack(kps))
        # the box is the square on the confident joints' diagonal, around their centre - worked out here, not by the code under test
        vis = np.stack(kps)[:, [j for j in range(K) if j not in LOW], :2]
        lo, hi = vis.min(1), vis.max(1)
        np.testing.assert_allclose(a[f"{pid}/bboxes"][:, :2], (lo + hi) / 2, rtol=1e-6)
        np.testing.assert_allclose(a[f"{pid}/bboxes"][:, 2], np.linalg.norm(hi - lo, axis=1), rtol=1e-6)
    assert np.abs(a["0/pose"] - a["1/pose"]).max() > 1e-3                        # two different people were regressed
    # --skip_frame slices the keypoints with the boxes and the frames; --tracking_method pose accepts the file
    out = _demo(tmp, common, "clean_skip", tmp / "pose.json", ["--no_render", "--skip_frame", "2", "--tracking_method", "pose"])
    s = dict(np.load(out / "poco_results.npz"))
    for pid, kps in people.items():
        assert np.array_equal(s[f"{pid}/frame_ids"], np.arange(0, T, 2)) and np.array_equal(s[f"{pid}/joints2d"], np.stack(kps)[::2])
        assert np.array_equal(s[f"{pid}/bboxes"], derived[pid]["bbox"][::2])
    # ... and refuses a box file, naming the track, before any result is written
    with pytest.raises(SystemExit, match="'0'.*joints2d"):
        _demo(tmp, common, "refused", tmp / "boxes.json", ["--no_render", "--tracking_method", "pose"])
    assert not (tmp / "refused").exists()


def test_trim_and_gap(gappy):
    people, derived, out_pose, out_box = gappy
    a = _same_except_joints2d(out_pose / "poco_results.npz", out_box / "poco_results.npz")
    assert np.array_equal(a["0/frame_ids"], np.arange(2, T)) and np.array_equal(a["1/frame_ids"], np.arange(T))
    assert a["0/verts"].shape == (T - 2, 6890, 3) and a["0/joints2d"].shape == (T - 2, K, 3)
    row = int(np.nonzero(a["0/frame_ids"] == 6)[0][0])                        # the interpolated frame is present ...
    assert not a["0/joints2d"][row].any()                                     # ... without keypoints of its own
    for k, f in enumerate(range(2, T)):
        if f != 6:
            assert np.array_equal(a["0/joints2d"][k], people["0"][f])
    # its box: centre = the mean of the neighbours' centres, side = 150 / the mean of the neighbours' 150 / side
    b = a["0/bboxes"].astype(np.float64)
    np.testing.assert_allclose(b[row, :2], (b[row - 1, :2] + b[row + 1, :2]) / 2, rtol=1e-6)
    np.testing.assert_allclose(b[row, 2:], 2.0 / (1.0 / b[row - 1, 2:] + 1.0 / b[row + 1, 2:]), rtol=1e-6)
    # (_same_except_joints2d: that row equals the row of the run on the box file, which holds this interpolated box)
    assert np.array_equal(a["0/bboxes"], derived["0"]["bbox"]) and np.abs(a["0/pose"][row] - a["0/pose"][row - 1]).max() > 0


def test_input_keypoints_are_drawn(case, gappy):
    """--render --draw_keypoints: the picture of the keypoint file is the picture of the box file (same run, no keypoints to draw)
    with the r = 4 stamps of tests/render_overlay_np.py at every input keypoint above the threshold, black."""
    from PIL import Image
    _, _, frames = case
    people, derived, out_pose, out_box = gappy
    drawn = 0
    for f in range(T):
        png = np.asarray(Image.open(out_pose / "tmp_images_output" / f"{f:06d}.png"))
        base = np.asarray(Image.open(out_box / "tmp_images_output" / f"{f:06d}.png"))
        assert png.shape == base.shape == (H, W, 3)
        above, below = [], []
        for pid, kps in people.items():
            if f in derived[pid]["frames"] and kps[f] is not None:
                above.append(kps[f][kps[f][:, 2] > THRESH, :2])
                below.append(kps[f][kps[f][:, 2] <= THRESH, :2])
        assert (base != frames[f]).any(), "no mesh was drawn"
        if not above:
            assert np.array_equal(png, base)
            continue
        above, below = np.concatenate(above).astype(np.float32), np.concatenate(below).astype(np.float32)
        for pts in (np.trunc(above), np.rint(above)):                             # the stamp's centre pixel, and the rounded position
            assert not png[pts[:, 1].astype(int), pts[:, 0].astype(int)].any()
        at = np.trunc(below).astype(int)
        assert len(at) >= len(LOW) and np.array_equal(png[at[:, 1], at[:, 0]], base[at[:, 1], at[:, 0]])
        assert np.array_equal(png, ov.draw_discs_np(base, above, [[0, 0, 0]], 4))
        drawn += len(above)
    # frames 0, 1 (person 0 trimmed) and 6 (no keypoints) draw person 1's only
    assert drawn == (K - len(LOW)) * (T + T - 3)


def _run(cmd, timeout=600):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None); e.pop("RANK", None); e.pop("LOCAL_RANK", None)
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)


def test_two_ranks_merge_keypoint_tracks(case, clean):
    """demo.py --gpus 2 --dist_backend gloo (the pattern of tests/test_multirank_gpu.py: two ranks share the device): each rank
    derives the boxes itself, one track each; rank 0 writes both tracks' keypoints, boxes and frames exactly, and the regressed
    arrays within that test's tolerances (rank 0 re-derives the other rank's meshes from the gathered pose)."""
    tmp, common, _ = case
    _, _, out_pose, _ = clean
    two = _run(["demo.py"] + common + ["--tracking", str(tmp / "pose.json"), "--no_render", "--output_folder", str(tmp / "two"),
                                       "--gpus", "2", "--dist_backend", "gloo"])
    assert two.returncode == 0, two.stderr[-3000:]
    stats = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1])
    assert stats["ranks"] == 2 and stats["tracks"] == 2 and stats["crops"] == 2 * T
    a, b = dict(np.load(out_pose / "poco_results.npz")), dict(np.load(tmp / "two" / "frames_" / "poco_results.npz"))
    assert set(a) == set(b) and "1/joints2d" in b
    for k in a:
        assert a[k].shape == b[k].shape, k
        if k.split("/")[1] in ("joints2d", "bboxes", "frame_ids"):
            assert np.array_equal(a[k], b[k]), k
        else:
            tol = 2e-2 if k.endswith("smpl_joints2d") else 1e-4            # 2-D joints in full-image pixels (values ~1e3)
            assert np.abs(a[k].astype(np.float64) - b[k]).max() <= tol, (k, np.abs(a[k].astype(np.float64) - b[k]).max())
