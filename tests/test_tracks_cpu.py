"""CPU: keypoint tracks -> boxes (poco_amd/tracks.py) against the reference's own functions, whose outputs on seeded tracks are
stored in tests/golden/tracks.npz (tools/gen_tracks_golden.py: pocolib/utils/smooth_bbox.py get_all_bbox_params(., 0.3) and
smooth_bbox_params); load_tracking on keypoint files; the demo's three flags.

The reference's parameters take the keypoints' float type: float64 keypoints (what a tracker's pickle holds, and what a json file
is read as) give float64 parameters - stacking a float64 row onto its float32 [0,3] start array promotes it - and float32
keypoints give float32 ones.  poco_amd/tracks.py calls the same numpy functions on operands of the same types, so every case below
was bit-equal when the fixture was written, both float types and the smoothed parameters included; the tests assert the
1e-6 relative bound and, for the unsmoothed parameters, bit-equality."""
import json
from pathlib import Path

import numpy as np
import pytest

from poco_amd import tracks

GOLDEN = Path(__file__).resolve().parent / "golden" / "tracks.npz"
CASES = ("c1", "c2", "c3", "c4", "c5", "c6", "c7")
RTOL = 1e-6


def _decode(q, dtype=np.float64):
    """The fixture's int16 keypoints: x, y in half pixels, confidence in 1/16 (exact in float32 and float64)."""
    return np.concatenate([q[..., :2].astype(dtype) / dtype(2), q[..., 2:].astype(dtype) / dtype(16)], -1)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    q = {f"c{i + 1}": (g["kp40"][i], g["none40"][i]) for i in range(5)}
    q["c6"] = (g["kp5"], np.zeros(5, bool))
    q["c7"] = (g["kp44"], g["none44"])
    g["tracks"] = q
    return g


def _track(golden, case, dtype=np.float64):
    q, none = golden["tracks"][case]
    return [None if n else k for k, n in zip(_decode(q, dtype), none)]


def test_fixture_is_what_the_cases_say(golden):
    """The fixture cannot pass vacuously: the trim, the gaps, the None entries and the degenerate frame are in it."""
    assert GOLDEN.stat().st_size < 32 << 10
    rng = {c: tuple(int(v) for v in golden[f"{c}_range"]) for c in CASES}
    assert rng == {"c1": (0, 40), "c2": (3, 37), "c3": (0, 40), "c4": (2, 39), "c5": (0, 40), "c6": (0, 5), "c7": (0, 12)}
    c1, c3, c5 = golden["c1_params64"], golden["c3_params64"], golden["c5_params64"]
    gap = [10] + list(range(20, 27))
    assert (c3[gap] != c1[gap]).any(1).all() and np.array_equal(np.delete(c3, gap, 0), np.delete(c1, gap, 0))
    assert (c5[12] != c1[12]).any() and np.array_equal(np.delete(c5, 12, 0), np.delete(c1, 12, 0))
    assert golden["tracks"]["c7"][0].shape == (12, 44, 3) and sum(k is None for k in _track(golden, "c4")) == 6


@pytest.mark.parametrize("case", CASES)
def test_params_match_reference(golden, case):
    kps = _track(golden, case)
    params, start, end = tracks.bbox_params_from_keypoints(kps, float(golden["vis_thresh"]))
    ref = golden[f"{case}_params64"]
    assert (start, end) == tuple(golden[f"{case}_range"]) and params.dtype == ref.dtype == np.float64 and params.shape == ref.shape
    np.testing.assert_allclose(params, ref, rtol=RTOL, atol=0)
    assert np.array_equal(params, ref)
    smoothed = tracks.smooth_bbox_params(params)
    assert smoothed.dtype == np.float64
    np.testing.assert_allclose(smoothed, golden[f"{case}_smooth64"], rtol=RTOL, atol=0)
    assert np.abs(smoothed - params).max() > 1e-3                           # the filters did something


@pytest.mark.parametrize("case", ["c3", "c7"])
def test_float32_keypoints_give_the_reference_float32_params(golden, case):
    params, start, end = tracks.bbox_params_from_keypoints(_track(golden, case, np.float32), 0.3)
    ref = golden[f"{case}_params32"]
    assert params.dtype == ref.dtype == np.float32 and (start, end) == tuple(golden[f"{case}_range"])
    np.testing.assert_allclose(params, ref, rtol=RTOL, atol=0)
    assert np.array_equal(params, ref)


def test_input_forms_agree(golden):
    """[T,K,3] array == list of [K,3] arrays == nested lists (a json file)."""
    arr = _decode(golden["kp40"][2])
    want = golden["c3_params64"]
    for form in (arr, list(arr), arr.tolist()):
        params, start, end = tracks.bbox_params_from_keypoints(form, 0.3)
        assert np.array_equal(params, want) and (start, end) == (0, 40)


def test_interpolation_is_linear(golden):
    """Independent of the fixture: a one-frame gap is the mean of its neighbours, a seven-frame gap divides the step by 8."""
    p = golden["c3_params64"]
    got, _, _ = tracks.bbox_params_from_keypoints(_track(golden, "c3"), 0.3)
    np.testing.assert_allclose(got[10], (p[9] + p[11]) / 2, rtol=1e-12)
    for i in range(1, 8):
        np.testing.assert_allclose(got[19 + i], p[19] + (p[27] - p[19]) * i / 8, rtol=1e-12)


@pytest.mark.parametrize("case", ["c2", "c4", "c7"])
def test_boxes_from_keypoints(golden, case):
    kps = _track(golden, case)
    frames = np.arange(100, 100 + len(kps))
    start, end = (int(v) for v in golden[f"{case}_range"])
    tr = tracks.boxes_from_keypoints(kps, frames)
    p = golden[f"{case}_params64"]
    side = 150.0 / p[:, 2]
    assert tr["bbox"].dtype == np.float32 and tr["bbox"].shape == (end - start, 4)
    assert np.array_equal(tr["bbox"], np.stack([p[:, 0], p[:, 1], side, side], 1).astype(np.float32))
    assert np.array_equal(tr["frames"], frames[start:end]) and tr["frames"].dtype == np.int64
    assert tr["joints2d"].shape == (end - start,) + kps[start].shape and tr["joints2d"].dtype == np.float64
    for row, kp in zip(tr["joints2d"], kps[start:end]):
        assert np.array_equal(row, np.zeros_like(row) if kp is None else kp)        # a None inside the range: confidence 0
    # the box is the square around the visible joints whose side is their diagonal
    k = next(i for i in range(start, end) if kps[i] is not None)
    vis = kps[k][kps[k][:, 2] > 0.3, :2]
    np.testing.assert_allclose(tr["bbox"][k - start, 2], np.linalg.norm(vis.max(0) - vis.min(0)), rtol=1e-6)
    np.testing.assert_allclose(tr["bbox"][k - start, :2], (vis.max(0) + vis.min(0)) / 2, rtol=1e-6)
    # smoothing: the reference's smoothed parameters, same rule
    sm = tracks.boxes_from_keypoints(kps, frames, smooth=True)
    s = golden[f"{case}_smooth64"]
    np.testing.assert_allclose(sm["bbox"], np.stack([s[:, 0], s[:, 1], 150.0 / s[:, 2], 150.0 / s[:, 2]], 1), rtol=1e-6)
    assert np.array_equal(sm["frames"], tr["frames"]) and np.array_equal(sm["joints2d"], tr["joints2d"])
    with pytest.raises(ValueError, match="frames"):
        tracks.boxes_from_keypoints(kps, frames[:-1])


def test_track_without_a_usable_frame_is_empty(golden):
    """The reference fails there (it returns start = -1 and an empty array that Inference then indexes)."""
    low = _decode(golden["kp40"][0])
    low[..., 2] = 0.1
    point = _decode(golden["kp40"][0])
    point[..., :2] = point[:, :1, :2]                                  # every frame: all joints on one spot, diagonal 0
    for kps in (low, [None] * 4, [], point):
        params, start, end = tracks.bbox_params_from_keypoints(kps, 0.3)
        assert params.shape == (0, 3) and (start, end) == (0, 0)
        tr = tracks.boxes_from_keypoints(kps, np.arange(len(kps)))
        assert tr["bbox"].shape == (0, 4) and tr["bbox"].dtype == np.float32 and len(tr["frames"]) == 0 and len(tr["joints2d"]) == 0


def _pose_file(golden):
    """Two keypoint tracks as a tracker writes them: c2 (trimmed to 34 frames) and c3 (40 frames)."""
    return {1: {"joints2d": _decode(golden["kp40"][1]), "frames": np.arange(5, 45)},
            2: {"joints2d": _decode(golden["kp40"][2]), "frames": np.arange(40)}}


def test_load_tracking_reads_keypoint_tracks(golden, tmp_path):
    """json and pickle files of {'joints2d', 'frames'} tracks (the parent commit: KeyError 'bbox')."""
    import joblib
    from poco_amd.tester import load_tracking
    raw = _pose_file(golden)
    joblib.dump(raw, tmp_path / "tracking_results_pose.pkl")
    (tmp_path / "pose.json").write_text(json.dumps({str(k): {"joints2d": v["joints2d"].tolist(), "frames": v["frames"].tolist()}
                                                    for k, v in raw.items()}))
    for name in ("tracking_results_pose.pkl", "pose.json"):
        for method in ("bbox", "pose"):                                  # the content decides; pose only insists on keypoints
            got = load_tracking(str(tmp_path / name), method=method)
            assert list(got) == ["1", "2"]
            for pid, case in (("1", "c2"), ("2", "c3")):
                want = tracks.boxes_from_keypoints(raw[int(pid)]["joints2d"], raw[int(pid)]["frames"])
                assert set(got[pid]) == {"bbox", "frames", "joints2d"}
                for k in want:
                    assert np.array_equal(got[pid][k], want[k]) and got[pid][k].dtype == want[k].dtype, (name, pid, k)
                p = golden[f"{case}_params64"]
                assert np.array_equal(got[pid]["bbox"][:, :2], p[:, :2].astype(np.float32))
            assert got["1"]["frames"].tolist() == list(range(8, 42)) and got["2"]["frames"].tolist() == list(range(40))
    # the keyword arguments: another threshold, smoothing
    sm = load_tracking(str(tmp_path / "pose.json"), smooth_bbox=True)["2"]
    s = golden["c3_smooth64"]
    np.testing.assert_allclose(sm["bbox"][:, 2], 150.0 / s[:, 2], rtol=1e-6)
    hi = load_tracking(str(tmp_path / "pose.json"), vis_thresh=0.99)
    want = tracks.boxes_from_keypoints(raw[2]["joints2d"], raw[2]["frames"], 0.99)
    assert np.array_equal(hi["2"]["bbox"], want["bbox"]) and not np.array_equal(hi["2"]["bbox"], sm["bbox"])


def test_load_tracking_short_and_empty_keypoint_tracks(golden, tmp_path, capsys):
    """The 25-frame rule of .pkl files counts the frames left after the trim; a track without a usable frame is dropped and
    named on stderr; json keeps short tracks (explicit input), as for boxes."""
    import joblib
    from poco_amd.tester import load_tracking
    kp = _decode(golden["kp40"][0])[:30].copy()
    kp[:3, :, 2] = 0.1
    kp[27:, :, 2] = 0.1                                                    # 30 frames, 24 after the trim
    full = _decode(golden["kp40"][0])[:30]
    dead = np.zeros((30, 25, 3))
    raw = {"short": {"joints2d": kp, "frames": np.arange(30)}, "full": {"joints2d": full, "frames": np.arange(30)},
           "dead": {"joints2d": dead, "frames": np.arange(30)}}
    joblib.dump(raw, tmp_path / "t.pkl")
    got = load_tracking(str(tmp_path / "t.pkl"))
    assert list(got) == ["full"] and len(got["full"]["frames"]) == 30
    err = capsys.readouterr().err.strip().splitlines()
    assert len(err) == 1 and "'dead'" in err[0]
    (tmp_path / "t.json").write_text(json.dumps({k: {"joints2d": v["joints2d"].tolist(), "frames": v["frames"].tolist()}
                                                 for k, v in raw.items()}))
    got = load_tracking(str(tmp_path / "t.json"))
    assert list(got) == ["short", "full"] and got["short"]["frames"].tolist() == list(range(3, 27))
    # json null entries
    lst = full[:6].tolist()
    lst[0] = lst[3] = None
    (tmp_path / "n.json").write_text(json.dumps({"p": {"joints2d": lst, "frames": [10, 11, 12, 13, 14, 15]}}))
    got = load_tracking(str(tmp_path / "n.json"))["p"]
    assert got["frames"].tolist() == [11, 12, 13, 14, 15] and not got["joints2d"][2].any() and got["bbox"].shape == (5, 4)
    np.testing.assert_allclose(got["bbox"][2], (got["bbox"][1].astype(np.float64) + got["bbox"][3]) / 2, rtol=1e-2)
    np.testing.assert_allclose(got["bbox"][2, :2], (got["bbox"][1, :2].astype(np.float64) + got["bbox"][3, :2]) / 2, rtol=1e-6)


def test_load_tracking_box_tracks_are_read_as_before(golden, tmp_path):
    import joblib
    from poco_amd.tester import load_tracking
    r = np.random.default_rng(0)
    boxes = {1: r.uniform(10, 300, (30, 4)), 2: r.uniform(10, 300, (5, 4)), 3: r.uniform(10, 300, (26, 4)).astype(np.float32)}
    raw = {k: {"bbox": b, "frames": np.arange(k, k + len(b))} for k, b in boxes.items()}
    kp = _decode(golden["kp40"][0])[:26]
    raw[3]["joints2d"] = kp                                                # keypoints next to boxes: kept, the boxes win
    joblib.dump(raw, tmp_path / "tracking_results_bbox.pkl")
    got = load_tracking(str(tmp_path / "tracking_results_bbox.pkl"))
    assert list(got) == ["1", "3"]                                         # 5 frames < 25: dropped
    for k in (1, 3):
        t = got[str(k)]
        assert t["bbox"].dtype == np.float32 and np.array_equal(t["bbox"], boxes[k].astype(np.float32))
        assert t["frames"].dtype == np.int64 and np.array_equal(t["frames"], raw[k]["frames"])
    assert set(got["1"]) == {"bbox", "frames"} and np.array_equal(got["3"]["joints2d"], kp)
    (tmp_path / "t.json").write_text(json.dumps({"7": {"bbox": boxes[2].tolist(), "frames": [4, 5, 6, 7, 8]}}))
    t = load_tracking(str(tmp_path / "t.json"))["7"]
    assert set(t) == {"bbox", "frames"} and np.array_equal(t["bbox"], boxes[2].astype(np.float32)) and t["frames"].tolist() == [4, 5, 6, 7, 8]
    # --tracking_method pose on a box file: an error that names the track
    with pytest.raises(ValueError, match="'7'.*joints2d"):
        load_tracking(str(tmp_path / "t.json"), method="pose")
    assert load_tracking(None) is None


def test_demo_flags():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "c.pt"]
    a = demo.parse_args(base)
    assert a.tracking_method == "bbox" and a.kp_vis_thresh == 0.3 and a.smooth_bbox is False
    a = demo.parse_args(base + ["--tracking_method", "pose", "--kp_vis_thresh", "0.1", "--smooth_bbox"])
    assert a.tracking_method == "pose" and a.kp_vis_thresh == 0.1 and a.smooth_bbox is True
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--tracking_method", "staf"])
    from poco_amd.tester import tracking_options
    assert tracking_options(a) == {"method": "pose", "vis_thresh": 0.1, "smooth_bbox": True}
    assert tracking_options(demo.parse_args(base)) == {"method": "bbox", "vis_thresh": 0.3, "smooth_bbox": False}


def test_input_keypoints_of_the_renderer():
    """--draw_keypoints: the input keypoints above the threshold, black (poco_amd/render.py input_keypoints)."""
    from poco_amd.render import input_keypoints
    kp = np.array([[10.5, 20.25, 0.9], [30, 40, 0.3], [50, 60, 0.31], [70, 80, 0.0]])
    pts, rgb = input_keypoints(kp, 0.3)
    assert pts.dtype == np.float32 and np.array_equal(pts, np.array([[10.5, 20.25], [50, 60]], np.float32))
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 3) and not rgb.any()
    assert input_keypoints(kp, 0.95)[0].shape == (0, 2)
