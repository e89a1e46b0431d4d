"""CPU: SORT without a GPU - the restatement tests/sort_np.py against scipy's optimum and on a six-frame
example worked out by hand, the C ABI's declaration and argument checks of poco_op_sort_tracks (fake pointers, refused before any GPU
work), ops.sort_tracks' refusals, poco_amd/sort.py on both forms of a detections file (ops.sort_tracks replaced by the restatement),
demo.py's flags, and the decision margins of every seeded scene tests/test_sort_gpu.py uses."""
import ctypes as C
import json
import pickle

import numpy as np
import pytest

from poco_amd import _lib, sort
from tests import sort_np, sort_scenes


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_assignment_reaches_scipys_optimum_on_random_gated_matrices():
    from scipy.optimize import linear_sum_assignment
    r = np.random.default_rng(5)
    for trial in range(300):
        n, m = int(r.integers(1, 9)), int(r.integers(1, 9))
        g = r.uniform(0, 1, (n, m))
        g[g < 0.3] = 0.0
        if trial % 7 == 0:
            g[:] = 0.0
        rows, cols = linear_sum_assignment(g, maximize=True)
        want = g[rows, cols].sum()
        for total, pairs in (sort_np.assign(g), sort_np.assign(g, brute_below=0)) + ((sort_np.brute_assign(g),) if max(n, m) <= 6 else ()):
            assert abs(total - want) < 1e-12, (n, m, total, want)
            assert len({d for d, _ in pairs}) == len(pairs) == len({k for _, k in pairs}) and all(g[d, k] > 0 for d, k in pairs)
            assert abs(sum(g[d, k] for d, k in pairs) - total) < 1e-12


def test_matrices_are_those_of_the_published_sort():
    F, H, Q, R, P = sort_np.dense_matrices()
    assert np.array_equal(F, np.eye(7) + np.eye(7, k=4) * np.array([1, 1, 1, 0, 0, 0, 0])[:, None])
    assert np.array_equal(H, np.eye(7)[:4])
    assert np.array_equal(np.diag(R), [1, 1, 10, 10]) and np.array_equal(np.diag(Q), [1, 1, 1, 1, 0.01, 0.01, 0.0001])
    assert np.array_equal(np.diag(P), [10, 10, 10, 10, 1e4, 1e4, 1e4])
    # one update of a fresh tracker against the textbook dense form
    t = sort_np.Tracker((100.0, 50.0, 20.0, 40.0), 0, np.float64)
    t.predict()
    x0, P0 = t.x.copy(), t.P.copy()
    t.update((103.0, 52.0, 22.0, 41.0))
    z = np.array([103.0, 52.0, 22.0 * 41.0, 22.0 / 41.0])
    S = H @ P0 @ H.T + R
    K = P0 @ H.T @ np.linalg.inv(S)
    A = np.eye(7) - K @ H
    np.testing.assert_allclose(t.x, x0 + K @ (z - H @ x0), rtol=1e-12)
    np.testing.assert_allclose(t.P, A @ P0 @ A.T + K @ R @ K.T, rtol=1e-10, atol=1e-10)
    assert np.array_equal(t.P, t.P.T)


def test_six_frames_by_hand():
    """min_hits = 3, max_age = 1, iou_thresh = 0.3; A stands at (100, 100), B at (300, 100), both 40 x 80; detection order as listed.
      frame 1: A        -> A is born as 0; frame 1 <= min_hits: emitted                                  tracker [0]     id [0]
      frame 2: B, A     -> A matches 0 (streak 1, frame 2 <= 3: emitted); B is born as 1 (emitted)       tracker [1, 0]  id [1, 0]
      frame 3: A        -> 0 streak 2, frame 3 <= 3: emitted; 1 missed once (time_since_update 1 <= 1)   tracker [0]     id [0]
      frame 4: A, B     -> 0 streak 3: emitted; 1 matches B but its streak was reset: 1 < 3, not emitted  tracker [0, 1]  id [0, -1]
      frame 5: (none)   -> both missed once, both kept
      frame 6: B, A     -> 1 streak 1 after the reset, 0 streak 1: neither emitted                        tracker [1, 0]  id [-1, -1]
    Two trackers were created; every detection lands in a tracker."""
    A, B = (100.0, 100.0, 40.0, 80.0), (300.0, 100.0, 40.0, 80.0)
    sc = sort_scenes.pack([[[A], [B, A], [A], [A, B], [], [B, A]]])
    out = sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"])
    assert out["tracker"].tolist() == [0, 1, 0, 0, 0, 1, 1, 0]
    assert out["id"].tolist() == [0, 1, 0, 0, 0, -1, -1, -1]
    assert out["count"].tolist() == [2] and out["status"].tolist() == [0]
    np.testing.assert_allclose(out["box"], sc["dets"], rtol=1e-12)               # people who stand still: the filter returns their box
    # max_age = 0: B is dropped after frame 3 and reborn as 2 in frame 4; both are dropped after frame 5
    out = sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"], max_age=0)
    assert out["tracker"].tolist() == [0, 1, 0, 0, 0, 2, 3, 4] and out["count"].tolist() == [5]


def test_every_gpu_scene_has_decision_margins():
    """The condition under which the discrete outputs of two fp64 implementations must agree, checked here on the CPU: in every frame
    of every seeded scene the best total beats the best total without any one of its pairs by more than 1e-9 and no IoU lies within
    1e-9 of the threshold.  The scenes also do what they are named for."""
    got = {}
    for name, sc in sort_scenes.scenes().items():
        out = got[name] = sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"], **sc["params"])
        assert out["margin_assign"].min() > 1e-9 and out["margin_gate"].min() > 1e-9, name
    assert set(got) >= {"t1", "ragged", "empty_frames", "one_person", "crossing", "lost_age0", "lost_age1", "lost_age5", "late_hits0",
                        "late_hits3", "more_dets_then_fewer", "shrinking", "cap64", "overflow", "walkers"}
    sc = sort_scenes.scenes()
    assert len(sc["t1"]["frame_offsets"]) == 2 and np.diff(sc["ragged"]["clip_offsets"]).tolist() == [5, 0, 3]
    assert np.diff(sc["empty_frames"]["frame_offsets"]).tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0, 0]
    assert got["crossing"]["count"].tolist() == [2] and got["one_person"]["count"].tolist() == [1]
    for age in (0, 1, 5):                       # lost for max_age frames: kept; for max_age + 1: reborn under a new id
        t = got[f"lost_age{age}"]["tracker"]
        assert got[f"lost_age{age}"]["count"].tolist() == [3] and sorted(set(t.tolist())) == [0, 1, 2]
        assert (t == 1).sum() == 12 and (t == 2).sum() == 6
    assert (got["late_hits0"]["id"] >= 0).all() and (got["late_hits3"]["id"] == -1).sum() == 3
    assert got["more_dets_then_fewer"]["count"].tolist() == [7]
    assert got["shrinking"]["shrink_rule"] >= 1
    assert got["cap64"]["count"].tolist() == [64] and got["cap64"]["status"].tolist() == [0]
    o = got["overflow"]
    assert o["status"].tolist() == [1, 0] and o["count"].tolist() == [2, 1] and (o["tracker"][4:16] == -1).all() and (o["id"][4:16] == -1).all()
    assert np.isnan(o["box"][4:16]).all() and (o["tracker"][16:] == 0).all()
    assert got["walkers"]["count"].tolist() == [5] and len(sc["walkers"]["frame_offsets"]) == 301
    tie = sort_scenes.tie_scene()
    assert sort_np.sort_tracks(tie["dets"], tie["frame_offsets"], tie["clip_offsets"], **tie["params"])["margin_assign"].min() == 0.0


def test_recorded_rounding_floor_is_the_measured_one():
    """BOX_FLOOR of tests/sort_scenes.py (the tolerance of the GPU test is 16 x it) is what float64 against numpy.longdouble gives
    here, with the same discrete outputs; where long double is no wider than double the difference is 0 and only that is checked."""
    worst = 0.0
    for name, sc in sort_scenes.scenes().items():
        a = sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"], **sc["params"])
        b = sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"], **sc["params"], dtype=np.longdouble)
        assert all(np.array_equal(a[k], b[k]) for k in ("tracker", "id", "count", "status")), name
        ok = np.isfinite(a["box"]).all(1)
        assert np.array_equal(ok, np.isfinite(b["box"]).all(1))
        if ok.any():
            worst = max(worst, float(np.abs((a["box"][ok] - b["box"][ok]) / b["box"][ok]).max()))
    print(f"sort_np float64 against longdouble: largest relative difference of the filtered boxes {worst:.3e}")
    assert worst <= sort_scenes.BOX_FLOOR * 1.001
    if np.finfo(np.longdouble).eps < 1e-18:
        assert worst >= sort_scenes.BOX_FLOOR * 0.99


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_exports_and_checks_its_arguments():
    L = _lib.lib()
    assert "poco_op_sort_tracks" in _lib.header_symbols() and hasattr(L, "poco_op_sort_tracks")
    txt = _lib.HEADER.read_text()
    assert "#define POCO_SORT_MAX 64" in txt and "POCOTester.run_tracking" in txt
    fake, null = C.c_void_p(4096), C.c_void_p(0)

    def call(dets=fake, fo=fake, co=fake, Cn=2, F=10, N=30, thr=0.3, max_age=1, min_hits=3, max_trackers=64, tracker=fake, ident=fake,
             box=fake, count=fake, status=fake):
        return L.poco_op_sort_tracks(dets, fo, co, C.c_int64(Cn), C.c_int64(F), C.c_int64(N), C.c_double(thr), max_age, min_hits,
                                     max_trackers, tracker, ident, box, count, status, null)
    for kw in (dict(Cn=0), dict(Cn=-1), dict(F=-1), dict(N=-1), dict(Cn=(1 << 24) + 1), dict(F=(1 << 30) + 1), dict(N=(1 << 28) + 1),
               dict(N=1 << 40), dict(dets=null), dict(fo=null), dict(co=null), dict(tracker=null), dict(ident=null), dict(box=null),
               dict(count=null), dict(status=null), dict(fo=null, N=0), dict(thr=0.0), dict(thr=1.0), dict(thr=-0.5),
               dict(thr=float("nan")), dict(thr=float("inf")), dict(max_age=-1), dict(min_hits=-1), dict(max_trackers=0),
               dict(max_trackers=65), dict(max_trackers=-3)):
        assert call(**kw) == 1, kw
        assert "poco_op_sort_tracks" in L.poco_last_error().decode(), kw


def test_ops_sort_tracks_refuses_bad_arguments_without_a_gpu():
    import torch
    from poco_amd import ops
    boxes = torch.tensor([[10.0, 10.0, 4.0, 8.0]] * 6, dtype=torch.float64)
    ok = dict(dets=boxes, frame_offsets=[0, 2, 4, 6], clip_offsets=[0, 1, 3])
    crowd = torch.tensor([[10.0, 10.0, 4.0, 8.0]] * 70, dtype=torch.float64)
    bad_box = lambda i, j, v: boxes.clone().index_put((torch.tensor(i), torch.tensor(j)), torch.tensor(v, dtype=torch.float64))   # noqa: E731
    for kw, word in ((dict(dets=boxes.float()), "float64"), (dict(dets=boxes[:, :3]), "[N,4]"), (dict(dets=boxes.numpy()), "float64"),
                     (dict(frame_offsets=[0, 4, 2, 6]), "not monotone at frame 1"), (dict(frame_offsets=[1, 2, 4, 6]), "start at 0"),
                     (dict(frame_offsets=[0, 2, 4, 5]), "end at N"), (dict(frame_offsets=[0.0, 2.0, 4.0, 6.0]), "integer"),
                     (dict(frame_offsets=torch.tensor([0, 2, 4, 6], dtype=torch.int32), clip_offsets=[0, 2, 1, 3]), "not monotone at clip 1"),
                     (dict(clip_offsets=[0, 1, 2]), "end at F"), (dict(clip_offsets=[0]), "C >= 1"),
                     (dict(dets=crowd, frame_offsets=[0, 2, 67, 70]), "frame 1 holds 65"),
                     (dict(dets=bad_box(3, 2, 0.0)), "frame 1"), (dict(dets=bad_box(4, 3, -1.0)), "frame 2"),
                     (dict(dets=bad_box(0, 0, float("nan"))), "frame 0"), (dict(dets=bad_box(5, 1, float("inf"))), "frame 2"),
                     (dict(iou_thresh=0.0), "iou_thresh"), (dict(iou_thresh=1.0), "iou_thresh"), (dict(iou_thresh=float("nan")), "iou_thresh"),
                     (dict(max_age=-1), "max_age"), (dict(max_age=1.5), "max_age"), (dict(min_hits=-1), "min_hits"),
                     (dict(max_trackers=0), "max_trackers"), (dict(max_trackers=65), "max_trackers"), ({}, "CUDA")):
        with pytest.raises(_lib.PocoHipError) as e:
            ops.sort_tracks(**{**ok, **kw})
        assert "sort_tracks" in str(e.value) and word in str(e.value), (kw, e.value)


# ---- poco_amd/sort.py with the restatement in the operator's place ----------------------------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    import torch
    from poco_amd import ops

    def fake(dets, frame_offsets, clip_offsets=None, **kw):
        out = sort_np.sort_tracks(dets.numpy(), np.asarray(frame_offsets), clip_offsets, **kw)
        return {k: torch.from_numpy(out[k]) for k in ("tracker", "id", "box", "count", "status")}
    monkeypatch.setattr(ops, "sort_tracks", fake)


def _clip(T=12, late=5):
    """Person A in every frame, person B from frame `late` on and listed FIRST where both are there; frame 8 has no detection of A."""
    names = [f"{i:06d}.png" for i in range(T)]
    A = lambda i: [100.0 + 2 * i, 100.0, 40.0, 80.0]                           # noqa: E731
    B = lambda i: [300.0, 120.0 + i, 50.0, 90.0, 0.9]                          # noqa: E731 (a score column)
    return names, {n: ([B(i)] if i >= late else []) + ([A(i) + [0.8]] if i != 8 else []) for i, n in enumerate(names)}


def test_detections_to_buffers_reads_both_forms(tmp_path):
    names, by_name = _clip()
    a = sort.detections_to_buffers(by_name, names)
    assert a["dets"].dtype == np.float64 and a["dets"].shape == (18, 4) and a["frame_offsets"].dtype == np.int32
    assert a["frame_offsets"].tolist() == [0, 1, 2, 3, 4, 5, 7, 9, 11, 12, 14, 16, 18]
    assert a["dets"][5].tolist() == [300.0, 125.0, 50.0, 90.0]                   # the score is gone, B comes first in frame 5
    # the reference's cache: a list by position, float32 arrays, a frame without people as an empty list, a short list
    by_pos = [np.asarray(by_name[n], np.float32).reshape(-1, 5)[:, :4] if by_name[n] else [] for n in names[:-1]]
    with open(tmp_path / "detection_results.pkl", "wb") as f:
        pickle.dump(by_pos, f)
    (tmp_path / "d.json").write_text(json.dumps(by_name))
    from poco_amd.tester import load_detections
    b = sort.detections_to_buffers(load_detections(str(tmp_path / "detection_results.pkl")), names)
    assert b["frame_offsets"].tolist() == a["frame_offsets"].tolist()[:-1] + [16] and all(r.dtype == np.float32 for r in b["rows"])
    assert np.array_equal(b["dets"], a["dets"][:16])
    c = sort.detections_to_buffers(load_detections(str(tmp_path / "d.json")), names)
    assert np.array_equal(c["dets"], a["dets"]) and all(r.dtype == np.float64 for r in c["rows"] if len(r))
    assert sort.detections_to_buffers(None, names)["frame_offsets"].tolist() == [0] * 13
    with pytest.raises(ValueError, match="frame 1"):
        sort.detections_to_buffers({names[1]: [[1.0, 2.0, 3.0]]}, names)


def test_build_tracks_backfill_boxes_and_the_short_track_rule(restated):
    names, by_name = _clip()
    kw = dict(device="cpu", min_frames=1)
    tr = sort.build_tracks(by_name, names, **kw)
    assert list(tr) == ["0", "1"] and tr["0"]["frames"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 11]   # the miss at 8 restarts the streak: 3 at 11
    assert tr["1"]["frames"].tolist() == [8, 9, 10, 11] and tr["1"]["frames"].dtype == np.int64      # B: born at 5, emitted from its 4th frame
    assert tr["1"]["bbox"].dtype == np.float64 and tr["1"]["bbox"].tolist() == [by_name[names[i]][0][:4] for i in (8, 9, 10, 11)]
    assert tr["0"]["bbox"][5].tolist() == [110.0, 100.0, 40.0, 80.0]             # A's own row, the second of frame 5
    back = sort.build_tracks(by_name, names, backfill=True, **kw)
    assert back["1"]["frames"].tolist() == [5, 6, 7, 8, 9, 10, 11] and back["0"]["frames"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]
    f32 = {n: np.asarray(v, np.float32) for n, v in by_name.items() if v}
    assert sort.build_tracks(f32, names, **kw)["0"]["bbox"].dtype == np.float32                    # the user's dtype is kept
    filt = sort.build_tracks(by_name, names, boxes="filtered", **kw)
    assert filt["0"]["bbox"].dtype == np.float64 and filt["0"]["frames"].tolist() == tr["0"]["frames"].tolist()
    assert not np.array_equal(filt["0"]["bbox"], tr["0"]["bbox"]) and np.abs(filt["0"]["bbox"] - tr["0"]["bbox"]).max() < 3.0
    assert list(sort.build_tracks(by_name, names, device="cpu", min_frames=5)) == ["0"]            # B's four frames: dropped
    assert list(sort.build_tracks(by_name, names, device="cpu", min_frames=5, backfill=True)) == ["0", "1"]
    assert sort.build_tracks(by_name, names, device="cpu") == {} and sort.MIN_NUM_FRAMES == 25
    with pytest.raises(ValueError, match=r"frame 5 \(000005.png\)"):
        sort.build_tracks(by_name, names, max_trackers=1, **kw)
    with pytest.raises(ValueError, match="boxes"):
        sort.build_tracks(by_name, names, boxes="smooth", **kw)


def test_written_tracking_file_reads_back(restated, tmp_path):
    from poco_amd.tester import load_tracking
    names, by_name = _clip()
    tr = sort.build_tracks(by_name, names, device="cpu", min_frames=1, backfill=True)
    sort.write_tracking(str(tmp_path / "tracking_results_sort.json"), tr)
    back = load_tracking(str(tmp_path / "tracking_results_sort.json"))
    assert list(back) == list(tr)
    for pid in tr:
        assert np.array_equal(back[pid]["frames"], tr[pid]["frames"]) and np.array_equal(back[pid]["bbox"], tr[pid]["bbox"].astype(np.float32))


# ---- demo.py's flags ----------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt", "--mode", "video", "--vid_file", "none"]


def test_demo_flags_parse_and_conflicts_end_before_the_engine():
    import demo
    a = demo.parse_args(BASE)
    assert a.tracker == "none" and a.track_iou == 0.3 and a.track_max_age == 1 and a.track_min_hits == 3
    assert a.track_boxes == "detection" and a.track_backfill is False and sort.flag_error(a) is None
    a = demo.parse_args(BASE + ["--detections", "d.json", "--tracker", "sort", "--track_iou", "0.5", "--track_max_age", "4",
                                "--track_min_hits", "0", "--track_boxes", "filtered", "--track_backfill"])
    assert (a.tracker, a.track_iou, a.track_max_age, a.track_min_hits, a.track_boxes, a.track_backfill) == ("sort", 0.5, 4, 0, "filtered", True)
    assert sort.flag_error(a) is None
    with pytest.raises(SystemExit):
        demo.parse_args(BASE + ["--tracker", "deepsort"])
    sortf = ["--tracker", "sort"]
    for flags, word in ((sortf + ["--detections", "d.json", "--tracking", "t.json"], "--tracking"), (sortf, "--detections"),
                        (sortf + ["--tracking", "t.json"], "--tracking"), (["--track_backfill"], "needs --tracker sort"),
                        (["--track_iou", "0.5"], "needs --tracker sort"), (["--track_boxes", "filtered"], "needs --tracker sort"),
                        (sortf + ["--detections", "d.json", "--kp_refit", "1.0"], "--kp_refit"),
                        (sortf + ["--detections", "d.json", "--track_iou", "1.0"], "--track_iou"),
                        (sortf + ["--detections", "d.json", "--track_max_age", "-1"], "--track_max_age"),
                        (sortf + ["--detections", "d.json", "--mode", "folder", "--image_folder", "x"], "--mode video")):
        with pytest.raises(SystemExit) as e:                                   # no engine, no input folder needed
            demo.main(demo.parse_args(BASE + flags))
        assert word in str(e.value), (flags, e.value)
