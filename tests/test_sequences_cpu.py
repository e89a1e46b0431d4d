"""CPU: eval.py --sequences without a GPU - sequences.group_tracks on hand-written name lists, --seq_post
parsing and every refusal, the C ABI's declaration and argument checks of poco_op_track_accel (fake pointers, refused before any
GPU work), and the plain-loop restatement tests/accel_np.py on a motion whose acceleration is known."""
import ctypes as C

import numpy as np
import pytest

from poco_amd import _lib, sequences
from tests import accel_np


# ---- group_tracks ----------------------------------------------------------------------------------------------------------
def test_two_people_per_frame_without_person_id_are_told_apart_by_their_rank():
    names = ["imageFiles/courtyard_00/image_00000.jpg", "imageFiles/courtyard_00/image_00000.jpg",
             "imageFiles/courtyard_00/image_00001.jpg", "imageFiles/courtyard_00/image_00001.jpg",
             "imageFiles/courtyard_00/image_00002.jpg"]
    g = sequences.group_tracks(names)
    assert g["order"].tolist() == [0, 2, 4, 1, 3] and g["offsets"].tolist() == [0, 3, 5] and g["frames"].tolist() == [0, 1, 2, 0, 1]
    assert g["names"] == ["imageFiles/courtyard_00#0", "imageFiles/courtyard_00#1"]
    assert all(g[k].dtype == np.int32 for k in ("order", "offsets", "frames"))


def test_person_id_decides_where_the_file_has_it():
    names = ["s/a_10.png", "s/a_10.png", "s/a_11.png", "s/a_11.png"]
    g = sequences.group_tracks(names, person_id=np.array([7, 3, 3, 7]))        # the second frame lists the two people the other way round
    assert g["order"].tolist() == [0, 3, 1, 2] and g["offsets"].tolist() == [0, 2, 4] and g["frames"].tolist() == [10, 11, 10, 11]
    assert g["names"] == ["s#7", "s#3"]
    with pytest.raises(ValueError, match="person_id"):
        sequences.group_tracks(names, person_id=np.array([1, 2]))


def test_rows_out_of_frame_order_and_tracks_in_first_row_order():
    names = ["b/f5.jpg", "a/f2.jpg", "b/f3.jpg", "a/f1.jpg", "b/f4.jpg"]
    g = sequences.group_tracks(names)
    assert g["names"] == ["b#0", "a#0"]                                        # b's first row comes first in the file
    assert g["order"].tolist() == [2, 4, 0, 3, 1] and g["frames"].tolist() == [3, 4, 5, 1, 2] and g["offsets"].tolist() == [0, 3, 5]


def test_two_folders_with_the_same_basenames_are_two_tracks():
    names = ["S9/walk/000001.jpg", "S11/walk/000001.jpg", "S9/walk/000002.jpg", "S11/walk/000002.jpg"]
    g = sequences.group_tracks(names)
    assert g["names"] == ["S9/walk#0", "S11/walk#0"] and g["order"].tolist() == [0, 2, 1, 3] and g["offsets"].tolist() == [0, 2, 4]


def test_a_gap_in_the_frame_ids_stays_in_the_track_and_the_last_run_of_digits_counts():
    names =["v1/cam2_frame_0007.jpg", "v1/cam2_frame_0008.jpg", "v1/cam2_frame_0012.jpg", "noext_3"]
    g = sequences.group_tracks(names)
    assert g["frames"].tolist() == [7, 8, 12, 3] and g["offsets"].tolist() == [0, 3, 4] and g["names"] == ["v1#0", "#0"]
    out = accel_np.track_accel(np.zeros((4, 1, 3)), None, g["frames"], g["offsets"])
    assert not out["valid"].any()                                              # 7, 8, 12: no row has both neighbours one frame away


def test_both_value_errors():
    with pytest.raises(ValueError, match="row 1"):
        sequences.group_tracks(["a/img_1.jpg", "a/cover.jpg"])
    with pytest.raises(ValueError, match="rows 0 and 2"):
        sequences.group_tracks(["a/img_1.jpg", "a/img_2.jpg", "a/img_01.jpg"], person_id=[0, 0, 0])


# ---- --seq_post and the refusals -------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt", "--j_regressor", "none.npy", "--dataset", "none.npz"]


def test_seq_post_parsing():
    assert sequences.parse_pipelines(None) == [] and sequences.parse_pipelines("") == []
    p = sequences.parse_pipelines("infill:0.3, smooth_uncert:10 ,infill:0.25+smooth_uncert:1e2+smooth,smooth")
    assert p == [[("infill", 0.3)], [("smooth_uncert", 10.0)], [("infill", 0.25), ("smooth_uncert", 100.0), ("smooth", None)],
                 [("smooth", None)]]
    assert [sequences.pipeline_text(x) for x in p] == ["infill:0.3", "smooth_uncert:10", "infill:0.25+smooth_uncert:100+smooth", "smooth"]
    for bad, word in (("infill", "finite parameter"), ("infill:", "finite parameter"), ("infill:x", "finite parameter"),
                      ("infill:nan", "finite parameter"), ("smooth_uncert:0", "(0, 1e4]"), ("smooth_uncert:20000", "(0, 1e4]"),
                      ("smooth:3", "no parameter"), ("median:3", "unknown step"), ("infill:0.3+", "unknown step"),
                      ("smooth,smooth,smooth,smooth,smooth", "at most 4")):
        with pytest.raises(ValueError) as e:
            sequences.parse_pipelines(bad)
        assert word in str(e.value), (bad, e.value)


def test_eval_flags_parse_and_are_refused_where_they_cannot_work():
    import eval as ev
    a = ev.parse_args(BASE)
    assert a.sequences is False and a.seq_post is None and a.seq_max_gap is None and a.seq_uncert_ref is None
    a = ev.parse_args(BASE + ["--sequences", "--seq_post", "infill:0.3", "--seq_max_gap", "8", "--seq_uncert_ref", "0.5", "--beta", "0.7"])
    assert a.sequences and a.seq_post == "infill:0.3" and a.seq_max_gap == 8 and a.seq_uncert_ref == 0.5 and a.beta == 0.7
    assert sequences.flag_error(a) is None and sequences.flag_error(ev.parse_args(BASE)) is None
    seq = ["--sequences"]
    for flags, word in ((["--seq_post", "infill:0.3"], "needs --sequences"), (["--seq_max_gap", "8"], "needs --sequences"),
                        (["--seq_uncert_ref", "0.5"], "needs --sequences"), (["--min_cutoff", "0.1"], "needs --sequences"),
                        (["--beta", "1"], "needs --sequences"),
                        (seq + ["--cfg2", "x.yaml"], "--cfg2"), (seq + ["--ckpt2", "x.pt"], "--ckpt2"),
                        (seq + ["--tta", "flip"], "--tta"), (seq + ["--segm"], "--segm"),
                        (seq + ["--likelihood"], "--likelihood"), (seq + ["--rank_metrics"], "--rank_metrics"),
                        (seq + ["--aug_rot", "10"], "--aug_rot"), (seq + ["--aug_scale", "1.1"], "--aug_scale"),
                        (seq + ["--aug_flip"], "--aug_flip"), (seq + ["--aug_noise", "1,1,1"], "--aug_noise"),
                        (seq + ["--aug_occlude", "occ.npz"], "--aug_occlude"), (seq + ["--augment"], "--augment"),
                        (seq + ["--seq_post", "median:3"], "unknown step"), (seq + ["--seq_max_gap", "0"], "--seq_max_gap"),
                        (seq + ["--seq_uncert_ref", "0"], "--seq_uncert_ref")):
        with pytest.raises(SystemExit) as e:                                   # before any GPU work: no engine, no dataset needed
            ev.main(ev.parse_args(BASE + flags))
        assert word in str(e.value), (flags, e.value)


def test_a_dataset_that_does_not_group_is_refused_before_the_engine(tmp_path):
    import eval as ev
    np.savez(tmp_path / "ds.npz", imgname=np.array(["a/1.jpg", "a/cover.jpg"]), center=np.zeros((2, 2), np.float32),
             scale=np.ones(2, np.float32), pose=np.zeros((2, 72), np.float32), shape=np.zeros((2, 10), np.float32))
    with pytest.raises(SystemExit) as e:
        ev.main(ev.parse_args(BASE[:-1] + [str(tmp_path / "ds.npz"), "--sequences"]))
    assert "row 1" in str(e.value)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_exports_and_checks_its_arguments():
    L = _lib.lib()
    for sym in ("poco_op_track_accel", "poco_evaluator_copy_records"):
        assert sym in _lib.header_symbols() and hasattr(L, sym), sym
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and "#define POCO_ACCEL_MAX_JOINTS 32" in txt and "POCO_ACCEL_SCRATCH_DOUBLES(N)" in txt
    fake, null = C.c_void_p(4096), C.c_void_p(0)

    def call(pred=fake, gt=fake, stride=416, M=14, frames=fake, offsets=fake, P=2, N=10, scratch=fake, accel=fake, err=fake, sums=fake,
             total=fake, max_blocks=0):
        return L.poco_op_track_accel(pred, gt, stride, M, frames, offsets, P, N, scratch, accel, err, sums, total, max_blocks, null)
    for kw in (dict(M=0), dict(M=33), dict(M=-1), dict(stride=41), dict(stride=3, M=2), dict(stride=65537), dict(P=0), dict(N=1),
               dict(N=(1 << 24) + 1), dict(pred=null), dict(frames=null), dict(offsets=null), dict(scratch=null), dict(accel=null),
               dict(err=null), dict(sums=null), dict(total=null), dict(max_blocks=-1)):
        assert call(**kw) == 1, kw
        assert "poco_op_track_accel" in L.poco_last_error().decode(), kw
    assert L.poco_evaluator_copy_records(null, null, C.c_int64(1), fake, null) == 1
    assert "poco_evaluator_copy_records" in L.poco_last_error().decode()


def test_ops_track_accel_refuses_bad_arguments_without_a_gpu():
    import torch
    from poco_amd import ops
    assert ops.accel_scratch_doubles(10) == 30
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                          # noqa: E731
    ok = dict(pred=torch.zeros(6, 14, 3), gt=torch.zeros(6, 14, 3), frames=i32(range(6)), offsets=i32([0, 2, 6]))
    for kw, word in ((dict(pred=torch.zeros(6, 0, 3), gt=None), "M = 0"), (dict(pred=torch.zeros(6, 33, 3), gt=None), "M = 33"),
                     (dict(pred=torch.zeros(6, 99)[:, ::3], gt=None), "adjacent"),
                     (dict(pred=torch.zeros(6, 14, 6)[:, :, :3], gt=None), "adjacent"),
                     (dict(gt=torch.zeros(6, 416)[:, :42]), "row stride"),
                     (dict(offsets=i32([0, 2, 2, 6])), "increase strictly"), (dict(offsets=i32([0, 4, 2, 6])), "increase strictly"),
                     (dict(offsets=i32([0, 2, 5])), "end at N"), (dict(offsets=i32([1, 2, 6])), "start at 0"),
                     (dict(offsets=i32([6])), "P >= 1"), (dict(frames=i32(range(5))), "frames"), (dict(max_blocks=-1), "max_blocks"),
                     ({}, "CUDA")):
        with pytest.raises(_lib.PocoHipError) as e:
            ops.track_accel(**{**ok, **kw})
        assert "track_accel" in str(e.value) and word in str(e.value), (kw, e.value)


# ---- the restatement on a motion whose acceleration is known -------------------------------------------------------------------
def test_accel_np_on_uniform_acceleration():
    r = np.random.default_rng(29)
    T, M = 12, 14
    a = r.standard_normal((M, 3))
    x0, v0 = r.standard_normal((M, 3)), 0.1 * r.standard_normal((M, 3))
    frames = np.array([3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15])               # a hole after frame 7
    tt = frames[:, None, None].astype(np.float64)
    moving = x0 + v0 * tt + 0.5 * a * tt * tt
    rest = np.broadcast_to(x0, moving.shape)
    want = np.linalg.norm(a, axis=1).mean()
    offsets = np.array([0, T])
    valid = np.array([0, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0], bool)
    for gt, err in ((rest, want), (moving, 0.0), (None, None)):
        out = accel_np.track_accel(moving, gt, frames, offsets)
        assert np.array_equal(out["valid"], valid) and np.array_equal(np.isnan(out["accel64"]), ~valid)
        assert np.abs(out["accel64"][valid] - want).max() < 1e-11
        if gt is None:
            assert np.isnan(out["accel_err64"]).all() and out["total"][0] == 0.0
        else:
            assert np.array_equal(np.isnan(out["accel_err64"]), ~valid) and np.abs(out["accel_err64"][valid] - err).max() < 1e-11
            assert abs(out["total"][0] - err * valid.sum()) < 1e-10
        assert out["total"][2] == valid.sum() and abs(out["total"][1] - want * valid.sum()) < 1e-10
        assert np.array_equal(out["track_sums"][0], out["total"])
    # two tracks: the rows at the seam are invalid although their frame ids are consecutive
    out = accel_np.track_accel(moving, rest, np.arange(T), np.array([0, 5, T]))
    assert out["valid"].tolist() == [False, True, True, True, False, False, True, True, True, True, True, False]
    assert out["track_sums"][:, 2].tolist() == [3.0, 5.0]
    assert accel_np.ulp_distance(np.float32([1.0, -1.0, np.nan]), [1.0 + 2.0 ** -23, -1.0, 0.0]).tolist() == [1, 0, -1]
