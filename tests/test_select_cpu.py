"""CPU: the contract of choosing between two regressors pinned on hand-checkable rows of its numpy restatement
tests/select_np.py - the yardstick of tests/test_select_gpu.py - plus the C ABI's declaration and argument checks (fake pointers,
refused before any GPU work), the flag refusals of demo.py and eval.py and
the per-row host helpers of poco_amd/select.py."""
import ctypes as C

import numpy as np
import pytest

from poco_amd import _lib
from tests import select_np as snp

THR = 0.40


def _rows(var0, var1, seed=0):
    """Two models' rows from their var [B,24]; pose and one payload carry the model in every word (0.x against 1.x)."""
    var0, var1 = np.asarray(var0, np.float32).reshape(-1, 24), np.asarray(var1, np.float32).reshape(-1, 24)
    B = len(var0)
    r = np.random.default_rng(seed)
    pose0, pose1 = r.uniform(0, 0.9, (B, 24, 3, 3)).astype(np.float32), r.uniform(1, 1.9, (B, 24, 3, 3)).astype(np.float32)
    pay = (r.uniform(0, 0.9, (B, 5)).astype(np.float32), r.uniform(1, 1.9, (B, 5)).astype(np.float32))
    return dict(pose0=pose0, var0=var0, pose1=pose1, var1=var1, payloads=[pay])


def _sel(var0, var1, kind0=1, kind1=1, kinematic=False, thr=THR, scale=1.0, mode=0):
    d = _rows(var0, var1)
    return d, snp.select(d["pose0"], d["var0"], kind0, d["pose1"], d["var1"], kind1, kinematic, thr, scale, mode, d["payloads"])


def _flat(v):
    return np.full(24, v, np.float32)


def test_a_tie_goes_to_model_0_and_the_lower_score_wins():
    d, o = _sel([_flat(0.2), _flat(0.2), _flat(0.1)], [_flat(0.2), _flat(0.1), _flat(0.2)])
    assert o["choice"][:, 0].tolist() == [0, 1, 0]
    assert (o["choice"] == o["choice"][:, :1]).all() and not o["mixed"].any() and o["rows"].size == 0
    assert np.array_equal(o["score"], np.float32([[0.2, 0.2], [0.2, 0.1], [0.1, 0.2]]))
    # copies, bit for bit, from the chosen model; the payload follows the root
    assert np.array_equal(o["pose"][1], d["pose1"][1]) and np.array_equal(o["pose"][0], d["pose0"][0])
    assert np.array_equal(o["var"][1], d["var1"][1]) and np.array_equal(o["var"][2], d["var0"][2])
    assert np.array_equal(o["payloads"][0], np.stack([d["payloads"][0][0][0], d["payloads"][0][1][1], d["payloads"][0][0][2]]))


@pytest.mark.parametrize("mode", [0, 1])
def test_nan_in_either_model_or_both_takes_model_0(mode):
    nan = _flat(np.nan)
    _, o = _sel([nan, _flat(0.3), nan], [_flat(0.1), nan, nan], mode=mode)
    assert not o["choice"].any() and not o["mixed"].any()
    assert o["score"].view(np.uint32).tolist() == [[0x7FC00000, np.float32(0.1).view(np.uint32)],
                                                   [np.float32(0.3).view(np.uint32), 0x7FC00000], [0x7FC00000, 0x7FC00000]]


def test_a_single_nan_joint_in_joint_mode_keeps_model_0_there_only():
    v0 = _flat(0.3)
    v0[7] = np.nan
    _, o = _sel([v0], [_flat(0.1)], mode=1)
    assert o["choice"][0].tolist() == [1] * 7 + [0] + [1] * 16 and o["mixed"].tolist() == [1]


def test_scale_flips_a_decision():
    v0, v1 = [_flat(0.2)], [_flat(0.3)]
    assert _sel(v0, v1, scale=1.0)[1]["choice"][0, 0] == 0
    _, o = _sel(v0, v1, scale=0.5)
    assert o["choice"][0, 0] == 1 and o["score"][0].tolist() == [np.float32(0.2), np.float32(0.5 * float(np.float32(0.3)))]
    assert _sel([_flat(0.3)], [_flat(0.2)], scale=2.0)[1]["choice"][0, 0] == 0


def test_kinematic_changes_a_childs_decision_but_not_the_roots():
    v0, v1 = _flat(0.1), _flat(0.1)
    v0[0], v1[0] = 0.05, 0.20                        # the root: model 0 either way
    v0[1], v1[1] = 0.20, 0.10                        # child 1 of the root: raw -> model 1; accumulated 0.25 against 0.30 -> model 0
    off = _sel([v0], [v1], kinematic=False, mode=1)[1]
    on = _sel([v0], [v1], kinematic=True, mode=1)[1]
    assert off["choice"][0, 0] == 0 and on["choice"][0, 0] == 0
    assert off["choice"][0, 1] == 1 and on["choice"][0, 1] == 0
    # the accumulation is postproc.kinematic_uncert's: fp32 additions in child order
    assert on["u"][0, 0, 1] == np.float32(np.float32(0.20) + np.float32(0.05))
    assert on["u"][0, 0, 4] == np.float32(np.float32(0.1) + on["u"][0, 0, 1])
    from poco_amd import postproc
    r = np.random.default_rng(5)
    v = r.uniform(0, 1, (6, 24)).astype(np.float32)
    got = np.stack([snp.processed(row, True) for row in v])
    assert np.array_equal(got, postproc.kinematic_uncert(v))


def test_the_threshold_rules_turn_a_score_into_exactly_one():
    thr = 0.25                                                        # exact in fp32 and fp64, and so is 2 thr
    # kind 1 (root rule): above 2 thr -> 1.0; equal to 2 thr -> the value itself
    _, o = _sel([_flat(0.75), _flat(0.5)], [_flat(0.9), _flat(0.9)], kind0=1, kind1=1, thr=thr)
    assert o["score"][:, 0].tolist() == [1.0, 0.5] and o["score"][:, 1].tolist() == [1.0, 1.0]
    assert o["choice"][:, 0].tolist() == [0, 0]                       # 1.0 against 1.0 is a tie
    # kind 0 (mean rule): the root above thr -> 1.0; equal to thr -> the mean
    a, b = _flat(0.125), _flat(0.125)
    a[0], b[0] = 0.5, 0.25
    _, o = _sel([a, b], [_flat(0.9), _flat(0.9)], kind0=0, kind1=1, thr=thr)
    assert o["score"][0, 0] == 1.0 and o["score"][1, 0] == np.float32((0.25 + 23 * 0.125) / 24)
    # in joint mode the 1.0 rule does not decide, but the score is still written
    _, o = _sel([_flat(0.75)], [_flat(0.9)], thr=thr, mode=1)
    assert o["score"][0].tolist() == [1.0, 1.0] and not o["choice"].any()
    _, o = _sel([_flat(0.95)], [_flat(0.9)], thr=thr, mode=1)
    assert o["score"][0].tolist() == [1.0, 1.0] and o["choice"].all()


def test_the_kind_0_mean_is_the_float64_sum_in_joint_order():
    r = np.random.default_rng(2)
    v = r.uniform(0, 0.3, 24).astype(np.float32)
    s = 0.0
    for x in v:
        s += float(x)
    _, o = _sel([v], [_flat(0.0)], kind0=0)
    assert o["score"][0, 0] == np.float32(s / 24) and o["choice"][0, 0] == 1
    _, o = _sel([_flat(0.2)], [v], kind0=1, kind1=0, scale=0.5)
    assert o["score"][0, 1] == np.float32(0.5 * (s / 24))


def test_joint_mode_makes_mixed_rows_and_their_ordered_list_and_crop_mode_never_does():
    r = np.random.default_rng(3)
    v0, v1 = r.uniform(0, 0.3, (9, 24)).astype(np.float32), r.uniform(0, 0.3, (9, 24)).astype(np.float32)
    v1[2] = v0[2] + 1                                                 # all from model 0
    v1[5] = v0[5] / 2                                                 # all from model 1
    d, o = _sel(v0, v1, mode=1)
    assert o["mixed"].tolist() == [1, 1, 0, 1, 1, 0, 1, 1, 1] and o["rows"].tolist() == [0, 1, 3, 4, 6, 7, 8]
    assert not o["choice"][2].any() and o["choice"][5].all()
    assert np.array_equal(o["choice"], (v1 < v0).astype(np.uint8))
    for t in range(9):
        for j in range(24):
            src = d["pose1"] if o["choice"][t, j] else d["pose0"]
            assert np.array_equal(o["pose"][t, j], src[t, j])
        pay = d["payloads"][0][int(o["choice"][t, 0])]
        assert np.array_equal(o["payloads"][0][t], pay[t])            # the payload follows the root, also in a mixed row
    _, o = _sel(v0, v1, mode=0)
    assert not o["mixed"].any() and o["rows"].size == 0 and (o["choice"] == o["choice"][:, :1]).all()
    assert 0 < o["choice"][:, 0].sum() < 9


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_c_abi_declares_the_entry_and_refuses_bad_arguments():
    from poco_amd import ops
    L = _lib.lib()
    assert "poco_op_select_regressor" in _lib.header_symbols() and hasattr(L, "poco_op_select_regressor")
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and "#define POCO_SELECT_MAX_PAYLOADS 8" in txt            # additions only
    assert L.poco_abi_version() == 4
    fn = L.poco_op_select_regressor
    fn.argtypes = ops.SELECT_ARGTYPES
    fake, other, null = 4096, 8192, None
    one = [(fake, fake, other, 3)]

    def call(pose0=fake, var0=fake, kind0=1, pose1=fake, var1=fake, kind1=0, B=4, kinematic=1, thr=0.4, scale=1.0, mode=0, pay=one,
             pose_out=other, var_out=other, choice=fake, score=fake, mixed=fake, rows=null, count=null):
        return fn(pose0, var0, kind0, pose1, var1, kind1, B, kinematic, thr, scale, mode, ops.select_payloads(pay), pose_out, var_out,
                  choice, score, mixed, rows, count, 0, None)
    bad = [dict(pose0=null), dict(var0=null), dict(pose1=null), dict(var1=null), dict(pose_out=null), dict(var_out=null),
           dict(choice=null), dict(score=null), dict(mixed=null), dict(B=0), dict(B=-3), dict(mode=2), dict(mode=-1), dict(kind0=2),
           dict(kind1=-1), dict(kinematic=2), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(pay=[(fake, fake, other, 3)] * 9), dict(pay=[(fake, fake, other, 0)]), dict(pay=[(fake, fake, other, -2)]),
           dict(pay=[(null, fake, other, 3)]), dict(pay=[(fake, null, other, 3)]), dict(pay=[(fake, fake, null, 3)]),
           dict(pay=[(fake, fake, fake, 3)]), dict(pose_out=fake), dict(var_out=fake), dict(rows=fake), dict(count=fake)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "select_regressor" in L.poco_last_error().decode(), kw


def test_ops_select_regressor_refuses_bad_arguments_without_a_gpu():
    """The wrapper's own checks come before any GPU work; host tensors are refused as such."""
    import torch
    from poco_amd import ops
    with pytest.raises(_lib.PocoHipError, match="select_regressor.*CUDA"):
        ops.select_regressor(torch.zeros(2, 24, 3, 3), torch.zeros(2, 24), 1, torch.zeros(2, 24, 3, 3), torch.zeros(2, 24), 1)


# ---- demo.py ---------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]
PAIR = ["--cfg2", "configs/demo_poco_pare.yaml", "--ckpt2", "none2.pt"]


def test_demo_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    import demo
    a = demo.parse_args(BASE)
    assert a.cfg2 is None and a.ckpt2 is None and a.select is None and a.select_scale is None and a.inf_model2 == "best"
    a = demo.parse_args(BASE + PAIR + ["--select", "joint", "--select_scale", "0.5", "--inf_model2", "last"])
    assert (a.cfg2, a.ckpt2, a.select, a.select_scale, a.inf_model2) == ("configs/demo_poco_pare.yaml", "none2.pt", "joint", 0.5, "last")
    with pytest.raises(SystemExit):
        demo.parse_args(BASE + PAIR + ["--select", "frame"])
    for flags, word in ((["--ckpt2", "x.pt"], "--cfg2"), (["--cfg2", "configs/demo_poco_pare.yaml"], "--ckpt2"),
                        (["--select", "crop"], "--cfg2"), (["--select_scale", "2"], "--cfg2"),
                        (PAIR + ["--select_scale", "0"], "--select_scale"), (PAIR + ["--select_scale", "-1"], "--select_scale"),
                        (PAIR + ["--select_scale", "inf"], "--select_scale"), (PAIR + ["--select_scale", "nan"], "--select_scale"),
                        (PAIR + ["--mode", "video", "--gpus", "2"], "--gpus"), (PAIR + ["--occlusion_map"], "--occlusion_map"),
                        (PAIR + ["--save_dataset", str(tmp_path / "d.npz")], "--save_dataset"), (PAIR + ["--save_segm"], "--save_segm")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work: no engine, no input folder needed
            demo.main(demo.parse_args(BASE + flags + ["--vid_file", str(tmp_path / "missing"), "--image_folder", str(tmp_path / "missing")]))
        assert word in str(e.value) and str(e.value).count(". ") == 0, (flags, e.value)


def test_eval_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("poco_eval_cli", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = BASE + ["--j_regressor", "none.npy", "--dataset", str(tmp_path / "missing.npz")]
    a = cli.parse_args(base)
    assert a.cfg2 is None and a.ckpt2 is None and a.select is None and a.select_scale is None and a.inf_model2 == "best"
    a = cli.parse_args(base + PAIR + ["--select", "joint", "--select_scale", "0.5", "--inf_model2", "last"])
    assert (a.cfg2, a.ckpt2, a.select, a.select_scale, a.inf_model2) == ("configs/demo_poco_pare.yaml", "none2.pt", "joint", 0.5, "last")
    with pytest.raises(SystemExit):
        cli.parse_args(base + PAIR + ["--select", "frame"])
    for flags, word in ((["--ckpt2", "x.pt"], "--cfg2"), (["--cfg2", "configs/demo_poco_pare.yaml"], "--ckpt2"),
                        (["--select", "crop"], "--cfg2"), (["--select_scale", "2"], "--cfg2"),
                        (PAIR + ["--select_scale", "0"], "--select_scale"), (PAIR + ["--select_scale", "-1"], "--select_scale"),
                        (PAIR + ["--select_scale", "inf"], "--select_scale"), (PAIR + ["--select_scale", "nan"], "--select_scale"),
                        (PAIR + ["--segm"], "--segm"), (PAIR + ["--likelihood"], "--likelihood")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work, before the dataset file is looked at
            cli.main(cli.parse_args(base + flags))
        assert word in str(e.value) and "missing.npz" not in str(e.value) and str(e.value).count(". ") == 0, (flags, e.value)
    with pytest.raises(SystemExit, match="missing.npz"):                         # a pair that may run gets as far as the dataset file
        cli.main(cli.parse_args(base + PAIR))


def test_selection_summary_on_hand_checkable_crops():
    from poco_amd import evaluate
    sel = np.zeros((4, 24), np.uint8)
    sel[1] = sel[2] = 1
    sel[3, 5] = 1                                                                # a mixed row: the root's model (1) counts
    s = evaluate.selection_summary(([0.1, 0.3, 0.2, 0.5], [0.2, 0.1, 0.4, 0.5]), ([0.01, 0.02, 0.03, 0.04], [0.04, 0.03, 0.02, 0.01]), sel)
    assert s["val_oracle_mpjpe"] == 1000.0 * np.float64(0.1 + 0.1 + 0.2 + 0.5) / 4 or abs(s["val_oracle_mpjpe"] - 225.0) < 1e-10
    assert abs(s["val_oracle_pampjpe"] - 1000.0 * (0.01 + 0.02 + 0.02 + 0.01) / 4) < 1e-10
    assert s["select_accuracy"] == 0.75 and s["select_share_m2"] == 0.5          # right: rows 0, 1 and the tie of row 3; wrong: row 2


def test_the_pair_refuses_what_it_does_not_offer():
    from poco_amd import select

    class Fake:
        _finalized, max_batch, variant = True, 4, "resnet50-cliff"
        import torch
        device = torch.device("cuda:0")
    with pytest.raises(ValueError, match="mode"):
        select.RegressorPair(Fake(), Fake(), mode="frame")
    with pytest.raises(ValueError, match="scale"):
        select.RegressorPair(Fake(), Fake(), scale=0.0)
    other = Fake()
    other.max_batch = 8
    with pytest.raises(_lib.PocoHipError, match="max_batch"):
        select.RegressorPair(Fake(), other)
    pair = select.RegressorPair(Fake(), Fake(), mode="joint", scale=0.5)
    assert pair.kinds == (1, 1) and pair.max_batch == 4
    with pytest.raises(AttributeError, match="graph_forward"):
        pair.graph_forward
    with pytest.raises(_lib.PocoHipError, match="want_segm"):
        pair({}, want_segm=True)


def test_per_row_helpers_follow_the_roots_model():
    from poco_amd import postproc, select
    r = np.random.default_rng(9)
    n = 6
    var_pose = r.uniform(0, 0.5, (n, 24)).astype(np.float32)
    var_pose[0, 0], var_pose[1, 0] = 0.5, 0.9                                  # over thr only / over 2 thr too
    sel = np.zeros((n, 24), np.uint8)
    sel[[1, 3, 4], 0] = 1
    sel[2, 5] = 1                                                                # a mixed row: its root is model 0's
    backs = ("resnet50-cliff", "hrnet_w32-pare")
    for kin, clip in ((True, True), (False, False)):
        var, g = select.pair_uncert(var_pose, sel, backs, kin, clip)
        v_ref = postproc.prepare_uncert(var_pose, kin)
        assert np.array_equal(var, v_ref)
        g0, g1 = postproc.global_uncert(v_ref, backs[0], clip=clip), postproc.global_uncert(v_ref, backs[1], clip=clip)
        assert np.array_equal(g, np.where(sel[:, 0] == 1, g1, g0)) and not np.array_equal(g0, g1)
    dets = np.float32([[50, 60, 40, 40]] * n)
    j2d = r.uniform(-1, 1, (n, 49, 2)).astype(np.float32)
    out = select.pair_joints2d(j2d, sel, backs, dets, 224)
    conv = postproc.convert_crop_coords_to_orig_img(dets, j2d, 224)
    pare = sel[:, 0] == 1
    assert out.dtype == np.float32 and np.array_equal(out[pare], conv[pare]) and np.array_equal(out[~pare], j2d[~pare])
    assert select.pair_joints2d(j2d, sel, ("resnet50-cliff", "hrnet_w48_cls-cliff"), dets, 224) is j2d
    assert "3 of 6 crops from model 2" in select.summary_line(sel, 0, "crop")
    assert "4 of 144 joint-entries" in select.summary_line(sel, 1, "joint")
