"""eval.py --bootstrap on the GPU (poco_amd/bootstrap.py), on the synthetic fixtures of tests/test_eval_rank_gpu.py
and tests/test_eval_gpu.py: the argument changes nothing that was there, the point estimates are finish()'s numbers, the same seed gives
the same bits, two models with the same weights differ by exactly nothing, track units and crop units equal the restatement
tests/boot_np.py fed the same planes, and the --cfg2, --tta and --kp_refit loops hand out their labels."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import bootstrap, evaluate, synth
from poco_amd.sequences import group_tracks
from tests import boot_np, util
from tests.test_eval_gpu import _synthetic_eval_files
from tests.test_eval_rank_gpu import SEL, host_inputs, stepped

pytestmark = pytest.mark.gpu
NSTAT = len(bootstrap.STAT_NAMES)
# The summary against the restatement: both form the same statistics from moment sums that agree within U x 2^-52 relative (the
# device's order of additions against math.fsum).  A mean carries that error as it is; Pearson's r divides centred sums whose
# cancellation is mild here (|r| < 0.9, variances of the order of the second moments), so 1e-9 relative leaves six orders of room
# over 2^-52 x U x 100 and still tells any wrong draw, unit or column apart.
RTOL = 1e-9


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eval_boot")
    base = _synthetic_eval_files(tmp)
    return tmp, base


@pytest.fixture(scope="module")
def model(cuda):
    return util.make_engine("resnet50-cliff", max_batch=16, weights=util.synth_weights("resnet50-cliff"))


def same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b or (a != a and b != b)


def test_run_eval_with_and_without_bootstrap(cuda, model, files, tmp_path):
    tmp, _ = files
    ds = evaluate.EvalDataset(str(tmp / "ds_img.npz"), None, "3dpw")
    J = synth.synth_j_regressor_h36m(11)
    B = 200
    plain = evaluate.run_eval(model, ds, J, batch_size=16)
    boot = evaluate.run_eval(model, ds, J, batch_size=16, bootstrap=bootstrap.BootSpec(B, seed=3))
    assert set(boot) - set(plain) == set(bootstrap.NPZ_KEYS) and not set(plain) - set(boot)
    assert all(same(v, boot[k]) for k, v in plain.items())
    s = boot["boot_summary"]
    assert boot["boot_names"].tolist() == list(bootstrap.STAT_NAMES) and s.shape == (NSTAT, 5)
    assert boot["boot_spec"].tolist() == [B, len(ds), 0.95, 3]
    for row, key in enumerate(("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")):
        print(key, plain[key], s[row].tolist())
        assert abs(s[row, 0] - plain[key]) <= 1e-12 * abs(plain[key]), key
    assert np.all(s[:3, 2] <= s[:3, 0]) and np.all(s[:3, 0] <= s[:3, 3]) and np.all(s[:, 1] > 0) and np.all(s[:, 4] == B)
    assert np.all(np.abs(s[3:, :4]) <= 1.0) and np.all(s[:, 2] < s[:, 3])
    again = evaluate.run_eval(model, ds, J, batch_size=16, bootstrap=bootstrap.BootSpec(B, seed=3), save_results=True)
    assert np.array_equal(again["boot_summary"].view(np.uint64), s.view(np.uint64))             # the same seed: the same bits
    reps = again["boot_replicates"]
    assert reps.shape == (B, NSTAT) and np.allclose(np.std(reps, axis=0, ddof=1), s[:, 1], rtol=1e-12, atol=0)
    other = evaluate.run_eval(model, ds, J, batch_size=16, bootstrap=bootstrap.BootSpec(B, seed=4))
    assert np.array_equal(other["boot_summary"][:, 0], s[:, 0]) and not np.array_equal(other["boot_summary"][:, 1:4], s[:, 1:4])
    evaluate.save_npz(str(tmp_path / "plain.npz"), plain, "3dpw")
    evaluate.save_npz(str(tmp_path / "boot.npz"), boot, "3dpw")
    zp, zb = dict(np.load(tmp_path / "plain.npz")), dict(np.load(tmp_path / "boot.npz"))
    assert set(zb) - set(zp) == set(bootstrap.NPZ_KEYS) and not any(k.startswith("boot_") for k in zp)
    assert all(same(zp[k], zb[k]) for k in zp) and zb["boot_names"].tolist() == list(bootstrap.STAT_NAMES)
    lines = bootstrap.report_lines(boot)
    assert len(lines) == 1 + NSTAT and lines[0].startswith(f"Bootstrap: {B} replicates of {len(ds)} units") and lines[1].startswith("MPJPE  ")
    assert lines[1].endswith(f"({B}/{B})") and "+-" in lines[1] and "[" in lines[1]


def test_two_models_with_the_same_weights_differ_by_exactly_nothing(cuda, model, files):
    from poco_amd import select
    tmp, _ = files
    twin = util.make_engine("resnet50-cliff", max_batch=16, weights=util.synth_weights("resnet50-cliff"))
    ds = evaluate.EvalDataset(str(tmp / "ds_img.npz"), None, "3dpw")
    J = synth.synth_j_regressor_h36m(11)
    plain = evaluate.run_eval_pair(select.RegressorPair(model, twin), ds, J, batch_size=16)
    res = evaluate.run_eval_pair(select.RegressorPair(model, twin), ds, J, batch_size=16, bootstrap=bootstrap.BootSpec(64))
    assert set(res) - set(plain) == set(bootstrap.NPZ_KEYS) and all(same(v, res[k]) for k, v in plain.items())
    names, s = res["boot_names"].tolist(), res["boot_summary"]
    assert len(names) == 5 * NSTAT and names[0] == "Model 1 MPJPE" and names[NSTAT] == "Model 2 MPJPE"
    assert names[2 * NSTAT] == "Model 2 - Model 1 MPJPE" and names[3 * NSTAT] == "Selected MPJPE" and names[4 * NSTAT + 3] == "Selected - Model 1 Uncert Error Correlation"
    for lo in (2 * NSTAT, 4 * NSTAT):                                     # the paired differences: point 0, se 0, [0, 0], every replicate valid
        assert np.all(s[lo:lo + NSTAT, :4] == 0.0) and np.all(s[lo:lo + NSTAT, 4] == 64), s[lo:lo + NSTAT]
    assert np.array_equal(s[:NSTAT].view(np.uint64), s[NSTAT:2 * NSTAT].view(np.uint64)) and np.all(s[:NSTAT, 1] > 0)
    for row, key in enumerate(("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr")):
        assert abs(s[row, 0] - res[key + "_m1"]) <= 1e-12 * abs(res[key + "_m1"]) and abs(s[3 * NSTAT + row, 0] - res[key]) <= 1e-12 * abs(res[key])


def _host_planes(evs):
    crop, joint = [], []
    for ev in evs:
        (ck, cv), (jk, jv) = host_inputs(ev.finish(return_records=True)["records"], SEL)
        crop += [ck[None], cv]
        joint += [jk[None], jv]
    return np.concatenate(crop), np.concatenate(joint)


def _agree(got, want):
    assert got.shape == want.shape and np.array_equal(got[:, 4], want[:, 4])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    rel = np.abs(got - want)[ok] / np.maximum(np.abs(want)[ok], 1e-300)
    print("largest relative deviation of the summary from the restatement:", float(rel.max()))
    assert np.all(np.abs(got - want)[ok] <= RTOL * np.abs(want)[ok])


def test_track_units_equal_the_restatement(cuda):
    ev = stepped(cuda, [5, 3, 70], SEL, seed=21)
    N, S, B, seed = 78, len(SEL), 40, 9
    names = [f"{'abc'[i % 3]}/cam/im_{i // 3:05d}.png" for i in range(N)]                       # three tracks, interleaved in the file
    names[4], names[7] = names[7], names[4]                                                    # and one of them out of frame order
    res = bootstrap.bootstrap_evaluators([("", ev)], bootstrap.BootSpec(B, "track", 0.9, seed), imgname=names)
    assert res["boot_spec"].tolist() == [B, 3, 0.9, seed] and res["boot_names"].tolist() == list(bootstrap.STAT_NAMES)
    g = group_tracks(names)
    assert len(g["offsets"]) == 4
    crop, joint = _host_planes([ev])
    order = g["order"].astype(np.int64)
    jrows = (order[:, None] * S + np.arange(S)[None]).reshape(-1)
    want = boot_np.evaluator_summary(crop[:, order], joint[:, jrows], g["offsets"], S, B, seed, 0.9)
    _agree(res["boot_summary"], want)
    with pytest.raises(ValueError, match="frame number"):
        bootstrap.bootstrap_evaluators([("", ev)], bootstrap.BootSpec(B, "track"), imgname=["x.png"] * N)
    with pytest.raises(ValueError, match="imgname"):
        bootstrap.bootstrap_evaluators([("", ev)], bootstrap.BootSpec(B, "track"))
    ev.close()


def test_crop_units_of_two_labels_equal_the_restatement(cuda):
    evs = [stepped(cuda, [70, 8], SEL, seed=21), stepped(cuda, [70, 8], SEL, seed=22)]
    B, seed = 30, 2 ** 40 + 1
    res = bootstrap.bootstrap_evaluators(list(zip(("A", "B"), evs)), bootstrap.BootSpec(B, seed=seed), save_replicates=True)
    assert len(res["boot_names"]) == 3 * NSTAT and res["boot_replicates"].shape == (B, 3 * NSTAT) and res["boot_spec"][1] == 78
    crop, joint = _host_planes(evs)
    _agree(res["boot_summary"], boot_np.evaluator_summary(crop, joint, None, len(SEL), B, seed, 0.95))
    short = stepped(cuda, [70], SEL, seed=23)
    with pytest.raises(ValueError, match="same number of crops"):
        bootstrap.bootstrap_evaluators([("A", evs[0]), ("B", short)], bootstrap.BootSpec(B))
    for ev in evs + [short]:
        ev.close()


def test_tta_and_refit_loops_hand_out_their_labels(cuda, model, files):
    from poco_amd import refit, tta
    tmp, base = files
    J = synth.synth_j_regressor_h36m(11)
    spec = bootstrap.BootSpec(16)
    ds = evaluate.EvalDataset(str(tmp / "ds_files.npz"), str(tmp / "imgs"), crop="dataset")
    res = evaluate.run_eval_tta(tta.TTAModel(model, tta.parse_views("flip"), "uncert"), ds, J, batch_size=16, bootstrap=spec)
    names = res["boot_names"].tolist()
    assert len(names) == 3 * NSTAT and names[0] == "Base view MPJPE" and names[NSTAT] == "Fused MPJPE" and names[2 * NSTAT] == "Fused - Base view MPJPE"
    s = res["boot_summary"]
    assert abs(s[0, 0] - res["val_mpjpe_base"]) <= 1e-12 * res["val_mpjpe_base"] and abs(s[NSTAT, 0] - res["val_mpjpe"]) <= 1e-12 * res["val_mpjpe"]
    assert abs(s[2 * NSTAT, 0] - (s[NSTAT, 0] - s[0, 0])) <= 1e-12 * s[0, 0] and np.all(s[:, 4] == 16)
    n = len(base["imgname"])
    r = np.random.default_rng(8)
    kp = np.concatenate([base["center"][:, None, :] + r.uniform(-60, 60, (n, 25, 2)), r.uniform(0.4, 1.0, (n, 25, 1))], axis=2).astype(np.float32)
    with np.load(tmp / "ds_img.npz") as z:
        np.savez(tmp / "ds_kp.npz", openpose=kp, **{k: z[k] for k in z.files})
    ds = evaluate.EvalDataset(str(tmp / "ds_kp.npz"), None, "3dpw")
    res = evaluate.run_eval_refit(model, ds, J, refit.joint_tables(str(tmp / "smpl.npz")), 1.0, batch_size=16, bootstrap=spec)
    names = res["boot_names"].tolist()
    assert len(names) == 3 * NSTAT and names[0] == "Raw MPJPE" and names[NSTAT] == "Refit MPJPE" and names[2 * NSTAT + 1] == "Refit - Raw PA-MPJPE"
    s = res["boot_summary"]
    assert abs(s[0, 0] - res["val_mpjpe_raw"]) <= 1e-12 * res["val_mpjpe_raw"] and abs(s[NSTAT + 3, 0] - res["val_corr"]) <= 1e-12 * abs(res["val_corr"])


def test_eval_cli_prints_the_block_and_writes_the_keys(files, tmp_path, cuda, capsys):
    tmp, _ = files
    spec = importlib.util.spec_from_file_location("poco_eval_cli_boot_gpu", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    argv = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "ckpt.pt"), "--smpl", str(tmp / "smpl.npz"),
            "--j_regressor", str(tmp / "J.npy"), "--dataset", str(tmp / "ds_img.npz"), "--batch_size", "16", "--output_folder", str(tmp_path / "out"),
            "--bootstrap", "25", "--boot_level", "0.8", "--boot_seed", "6", "--save_results"]
    res = cli.main(cli.parse_args(argv))
    printed = capsys.readouterr().out.splitlines()
    lines = bootstrap.report_lines(res)
    assert printed[-len(lines):] == lines and printed[-len(lines) - 5:-len(lines)] == evaluate.report_lines(res)
    z = dict(np.load(tmp_path / "out" / "evaluation_results_3dpw.npz"))
    assert z["boot_summary"].shape == (NSTAT, 5) and z["boot_spec"].tolist() == [25, 40, 0.8, 6] and z["boot_replicates"].shape == (25, NSTAT)
    assert z["boot_names"].tolist() == list(bootstrap.STAT_NAMES)
