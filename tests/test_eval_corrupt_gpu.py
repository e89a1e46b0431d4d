"""GPU: eval.py --corrupt end to end (resnet50-cliff, synthetic weights, eight synthetic samples on three synthetic images: the set-up
of tests/test_eval_tta_gpu.py with two more rows).

Levels gaussian_blur:2,jpeg:20+gaussian_noise:8 (K = 3 with the clean crop).  evaluate.run_eval_corrupt at batch size 24 regresses
the 3 x 8 level-major rows in one forward and hands out the crops it gave the forward and the per-level outputs:
  - level 0's per-crop records equal a run without the flag bit for bit.  The engine chooses its conv configurations by the rows of a
    forward, so two forwards of different sizes agree to the last bits only by luck (tests/test_eval_tta_gpu.py says the same of its
    base view): the run without the flag that level 0 is held to, bit for bit, is plain run_eval whose forward has the same 24 rows -
    the dataset file written three times over, rows 0..7 compared.  Against plain run_eval of the 8 rows in a forward of 8 the
    records agree within the forward's gate; measured on an MI355X: largest difference of a per-joint error 1.2e-7 m;
  - each level's crops equal tests/corrupt_np.py on the raw dataset crop within the operator's own bound (tests/test_corrupt_gpu.py:
    NORM_TOL; jpeg exactly), and the restated crops through the same forward give the level's outputs within the forward's gate of 1e-3;
  - the .npz carries the new keys, the printed lines the labels; every refusal of the flag is exercised."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import corrupt, evaluate, synth
from tests import corrupt_np, util

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = "configs/demo_poco_cliff_resnet50.yaml"
LEVELS = "gaussian_blur:2,jpeg:20+gaussian_noise:8"
SEED = 11
NORM_TOL = (2.0 ** -15 / 255.0 + 4 * 2.0 ** -25) / 0.224 + 2 * 2.0 ** -23          # tests/test_corrupt_gpu.py derives it
GATE = 1e-3


@pytest.fixture(scope="module")
def setup(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("eval_corrupt")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "ckpt.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    np.save(tmp / "J.npy", synth.synth_j_regressor_h36m(11))
    (tmp / "imgs").mkdir()
    r = np.random.default_rng(35)
    names = ["p0.png", "p1.png", "p0.png", "p2.png", "p1.png", "p2.png", "p0.png", "p1.png"]
    yy, xx = np.mgrid[0:240, 0:320]
    for i, n in enumerate(sorted(set(names))):                           # smooth pictures with some texture: blur and jpeg have something to do
        base = np.stack([128 + 100 * np.sin(xx / (9.0 + i)), 128 + 100 * np.cos(yy / (7.0 + i)), (xx + yy + 40 * i) % 256], -1)
        Image.fromarray(np.clip(base + r.integers(-25, 26, base.shape), 0, 255).astype(np.uint8)).save(tmp / "imgs" / n)
    n = len(names)
    ds = dict(imgname=np.array(names), center=r.uniform([120, 90], [200, 150], (n, 2)).astype(np.float32),
              scale=r.uniform(0.5, 1.0, n).astype(np.float32), pose=(0.3 * r.standard_normal((n, 72))).astype(np.float32),
              shape=(0.5 * r.standard_normal((n, 10))).astype(np.float32))
    np.savez(tmp / "ds.npz", **ds)
    np.savez(tmp / "ds3.npz", **{k: np.concatenate([v] * 3) for k, v in ds.items()})
    model = util.make_engine("resnet50-cliff", max_batch=24, weights=w)
    return tmp, model, ds


@pytest.fixture(scope="module")
def runs(setup, cuda):
    tmp, model, _ = setup
    J = synth.synth_j_regressor_h36m(11)
    data = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset")
    cm = corrupt.CorruptModel(model, corrupt.parse_levels(LEVELS), SEED)
    out = {"corrupt": evaluate.run_eval_corrupt(cm, data, J, batch_size=24, return_outputs=True)}
    assert data.raw_crop is False
    out["raw"] = _raw(data, 0, 8, cuda)
    data = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset")
    out["plain8"] = evaluate.run_eval(model, data, J, batch_size=8, return_records=True)
    data = evaluate.EvalDataset(str(tmp / "ds3.npz"), str(tmp / "imgs"), crop="dataset")
    out["plain"] = evaluate.run_eval(model, data, J, batch_size=24, return_records=True)
    return out


def _raw(data, lo, hi, dev):
    data.raw_crop = True
    try:
        return data.batch(lo, hi, dev)["img"].cpu().numpy()
    finally:
        data.raw_crop = False


def test_level_0_equals_a_run_without_the_flag_bit_for_bit(runs):
    res, plain, plain8 = runs["corrupt"], runs["plain"], runs["plain8"]
    assert res["N"] == plain8["N"] == 8 and plain["N"] == 24 and len(res["outputs"]) == 1
    for k in ("mpjpe", "pampjpe", "v2v"):
        assert np.array_equal(res[k], plain[k][:8]), k
        assert np.array_equal(res[k + "_l0"], plain[k][:8]), k
    sel = len(res["corr_x"])
    assert np.array_equal(res["corr_x"], plain["corr_x"][:sel]) and np.array_equal(res["corr_y"], plain["corr_y"][:sel])
    want_var = plain["records"][:8, evaluate.R_UNC:evaluate.R_UNC + 24].astype(np.float64).mean(axis=1)
    assert np.array_equal(res["var_l0"], want_var)
    # the same 8 rows in a forward of 8: within the forward's gate
    worst = max(float(np.abs(res[k] - plain8[k]).max()) for k in ("mpjpe", "pampjpe", "v2v"))
    print(f"level 0 against a forward of 8 rows: largest difference {worst:.3e} m (gate {GATE:.0e})")
    assert worst <= GATE


def test_each_levels_crops_equal_the_restatement_and_go_through_the_same_forward(setup, runs, cuda):
    _, model, _ = setup
    res, raw = runs["corrupt"], runs["raw"]
    assert raw.shape == (8, 3, 224, 224) and raw.min() >= 0 and raw.max() <= 255 and raw.max() > 200
    levels = corrupt.parse_levels(LEVELS)
    recs = corrupt.level_major_records(levels, range(8), SEED)
    got = res["outputs"][0]["level_imgs"]
    assert got.shape == (24, 3, 224, 224)
    # the restatement, level by level; jpeg through PIL (tests/test_corrupt_cpu.py holds it equal to the restatement byte for byte;
    # the pure-Python entropy coder takes seconds per 224 x 224 crop)
    from tests.test_corrupt_gpu import restate_step
    want = np.tile(raw, (3, 1, 1, 1))
    for p in range(recs.shape[1]):
        want = restate_step(want, recs[:, p], p)
    want_n = corrupt_np.normalize_np(want)
    dev = np.abs(got.astype(np.float64) - want_n).reshape(3, -1).max(axis=1)
    print("largest deviation of the normalised crops per level:", dev, f"(bound {NORM_TOL:.3e})")
    assert np.array_equal(got[:8], want_n[:8])                                        # level 0: the clean crop
    assert dev[1] <= NORM_TOL
    # level 2: the noise is added to whole bytes, so a flipped last place of z moves the raw value by at most the tolerance
    assert dev[2] <= NORM_TOL
    assert np.abs(got[8:16] - got[:8]).max() > 0.05 and np.abs(got[16:] - got[:8]).max() > 0.05
    # the restated crops through the same forward: the level's outputs within the forward's gate
    data_batch = _batch24(setup, cuda)
    data_batch["img"] = torch.from_numpy(want_n).to(cuda)
    out = model(data_batch, want_segm=False)
    for k in range(3):
        for key in ("pred_pose", "pred_shape", "pred_cam", "var_pose", "smpl_vertices", "smpl_joints3d"):
            a = out[key][8 * k:8 * (k + 1)].cpu().numpy()
            assert np.abs(a - res["outputs"][0]["levels"][k][key]).max() <= GATE, (k, key)


def _batch24(setup, cuda):
    tmp, _, _ = setup
    data = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset")
    b = data.batch(0, 8, cuda)
    return {k: v.repeat(3, *([1] * (v.dim() - 1))) for k, v in b.items()}


def test_summary_and_correlations(runs):
    res = runs["corrupt"]
    s = res["corrupt_summary"]
    assert s.shape == (3, len(evaluate.CORRUPT_SUMMARY_FIELDS)) and list(res["corrupt_levels"]) == ["clean", "gaussian_blur:2", "jpeg:20+gaussian_noise:8"]
    assert (s[0, 6:] == 0).all() and s[0, 0] == res["val_mpjpe"]
    for k in range(3):
        assert s[k, 4] == res[f"var_l{k}"].mean() and s[k, 5] == np.median(res[f"var_l{k}"])
        assert abs(s[k, 0] - 1000.0 * res[f"mpjpe_l{k}"].mean()) <= 1e-2
    assert not np.array_equal(res["mpjpe_l1"], res["mpjpe_l0"]) and not np.array_equal(res["var_l2"], res["var_l0"])
    from scipy import stats
    dv = np.concatenate([res[f"var_l{k}"] - res["var_l0"] for k in (1, 2)])
    de = np.concatenate([res[f"mpjpe_l{k}"].mean(axis=1).astype(np.float64) - res["mpjpe_l0"].mean(axis=1) for k in (1, 2)])
    assert abs(res["val_corr_dvar_dmpjpe"] - stats.pearsonr(dv, de)[0]) <= 1e-3


CLI_KEYS = ("corrupt_levels", "corrupt_summary", "val_corr_dvar_dmpjpe", "val_spearman_dvar_dmpjpe") + tuple(
    f"{m}_l{k}" for k in range(3) for m in ("mpjpe", "pampjpe", "v2v", "var"))


def test_cli_prints_the_labelled_lines_writes_the_keys_and_refuses(setup, runs, capsys):
    tmp, _, _ = setup
    spec = importlib.util.spec_from_file_location("poco_eval_cli_corrupt_gpu", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    common = ["--cfg", CFG, "--ckpt", str(tmp / "ckpt.pt"), "--smpl", str(tmp / "smpl.npz"), "--j_regressor", str(tmp / "J.npy"),
              "--dataset", str(tmp / "ds.npz"), "--img_dir", str(tmp / "imgs"), "--batch_size", "24", "--crop", "dataset"]
    flag = ["--corrupt", LEVELS, "--corrupt_seed", str(SEED)]
    res = cli.main(cli.parse_args(common + ["--output_folder", str(tmp / "e_c"), "--bootstrap", "50", "--save_results"] + flag))
    text = capsys.readouterr().out
    for line in ("Corruption levels: clean,gaussian_blur:2,jpeg:20+gaussian_noise:8", "Level 0 (clean) MPJPE: ", "Level 1 (gaussian_blur:2) PA-MPJPE: ",
                 "Level 2 (jpeg:20+gaussian_noise:8) V2V (mm): ", "Level 1 (gaussian_blur:2) var mean / median: ", "Level 2 (jpeg:20+gaussian_noise:8) - clean: MPJPE ",
                 "N: 8", "Corr(delta var, delta MPJPE) over crops x levels: Pearson "):
        assert line in text, line
    assert np.abs(res["mpjpe_l2"] - runs["corrupt"]["mpjpe_l2"]).max() <= GATE
    with np.load(tmp / "e_c" / "evaluation_results_3dpw.npz") as z:
        for k in CLI_KEYS + ("mpjpe", "val_mpjpe", "N", "boot_names", "boot_summary", "pred_jnts3D"):
            assert k in z.files, k
        assert z["corrupt_summary"].shape == (3, 10) and z["var_l1"].shape == (8,) and z["mpjpe_l1"].shape[0] == 8
        assert any("Level 2" in str(n) for n in z["boot_names"])
    # without the flag the file has none of the new keys
    cli.main(cli.parse_args(common + ["--output_folder", str(tmp / "e_plain")]))
    capsys.readouterr()
    with np.load(tmp / "e_plain" / "evaluation_results_3dpw.npz") as z:
        assert not [k for k in z.files if k.startswith("corrupt_") or "_l0" in k or "dvar" in k]
    # every refusal, before an engine is built
    for extra, word in ((["--tta", "flip"], "--tta"), (["--cfg2", CFG, "--ckpt2", str(tmp / "ckpt.pt")], "--cfg2"), (["--segm"], "--segm"),
                        (["--likelihood"], "--likelihood"), (["--sequences"], "--sequences"), (["--visibility"], "--visibility"),
                        (["--kp_refit", "1.0"], "--kp_refit"), (["--calibrate", str(tmp / "c.npz")], "--calibrate"), (["--rank_metrics"], "--rank_metrics")):
        with pytest.raises(SystemExit) as e:
            cli.main(cli.parse_args(common + flag + extra))
        assert word in str(e.value) and "--corrupt" in str(e.value), extra
    with pytest.raises(SystemExit, match="--crop dataset"):
        cli.main(cli.parse_args(common[:-2] + flag))
    with pytest.raises(SystemExit, match="--corrupt"):
        cli.main(cli.parse_args(common + ["--corrupt_seed", "3"]))
