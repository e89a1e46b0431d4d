"""GPU: eval.py --cfg2 --ckpt2 end to end with synthetic weights and body model: a dataset that demo.py
--save_dataset wrote from model 1 (three 240 x 320 noise images, two boxes each) and a synthetic [17,6890] joint regressor, scored by
model 1 alone, by model 2 alone (both resnet50-cliff, seeds 0 and 1) and by the pair in crop mode at batch size 4 (a ragged last batch).
--select_scale is the median of the solo runs' score ratio, so both choices occur.  Everything the pair's run adds is a decision plus
copies of what the solo runs compute (the engine is bitwise repeatable), so every comparison is bit for bit; the
printed means are recomputed from the saved file in float64 as evaluate.selection_summary states them."""
import importlib.util
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import synth
from tests import select_np as snp, util

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CFG = "configs/demo_poco_cliff_resnet50.yaml"
NAMES = ["im0.png", "im1.png", "im2.png"]
# square boxes whose side is a multiple of 25: scale = side / 200 and scale * 200 are exact (tests/test_demo_dataset_gpu.py)
DETS = {"im0.png": [[160, 120, 150, 150], [90, 100, 100, 100]], "im1.png": [[200, 110, 125, 125], [120, 130, 175, 175]],
        "im2.png": [[150, 100, 200, 200], [100, 140, 75, 75]]}
N = 6
METRICS = ("mpjpe", "pampjpe", "v2v")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    """(solo model 1, solo model 2, pair): per run eval.py's returned dict, its saved file and its printed lines."""
    from PIL import Image
    import demo
    tmp = tmp_path_factory.mktemp("eval_select")
    for name, seed in (("m1", 0), ("m2", 1)):
        w = util.synth_weights("resnet50-cliff", seed)
        torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / f"{name}.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    np.save(tmp / "J.npy", synth.synth_j_regressor_h36m(11))
    (tmp / "imgs").mkdir()
    r = np.random.default_rng(0)
    for n in NAMES:
        Image.fromarray(r.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(tmp / "imgs" / n)
    (tmp / "dets.json").write_text(json.dumps(DETS))
    demo.main(demo.parse_args(["--cfg", CFG, "--ckpt", str(tmp / "m1.pt"), "--mode", "folder", "--image_folder", str(tmp / "imgs"),
                               "--output_folder", str(tmp / "demo"), "--batch_size", "8", "--smpl", str(tmp / "smpl.npz"), "--detections",
                               str(tmp / "dets.json"), "--no_render", "--save_dataset", str(tmp / "ds.npz")]))
    spec = importlib.util.spec_from_file_location("poco_eval_cli", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)

    def run(name, ckpt, *extra):
        import contextlib
        import io
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = cli.main(cli.parse_args(["--cfg", CFG, "--ckpt", str(tmp / f"{ckpt}.pt"), "--smpl", str(tmp / "smpl.npz"), "--j_regressor",
                                           str(tmp / "J.npy"), "--dataset", str(tmp / "ds.npz"), "--img_dir", str(tmp / "imgs"),
                                           "--batch_size", "4", "--output_folder", str(tmp / name), *extra]))
        return res, dict(np.load(tmp / name / "evaluation_results_3dpw.npz")), buf.getvalue().splitlines()

    s1, s2 = run("solo1", "m1"), run("solo2", "m2")
    # the crop scores of the two solo runs, from the processed uncertainty the evaluator recorded (corr_y, all 24 joints)
    g = [np.array([snp.crop_score(row, 1, 0.40) for row in s[1]["corr_y"].reshape(N, 24)]) for s in (s1, s2)]
    scale = float(np.median(g[0] / g[1]))
    pair = run("pair", "m1", "--cfg2", CFG, "--ckpt2", str(tmp / "m2.pt"), "--select_scale", repr(scale))
    return s1, s2, pair, scale


def test_a_solo_run_has_none_of_the_new_keys(runs):
    f = runs[0][1]
    assert f["mpjpe"].shape == (N, 14) and not any(k.endswith(("_m1", "_m2")) or k.startswith("select") or "oracle" in k for k in f)


def test_per_model_arrays_equal_the_two_solo_runs_bit_for_bit(runs):
    s1, s2, pair, _ = runs
    f = pair[1]
    for tag, solo in (("_m1", s1[1]), ("_m2", s2[1])):
        for k in METRICS:
            assert f[k + tag].dtype == np.float32 and np.array_equal(_bits(f[k + tag]), _bits(solo[k])), k + tag
        for k in ("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr"):
            assert float(f[k + tag]) == float(solo[k]), k + tag


def test_selected_metrics_are_the_chosen_models_rows_bit_for_bit(runs):
    s1, s2, pair, scale = runs
    f = pair[1]
    sel = f["select"]
    assert sel.dtype == np.uint8 and sel.shape == (N, 24) and f["select_score"].shape == (N, 2) and f["select_score"].dtype == np.float32
    choice = sel[:, 0] == 1
    assert choice.any() and not choice.all() and (sel == sel[:, :1]).all()             # both choices occur; crop mode never mixes
    # the choice is the restatement's, on the solo runs' own processed uncertainty (kinematic already applied there)
    z = np.zeros((N, 24, 3, 3), np.float32)
    ref = snp.select(z, s1[1]["corr_y"].reshape(N, 24), 1, z, s2[1]["corr_y"].reshape(N, 24), 1, False, 0.40, scale, 0)
    assert np.array_equal(sel, ref["choice"]) and np.array_equal(_bits(f["select_score"]), _bits(ref["score"]))
    for k in METRICS:
        want = np.where(choice.reshape((-1,) + (1,) * (f[k].ndim - 1)), f[k + "_m2"], f[k + "_m1"])
        assert np.array_equal(_bits(f[k]), _bits(want)), k
    assert int(f["N"]) == N and list(pair[0]["imgname"]) == list(s1[0]["imgname"])


def test_oracle_and_selection_accuracy_equal_their_recomputation_from_the_file(runs):
    s1, s2, pair, _ = runs
    f = pair[1]
    a1, a2 = f["crop_mpjpe_m1"].astype(np.float64), f["crop_mpjpe_m2"].astype(np.float64)
    p1, p2 = f["crop_pampjpe_m1"].astype(np.float64), f["crop_pampjpe_m2"].astype(np.float64)
    oracle = 0.0
    right = 0
    for i in range(N):                                                                 # plain loops, as the restatements are written
        oracle += min(a1[i], a2[i])
        chosen, other = (a2[i], a1[i]) if f["select"][i, 0] else (a1[i], a2[i])
        right += chosen <= other
    # 1000 * sum / N with the sum rounded once (math.fsum); the plain loop's float64 sum of 6 terms is within 6 roundings of it
    assert float(f["val_oracle_mpjpe"]) == 1000.0 * math.fsum(np.minimum(a1, a2)) / N
    assert abs(float(f["val_oracle_mpjpe"]) - 1000.0 * oracle / N) <= 8 * 2.0 ** -53 * float(f["val_oracle_mpjpe"])
    assert float(f["val_oracle_pampjpe"]) == 1000.0 * math.fsum(np.minimum(p1, p2)) / N
    assert float(f["select_accuracy"]) == right / N and float(f["select_share_m2"]) == float((f["select"][:, 0] == 1).mean())
    # the oracle is the bound no selection beats: not above either solo run, nor above the selection
    for k, o in (("val_mpjpe", "val_oracle_mpjpe"), ("val_pampjpe", "val_oracle_pampjpe")):
        assert float(f[o]) <= float(s1[1][k]) and float(f[o]) <= float(s2[1][k]) and float(f[o]) <= float(f[k]), k
    # the per-crop record value is the mean of the crop's per-joint values (one fp32 rounding of a 14-term mean apart at most)
    assert np.abs(a1 - f["mpjpe_m1"].astype(np.float64).mean(1)).max() <= 14 * 2.0 ** -24 * a1.max()


def test_printed_lines_name_the_three_results_and_the_oracle(runs):
    s1, s2, pair, _ = runs
    f, lines = pair[1], pair[2]
    for want in (f"Model 1 MPJPE: {float(s1[1]['val_mpjpe'])}", f"Model 2 MPJPE: {float(s2[1]['val_mpjpe'])}",
                 f"Model 1 PA-MPJPE: {float(s1[1]['val_pampjpe'])}", f"Model 2 V2V (mm): {float(s2[1]['val_v2v'])}",
                 f"Selected (crop) MPJPE: {float(f['val_mpjpe'])}", f"Oracle MPJPE: {float(f['val_oracle_mpjpe'])}",
                 f"Oracle PA-MPJPE: {float(f['val_oracle_pampjpe'])}", f"Selection accuracy: {float(f['select_accuracy'])}",
                 f"Crops from model 2: {float(f['select_share_m2'])}"):
        assert want in lines, want
    assert f"MPJPE: {float(s1[1]['val_mpjpe'])}" in s1[2]                              # a solo run prints the reference's lines unlabelled
