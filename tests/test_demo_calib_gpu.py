"""GPU: demo.py --calibration FILE in folder and video mode on the smallest variant (resnet50-cliff, synthetic weights and body model as
in tests/test_demo_sort_gpu.py): the four new arrays are the plain-loop map of tests/calib_np.py on the saved `var`, the crop key is
bitwise the evaluator's, a file fitted for another head or kinematic flag is refused before anything is written, and the output
without the flag is what it was."""
import numpy as np
import pytest
import torch

from poco_amd import calibrate, synth
from tests import calib_np, util

pytestmark = pytest.mark.gpu
T, H, W = 6, 96, 128


def calib_file(path, head="cliff", kinematic=True):
    """28 hand-made maps over the range the uncertainties take: map m has 3 + m % 5 blocks (joint_7: none), single keys and ranges."""
    r = np.random.default_rng(2)
    tabs = []
    for m in range(28):
        B = 0 if m == 4 + 7 else 3 + m % 5
        lo = np.cumsum(r.uniform(0.02, 0.3, B)).astype(np.float32).astype(np.float64)
        hi = (lo + (np.arange(B) % 2) * 0.01).astype(np.float32).astype(np.float64)
        tabs.append(np.stack([lo, hi, np.cumsum(r.uniform(0.01, 0.1, B)), 1.0 + np.arange(B)], axis=1).reshape(B, 4))
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tabs])]).astype(np.int32)
    meta = calibrate.make_meta("3dpw", kinematic, "resnet50-" + head)
    res = {"calib_names": np.asarray(calibrate.MAP_NAMES), "calib_offsets": offs, "calib_knots": np.concatenate(tabs),
           "calib_rows": np.full(28, 10, np.int64), "calib_dropped": np.zeros(28, np.int64), "calib_summary": np.full((28, 3), np.nan),
           "calib_meta": np.asarray([f"{k}={v}" for k, v in meta.items()])}
    calibrate.save(str(path), res)
    return res


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("demo_calib")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    fr = tmp / "frames"
    fr.mkdir()
    r = np.random.default_rng(9)
    for i in range(T):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(fr / f"{i:06d}.png")
    table = calib_file(tmp / "calib.npz")
    calib_file(tmp / "other_head.npz", head="pare")
    calib_file(tmp / "other_kin.npz", kinematic=False)
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--batch_size", "8",
              "--smpl", str(tmp / "smpl.npz"), "--no_render"]

    def run(name, mode, flags):
        import demo
        src = ["--mode", "video", "--vid_file", str(fr)] if mode == "video" else ["--mode", "folder", "--image_folder", str(fr)]
        demo.main(demo.parse_args(common + src + ["--output_folder", str(tmp / name), *flags]))
        out = tmp / name / "frames_"
        if mode == "video":
            return dict(np.load(out / "poco_results.npz"))
        return {f"{i}/{k}": v for i in range(T) for k, v in np.load(out / f"{i:06d}_poco.npz").items()}
    run.tmp, run.table = tmp, table
    return run


def check_errors(res, prefix, table):
    var = res[f"{prefix}/var"]
    n = len(var)
    key = calibrate.crop_key(var)
    m = np.zeros(n, np.float64)                                           # the evaluator's rule, restated: joint order, float64, one rounding
    for j in range(24):
        m = m + var[:, j].astype(np.float64)
    assert np.array_equal(key.view(np.uint32), (m / 24.0).astype(np.float32).view(np.uint32))
    dev_key = calibrate.crop_key(torch.from_numpy(var).cuda()).cpu().numpy()
    assert np.array_equal(dev_key.view(np.uint32), key.view(np.uint32))
    x = np.concatenate([var, key[:, None], key[:, None], key[:, None]], axis=1)
    want = calib_np.calib_apply(x, calibrate.DEMO_MAP_IDS, table["calib_offsets"], table["calib_knots"])
    got = np.concatenate([res[f"{prefix}/err_pose"], res[f"{prefix}/err_mpjpe"][:, None], res[f"{prefix}/err_pampjpe"][:, None],
                          res[f"{prefix}/err_v2v"][:, None]], axis=1)
    assert got.dtype == np.float32 and got.shape == (n, 27)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[:, 7]).all() and not np.isnan(np.delete(got, 7, axis=1)).any()
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok].astype(np.float64) - want[ok]) <= np.spacing(np.abs(want[ok])))


NEW = ("err_pose", "err_mpjpe", "err_pampjpe", "err_v2v")


@pytest.mark.parametrize("mode", ["folder", "video"])
def test_the_demo_gains_error_bars(case, mode):
    plain = case(f"plain_{mode}", mode, [])
    cal = case(f"cal_{mode}", mode, ["--calibration", str(case.tmp / "calib.npz")])
    assert not any(k.split("/")[1] in NEW for k in plain)
    assert {k for k in cal if k.split("/")[1] not in NEW} == set(plain)
    for k, v in plain.items():                                            # without the flag nothing changes
        assert np.array_equal(v, cal[k], equal_nan=v.dtype.kind == "f"), k
    for prefix in sorted({k.split("/")[0] for k in cal}):
        check_errors(cal, prefix, case.table)
    if mode == "video":
        post = case("cal_video_post", mode, ["--calibration", str(case.tmp / "calib.npz"), "--infill", "0.3", "--smooth_uncert", "10"])
        check_errors(post, "0", case.table)                               # after the post-processing, on the final var


def test_a_mismatching_file_is_refused_before_anything_is_written(case):
    for name, word in (("other_head.npz", "head"), ("other_kin.npz", "kinematic")):
        with pytest.raises(SystemExit, match=word):
            case("refused", "folder", ["--calibration", str(case.tmp / name)])
    with pytest.raises(SystemExit, match="--calibration"):
        case("refused", "video", ["--calibration", str(case.tmp / "missing.npz")])
    with pytest.raises(SystemExit, match="kinematic"):
        case("refused", "video", ["--calibration", str(case.tmp / "calib.npz"), "--no_kinematic_uncert"])
    assert not (case.tmp / "refused").exists()
