"""GPU: demo.py --mode video --kp_refit end to end on the smallest variant (resnet50-cliff, synthetic weights and body model as in
tests/test_demo_usmooth_gpu.py): a clip of 32 noise frames of 96 x 128 with two keypoint tracks (boxes and BODY_25 joints2d), one of 32
rows and one of 26.  The keypoints are seeded points inside the box with confidences either side of --kp_vis_thresh; frame 4 of
track 0 keeps two of them (under the four a fit needs).

The refitted file is checked against refit.refit_tracks applied to the file's own pose_net / betas_net / orig_cam_net / var (the same
operator on the same rows: the same bits), its meshes against the LBS operator, and everything the refit must not touch against the
run without the flag; the chain with --infill and --smooth_uncert against those two operators applied to the refit-only file; eval.py
--kp_refit on a pseudo-GT file written by demo.py --save_dataset in the test."""
import json

import numpy as np
import pytest
import torch

from poco_amd import refit, synth
from tests import util

pytestmark = pytest.mark.gpu
T, H, W = 32, 96, 128
LAM = 0.1
NEW_KEYS = ("refit_shift", "refit_cost", "refit_flag", "pose_net", "betas_net", "orig_cam_net")
LBS_TOL = 2e-5                # tests/test_model_gpu.py::test_smpl_lbs_op: the LBS operator against its float64 restatement


@pytest.fixture(scope="module")
def case(tmp_path_factory, cuda):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("refit")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    fr = tmp / "frames"
    fr.mkdir()
    r = np.random.default_rng(4)
    for i in range(T):
        Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(fr / f"{i:06d}.png")
    f0, f1 = np.arange(T), np.arange(3, 29)
    box = lambda cx, f: np.stack([cx + 0.25 * f, 48 + 0.1 * f, 60 + 0 * f, 60 + 0 * f], 1)        # noqa: E731

    def keypoints(b):
        xy = b[:, None, :2] + r.uniform(-25, 25, (len(b), 25, 2))
        conf = r.uniform(0.35, 1.0, (len(b), 25, 1))
        conf[r.random(conf.shape) < 0.2] = 0.1
        return np.concatenate([xy, conf], 2)
    k0, k1 = keypoints(box(36.0, f0)), keypoints(box(80.0, f1))
    k0[4, :, 2] = 0.0
    k0[4, [1, 8], 2] = 0.9
    tracks = {"0": {"bbox": box(36.0, f0).tolist(), "frames": f0.tolist(), "joints2d": k0.tolist()},
              "1": {"bbox": box(80.0, f1).tolist(), "frames": f1.tolist(), "joints2d": k1.tolist()}}
    (tmp / "tracks.json").write_text(json.dumps(tracks))
    (tmp / "boxes.json").write_text(json.dumps({k: {"bbox": v["bbox"], "frames": v["frames"]} for k, v in tracks.items()}))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video", "--vid_file", str(fr),
              "--batch_size", "32", "--smpl", str(tmp / "smpl.npz"), "--no_render"]

    def run(name, flags=(), tracking="tracks.json"):
        import demo
        demo.main(demo.parse_args(common + ["--tracking", str(tmp / tracking), "--output_folder", str(tmp / name), *flags]))
        return dict(np.load(tmp / name / "frames_" / "poco_results.npz"))
    run.smpl, run.ckpt, run.frames = str(tmp / "smpl.npz"), str(tmp / "poco_synth.pt"), str(fr)
    return run


@pytest.fixture(scope="module")
def plain(case):
    return case("plain")


@pytest.fixture(scope="module")
def u_ref(plain):
    return float(np.median(np.concatenate([plain["0/var"].ravel(), plain["1/var"].ravel()])))


@pytest.fixture(scope="module")
def refitted(case, u_ref):
    return case("refit", ["--kp_refit", repr(LAM), "--kp_refit_ref", repr(u_ref)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_run_without_the_flag_has_none_of_the_new_keys(plain):
    assert {k.split("/")[0] for k in plain} == {"0", "1"} and not any(k.split("/")[1] in NEW_KEYS for k in plain)
    assert plain["0/pose"].shape == (T, 24, 3, 3) and plain["1/pose"].shape == (26, 24, 3, 3) and plain["0/joints2d"].shape == (T, 25, 3)


def test_refitted_file_is_refit_tracks_on_its_own_net_values(case, plain, refitted, u_ref, cuda):
    model = util.make_engine("resnet50-cliff", max_batch=T)
    tables = refit.joint_tables(case.smpl)
    tracks = {}
    for pid in ("0", "1"):
        g = lambda k: refitted[f"{pid}/{k}"]                                     # noqa: E731
        for k in NEW_KEYS:
            assert f"{pid}/{k}" in refitted, k
        n = len(g("frame_ids"))
        assert g("refit_shift").shape == (n, 24) and g("refit_cost").shape == (n, 2) and g("refit_flag").shape == (n,)
        # what the refit starts from is the raw prediction, and what it must not touch stays raw
        for net, raw in (("pose_net", "pose"), ("betas_net", "betas"), ("orig_cam_net", "orig_cam")):
            assert np.array_equal(_bits(g(net)), _bits(plain[f"{pid}/{raw}"])), net
        for k in ("var", "var_global", "pred_cam", "smpl_joints2d", "bboxes", "frame_ids", "betas", "joints2d"):
            assert np.array_equal(g(k), plain[f"{pid}/{k}"]), k
        tracks[pid] = {"pose": g("pose_net"), "betas": g("betas_net"), "orig_cam": g("orig_cam_net"), "var": g("var"), "joints2d": g("joints2d"),
                       "bboxes": g("bboxes"), "frame_ids": g("frame_ids"), "verts": plain[f"{pid}/verts"],
                       "smpl_joints3d": plain[f"{pid}/smpl_joints3d"]}
    again = refit.refit_tracks(model, tracks, LAM, u_ref, 0.1, 0.3, 10, tables=tables, img_w=W, img_h=H)
    for pid in ("0", "1"):
        g = lambda k: refitted[f"{pid}/{k}"]                                     # noqa: E731
        for k in ("pose", "orig_cam", "refit_shift", "refit_cost", "refit_flag"):
            assert np.array_equal(_bits(g(k)), _bits(again[pid][k])), k
        flag, cost = g("refit_flag"), g("refit_cost")
        assert (cost[:, 1] <= cost[:, 0]).all() and (cost[flag == 0, 1] < cost[flag == 0, 0]).all()
        assert g("refit_shift")[flag == 0].max() > 0.0                             # it did move
        # every fitted frame re-posed from the refitted pose and the kept shape; the others keep their mesh bit for bit
        v, j = model.smpl_lbs(torch.from_numpy(g("betas")).to(cuda), torch.from_numpy(g("pose")).to(cuda))
        assert np.abs(g("verts") - v.cpu().numpy()).max() <= LBS_TOL and np.abs(g("smpl_joints3d") - j.cpu().numpy()).max() <= LBS_TOL
        for k, raw in (("pose", "pose"), ("orig_cam", "orig_cam"), ("verts", "verts")):
            assert np.array_equal(_bits(g(k)[flag != 0]), _bits(plain[f"{pid}/{raw}"][flag != 0])), k
    assert refitted["0/refit_flag"][4] == 1 and (np.delete(refitted["0/refit_flag"], 4) == 0).all() and (refitted["1/refit_flag"] == 0).all()
    line = refit.summary_line(again, tracks, tables, W, H)
    print(line)
    assert line.startswith("kp_refit: reprojection error ")
    e0, e1 = (float(x) for x in line.split("reprojection error ")[1].split(" of the box")[0].split(" -> "))
    assert e1 < e0


def test_infill_and_the_smoother_take_what_the_refit_left(case, plain, refitted, u_ref, cuda):
    """--kp_refit --infill --smooth_uncert = infill.infill_tracks, then usmooth.smooth_tracks, applied here to the refit-only file's
    pose / betas / orig_cam / meshes with the raw var: the same operators on the same rows, so the same bits.  A chain that
    started from pose_net, or ran its stages in another order, gives other bits."""
    from poco_amd import infill, usmooth
    thr = float(np.median(np.concatenate([plain["0/var"][:, 0], plain["1/var"][:, 0]])))
    both = case("chain", ["--kp_refit", repr(LAM), "--kp_refit_ref", repr(u_ref), "--infill", repr(thr), "--infill_max_gap", "8",
                          "--smooth_uncert", "10.0", "--smooth_uncert_ref", repr(u_ref)])
    model = util.make_engine("resnet50-cliff", max_batch=T)
    keys = ("pose", "betas", "orig_cam", "var", "frame_ids", "verts", "smpl_joints3d")
    tracks = {pid: {k: refitted[f"{pid}/{k}"] for k in keys} for pid in ("0", "1")}
    filled = infill.infill_tracks(model, tracks, thr, 8)
    assert sum(int((filled[pid]["infill"] != 0).sum()) for pid in filled) > 0          # the in-fill did touch something
    for pid in tracks:
        tracks[pid] = {**tracks[pid], **{k: filled[pid][k] for k in ("pose", "betas", "orig_cam", "verts", "smpl_joints3d")}}
    want = usmooth.smooth_tracks(model, tracks, 10.0, u_ref, 30)
    from_net = usmooth.smooth_tracks(model, {pid: {**tracks[pid], "pose": refitted[f"{pid}/pose_net"]} for pid in tracks}, 10.0, u_ref, 30)
    for pid in ("0", "1"):
        for k in NEW_KEYS + ("infill", "smooth_shift"):
            assert f"{pid}/{k}" in both, k
        for k in ("pose_net", "betas_net", "orig_cam_net", "var", "refit_shift", "refit_cost", "refit_flag"):   # the network's values; the refit's record
            assert np.array_equal(_bits(both[f"{pid}/{k}"]), _bits(refitted[f"{pid}/{k}"])), k
        assert np.array_equal(both[f"{pid}/infill"], filled[pid]["infill"])
        for k in ("pose", "betas", "orig_cam", "smooth_shift"):
            assert np.array_equal(_bits(both[f"{pid}/{k}"]), _bits(want[pid][k])), k
        assert not np.array_equal(_bits(both[f"{pid}/pose"]), _bits(from_net[pid]["pose"]))     # ... and the check can tell the difference


def test_eval_scores_raw_and_refit_side_by_side(case, tmp_path, capsys, cuda):
    """eval.py --kp_refit on a pseudo-GT file that demo.py --save_dataset writes in this test (it carries `openpose`): the line pair
    is printed, the .npz has the new keys, the raw half is what eval.py prints without the flag, and a file without `openpose` is
    refused in one sentence."""
    import importlib.util
    from pathlib import Path
    from poco_amd import evaluate
    spec = importlib.util.spec_from_file_location("poco_eval_cli", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    case("pseudo", ["--save_dataset", str(tmp_path / "pseudo.npz")])
    z = dict(np.load(tmp_path / "pseudo.npz"))
    n = len(z["imgname"])
    assert z["openpose"].shape == (n, 25, 3) and n == T + 26
    np.save(tmp_path / "J.npy", synth.synth_j_regressor_h36m(11))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", case.ckpt, "--smpl", case.smpl, "--j_regressor", str(tmp_path / "J.npy"),
              "--img_dir", case.frames, "--batch_size", "32"]
    capsys.readouterr()
    raw = cli.main(cli.parse_args(common + ["--dataset", str(tmp_path / "pseudo.npz"), "--output_folder", str(tmp_path / "raw")]))
    capsys.readouterr()
    res = cli.main(cli.parse_args(common + ["--dataset", str(tmp_path / "pseudo.npz"), "--output_folder", str(tmp_path / "fit"), "--kp_refit", repr(LAM)]))
    printed = capsys.readouterr().out.splitlines()
    lines = evaluate.refit_report_lines(res)
    assert printed[-len(lines):] == lines
    assert lines[0].startswith("Raw MPJPE: ") and lines[4].startswith("Refit MPJPE: ") and lines[-2].startswith("Refit - raw: MPJPE ")
    assert lines[-1].startswith("Refit shift: mean ")
    out = dict(np.load(tmp_path / "fit" / "evaluation_results_3dpw.npz"))
    for k, shape in (("mpjpe_raw", (n, 14)), ("pampjpe_raw", (n, 14)), ("v2v_raw", (n,)), ("mpjpe", (n, 14)), ("refit_shift", (n, 24)),
                     ("refit_cost", (n, 2)), ("refit_flag", (n,)), ("val_mpjpe_raw", ()), ("val_pampjpe_raw", ()), ("val_v2v_raw", ()),
                     ("val_corr_raw", ())):
        assert k in out and out[k].shape == shape, k
    # the raw half is the run without the flag, bit for bit; the refit moved something and every fitted row's cost fell
    for k in ("mpjpe", "pampjpe", "v2v"):
        assert np.array_equal(_bits(res[k + "_raw"]), _bits(raw[k])), k
    assert res["val_mpjpe_raw"] == raw["val_mpjpe"]
    fit = res["refit_flag"] == 0
    assert fit.sum() > n // 2 and (res["refit_cost"][fit, 1] < res["refit_cost"][fit, 0]).all() and res["refit_shift"][fit].max() > 0.0
    assert not np.array_equal(res["mpjpe"][fit], raw["mpjpe"][fit]) and np.array_equal(_bits(res["mpjpe"][~fit]), _bits(raw["mpjpe"][~fit]))
    np.savez(tmp_path / "bare.npz", **{k: v for k, v in z.items() if k != "openpose"})
    with pytest.raises(SystemExit) as e:
        cli.main(cli.parse_args(common + ["--dataset", str(tmp_path / "bare.npz"), "--kp_refit", repr(LAM)]))
    assert "--kp_refit" in str(e.value) and "openpose" in str(e.value) and str(e.value).count(". ") == 0
    with pytest.raises(SystemExit) as e:
        cli.main(cli.parse_args(common + ["--dataset", str(tmp_path / "pseudo.npz"), "--kp_refit", repr(LAM), "--rank_metrics"]))
    assert "--kp_refit" in str(e.value) and "--rank_metrics" in str(e.value)


def test_a_box_track_is_refused_in_one_sentence(case):
    with pytest.raises(SystemExit) as e:
        case("boxes", ["--kp_refit", repr(LAM)], tracking="boxes.json")
    msg = str(e.value)
    assert "--kp_refit" in msg and "joints2d" in msg and msg.count(". ") == 0
