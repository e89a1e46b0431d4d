"""GPU: eval.py --sequences end to end (resnet50-cliff, synthetic weights, 54 synthetic crops: three tracks of 5, 9 and 40 frames
written to the dataset file interleaved and out of frame order).

evaluate.run_eval_sequences returns under run_eval's keys bit for bit what run_eval returns; seq_accel / seq_accel_err equal the
plain-loop restatement tests/accel_np.py on the returned pred_jnts3D / gt_jnts3D, grouped by the test's own knowledge of the tracks;
the pipeline infill:<above every var> touches nothing and scores exactly the raw numbers; the pipeline infill:<median var> scores per
crop what a fresh Evaluator gives when fed the output of the existing infill.infill_tracks on the same tracks; a smoother moves every
row and lowers the jitter of the synthetic network's frame-to-frame noise; the .npz of the command line holds the new keys."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import evaluate, infill, ops, postproc, sequences, synth
from tests import accel_np, util

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LENGTHS = (5, 9, 40)
FOLDERS = ("courtyard_00", "downtown_01", "courtyard_00")               # the third track is a second person of the first folder
N = sum(LENGTHS)
BATCH = 16
U = 2.0 ** -52


def _layout():
    """(track, frame id) of every file row: the three tracks interleaved by a seeded shuffle, so no track is in frame order.
    Track 2 shares folder and frame numbers with track 0 and is told apart by person_id."""
    rows = [(k, 100 * k + 3 + t if k == 1 else 7 + t) for k, T in enumerate(LENGTHS) for t in range(T)]
    perm = np.random.default_rng(2929).permutation(len(rows))
    return [rows[i] for i in perm]


@pytest.fixture(scope="module")
def setup(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("eval_seq")
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "ckpt.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    np.save(tmp / "J.npy", synth.synth_j_regressor_h36m(11))
    r = np.random.default_rng(29)
    rows = _layout()
    ds = dict(imgname=np.array([f"imageFiles/{FOLDERS[k]}/image_{f:05d}.jpg" for k, f in rows]),
              person_id=np.array([0 if k < 2 else 1 for k, _ in rows], np.int32),
              center=r.uniform(80, 200, (N, 2)).astype(np.float32), scale=r.uniform(0.5, 1.0, N).astype(np.float32),
              pose=(0.4 * r.standard_normal((N, 72))).astype(np.float32), shape=(0.5 * r.standard_normal((N, 10))).astype(np.float32),
              # crops of very different contrast: the synthetic network's uncertainty then varies from frame to frame, and a
              # threshold at its median leaves every joint with confident and doubtful frames
              img=(r.uniform(0.2, 4.0, (N, 1, 1, 1)) * r.standard_normal((N, 3, 224, 224))).astype(np.float32), orig_shape=np.tile([[240.0, 320.0]], (N, 1)).astype(np.float32))
    np.savez(tmp / "ds.npz", **ds)
    model = util.make_engine("resnet50-cliff", max_batch=BATCH, weights=w)
    # the test's own grouping: track-major rows, each track in frame order, tracks by their first row in the file
    first = {k: min(i for i, (kk, _) in enumerate(rows) if kk == k) for k in range(3)}
    tracks = sorted(range(3), key=first.get)
    order = np.array([i for k in tracks for i in sorted((i for i, (kk, _) in enumerate(rows) if kk == k), key=lambda i: rows[i][1])])
    frames = np.array([rows[i][1] for i in order], np.int32)
    offsets = np.concatenate([[0], np.cumsum([LENGTHS[k] for k in tracks])]).astype(np.int32)
    return dict(tmp=tmp, model=model, ds=ds, tracks=tracks, order=order, frames=frames, offsets=offsets, J=synth.synth_j_regressor_h36m(11))


@pytest.fixture(scope="module")
def raw_outputs(setup, cuda):
    """The model's own outputs for every crop, on the host, from the loop run_eval runs; and the median processed uncertainty."""
    model = setup["model"]
    data = evaluate.EvalDataset(str(setup["tmp"] / "ds.npz"))
    out = {k: [] for k in ("pred_pose", "pred_shape", "var_pose", "smpl_vertices", "smpl_joints3d")}
    for lo in range(0, N, BATCH):
        o = model(data.batch(lo, min(lo + BATCH, N), cuda), want_segm=False)
        for k in out:
            out[k].append(o[k].cpu().numpy())
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["var"] = postproc.prepare_uncert(out["var_pose"], True)
    return out


@pytest.fixture(scope="module")
def runs(setup, raw_outputs, cuda):
    var = raw_outputs["var"]
    above, median = float(np.nextafter(np.float32(var.max()), np.float32(np.inf))) * 2.0, float(np.median(var))
    pipes = sequences.parse_pipelines(f"infill:{above!r},infill:{median!r},smooth_uncert:10+smooth")
    data = lambda: evaluate.EvalDataset(str(setup["tmp"] / "ds.npz"))           # noqa: E731
    plain = evaluate.run_eval(setup["model"], data(), setup["J"], batch_size=BATCH, save_results=True, return_records=True)
    seq = evaluate.run_eval_sequences(setup["model"], data(), setup["J"], batch_size=BATCH, save_results=True, return_records=True,
                                      pipelines=pipes)
    return dict(plain=plain, seq=seq, median=median, above=above)


def test_the_usual_results_are_run_evals_bit_for_bit(runs):
    plain, seq = runs["plain"], runs["seq"]
    assert set(plain) <= set(seq)
    for k, v in plain.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == seq[k].dtype and np.array_equal(v.view(np.uint8) if v.dtype.kind == "f" else v, seq[k].view(np.uint8) if v.dtype.kind == "f" else seq[k]), k
        else:
            assert v == seq[k] or (v != v and seq[k] != seq[k]), k


def test_grouping_and_accel_equal_the_restatement_on_the_returned_joints(setup, runs):
    seq, order, frames, offsets = runs["seq"], setup["order"], setup["frames"], setup["offsets"]
    rows = _layout()
    assert list(seq["seq_track_names"]) == [f"imageFiles/{FOLDERS[k]}#{0 if k < 2 else 1}" for k in setup["tracks"]]
    assert np.array_equal(seq["seq_frame"], [f for _, f in rows])
    tr = np.empty(N, np.int64)
    tr[order] = np.repeat(np.arange(3), np.diff(offsets))
    assert np.array_equal(seq["seq_track"], tr)
    want = accel_np.track_accel(seq["pred_jnts3D"][order], seq["gt_jnts3D"][order], frames, offsets)
    assert want["valid"].sum() == N - 6                                           # every track: all but its first and last row
    worst = 0
    for key, ref in (("seq_accel", "accel64"), ("seq_accel_err", "accel_err64")):
        got = seq[key][order]
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), ~want["valid"]), key
        worst = max(worst, int(accel_np.ulp_distance(got, want[ref])[want["valid"]].max()))
    assert worst <= 1, worst
    M = seq["pred_jnts3D"].shape[1]
    for c in range(3):
        assert (np.abs(seq["seq_track_sums"][:, c] - want["track_sums"][:, c]) <= (np.diff(offsets) + M + 4) * U * want["abs_track"][:, c]).all()
        assert abs(seq["seq_total"][c] - want["total"][c]) <= (N + M + 4) * U * want["abs_total"][c]
    s = seq["seq_summary"]
    assert s.shape == (4, len(sequences.SUMMARY_FIELDS)) and list(seq["seq_pipelines"]) == [sequences.pipeline_text(p) for p in sequences.parse_pipelines(
        f"infill:{runs['above']!r},infill:{runs['median']!r},smooth_uncert:10+smooth")]
    assert s[0, 0] == seq["val_mpjpe"] and s[0, 1] == seq["val_pampjpe"] and s[0, 2] == seq["val_v2v"] and s[0, 5] == 0.0
    assert s[0, 3] == 1000.0 * seq["seq_total"][1] / seq["seq_total"][2] and s[0, 4] == 1000.0 * seq["seq_total"][0] / seq["seq_total"][2]
    assert s[0, 6] == (N - 6) / N
    print(f"rows within {worst} ulp; Accel {s[0, 3]:.3f}, Accel error {s[0, 4]:.3f} mm / frame^2 over {int(seq['seq_total'][2])} rows")


def test_an_infill_above_every_uncertainty_touches_nothing_and_scores_the_raw_numbers(runs):
    seq = runs["seq"]
    post = seq["seq_post"][0]
    assert np.array_equal(seq["seq_summary"][1, :5], seq["seq_summary"][0, :5]) and seq["seq_summary"][1, 5] == 0.0
    for k in ("mpjpe", "pampjpe", "v2v", "pred_jnts3D", "seq_accel", "seq_accel_err"):
        assert np.array_equal(post[k].view(np.uint32), seq[k].view(np.uint32)), k
    assert post["val_mpjpe"] == seq["val_mpjpe"] and post["val_pampjpe"] == seq["val_pampjpe"] and post["val_v2v"] == seq["val_v2v"]


def _existing_path(setup, raw, thresh, cuda):
    """infill.infill_tracks on the raw outputs of the same tracks, scored by a fresh Evaluator in track-major order -> per-crop
    mpjpe / pampjpe [N,14] in file order."""
    model, order, offsets, ds = setup["model"], setup["order"], setup["offsets"], setup["ds"]
    tracks = {}
    for p in range(3):
        idx = order[offsets[p]:offsets[p + 1]]
        tracks[p] = dict(pose=raw["pred_pose"][idx], betas=raw["pred_shape"][idx], orig_cam=np.zeros((len(idx), 4), np.float32),
                         var=raw["var"][idx], frame_ids=setup["frames"][offsets[p]:offsets[p + 1]], verts=raw["smpl_vertices"][idx],
                         smpl_joints3d=raw["smpl_joints3d"][idx])
    filled = infill.infill_tracks(model, tracks, thresh, 30)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)   # noqa: E731
    ev = evaluate.Evaluator(setup["J"], evaluate.joint_map("3dpw"), capacity=N, device=cuda)
    verts, pose = np.concatenate([filled[p]["verts"] for p in range(3)]), np.concatenate([filled[p]["pose"] for p in range(3)])
    for lo in range(0, N, BATCH):                                                  # track-major rows, at most max_batch at a time
        idx = order[lo:lo + BATCH]
        gt_pose = t(ds["pose"][idx])
        gt_verts, _ = model.smpl_lbs(t(ds["shape"][idx]), ops.rodrigues(gt_pose))
        ev.step({"smpl_vertices": t(verts[lo:lo + BATCH]), "pred_pose": t(pose[lo:lo + BATCH]), "var_pose": t(raw["var_pose"][idx])}, gt_pose,
                gt_vertices=gt_verts)
    res = ev.finish()
    ev.close()
    out = {}
    for k in ("mpjpe", "pampjpe"):
        out[k] = np.empty_like(res[k])
        out[k][order] = res[k]
    out["touched"] = sum(f["counts"]["touched_frames"] for f in filled.values())
    out["changed"] = sum(f["counts"]["interpolated"] + f["counts"]["held"] for f in filled.values())
    return out


def test_the_median_infill_scores_what_the_existing_infill_path_scores(setup, raw_outputs, runs, cuda):
    """Measured on an MI355X: two runs of the existing path (infill.infill_tracks, then a fresh Evaluator) differ by 0.0 m in both
    per-crop errors; the tolerance is that figure plus one rounding of the fp32 records, 2^-24 of the largest value."""
    a = _existing_path(setup, raw_outputs, runs["median"], cuda)
    b = _existing_path(setup, raw_outputs, runs["median"], cuda)
    post = runs["seq"]["seq_post"][1]
    doubtful = raw_outputs["var"] > np.float32(runs["median"])
    print(f"doubtful entries per joint at the median {runs['median']:.4f}: {doubtful.sum(0).tolist()} of {N}")
    assert 0 < a["touched"] <= N and a["touched"] == b["touched"]
    for k in ("mpjpe", "pampjpe"):
        d_ref = float(np.abs(a[k] - b[k]).max())
        tol = d_ref + 2.0 ** -24 * float(np.abs(a[k]).max())
        dev = float(np.abs(post[k] - a[k]).max())
        print(f"infill:{runs['median']:.4f} {k}: deviation {dev:.3e} m from the existing path (two runs of which differ by {d_ref:.3e}; "
              f"tolerance {tol:.3e}); {a['touched']} of {N} frames re-posed")
        assert dev <= tol, (k, dev, tol)
        assert np.abs(post[k] - runs["seq"][k]).max() > 1e-4                      # and the in-fill did move the error
    changed = runs["seq"]["seq_summary"][2, 5]
    assert 0.0 < changed <= a["changed"] / (N * 24)                               # an entry held at an identical matrix counts as unchanged


def test_a_smoother_moves_every_row_and_lowers_the_jitter(runs):
    s = runs["seq"]["seq_summary"]
    assert np.isfinite(s).all() and s[3, 5] == 1.0 and s[3, 6] == s[0, 6]
    assert s[3, 3] < s[0, 3]                                                       # the synthetic network's frame-to-frame noise is smoothed
    assert not np.array_equal(runs["seq"]["seq_post"][2]["mpjpe"], runs["seq"]["mpjpe"])


def test_cli_prints_the_lines_and_the_npz_holds_the_new_keys(setup, runs, capsys, cuda):
    spec = importlib.util.spec_from_file_location("poco_eval_cli", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    tmp = setup["tmp"]
    argv = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "ckpt.pt"), "--smpl", str(tmp / "smpl.npz"),
            "--j_regressor", str(tmp / "J.npy"), "--dataset", str(tmp / "ds.npz"), "--batch_size", str(BATCH), "--output_folder",
            str(tmp / "out"), "--sequences", "--seq_post", f"infill:{runs['median']!r}"]
    res = cli.main(cli.parse_args(argv))
    printed = capsys.readouterr().out.splitlines()
    assert printed[-9:-4] == evaluate.report_lines(res) and printed[-4:] == evaluate.sequence_lines(res)
    assert printed[-4].startswith("Accel: ") and printed[-3].startswith("Accel error: ") and printed[-2].startswith("Tracks: 3 ")
    assert printed[-1].startswith("Post infill:") and "MPJPE" in printed[-1] and "Accel error" in printed[-1] and "changed" in printed[-1]
    seq = runs["seq"]
    z = np.load(tmp / "out" / "evaluation_results_3dpw.npz")
    for k in evaluate.SEQ_NPZ_KEYS:
        assert k in z.files, k
    for k in ("seq_track", "seq_frame", "seq_accel", "seq_accel_err"):
        assert z[k].shape == (N,) and np.array_equal(z[k].view(np.uint32), seq[k].view(np.uint32)), k
    assert list(z["seq_track_names"]) == list(seq["seq_track_names"]) and list(z["seq_pipelines"]) == [sequences.pipeline_text([("infill", runs["median"])])]
    assert z["seq_summary"].shape == (2, len(sequences.SUMMARY_FIELDS))
    assert np.array_equal(z["seq_summary"][0], seq["seq_summary"][0]) and np.array_equal(z["seq_summary"][1], seq["seq_summary"][2])
    assert float(z["val_mpjpe"]) == seq["val_mpjpe"]
