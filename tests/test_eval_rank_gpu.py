"""The evaluator's side of the rank-based metrics on the GPU: poco_evaluator_rank_inputs against the records bit for bit,
ranking.RankMetrics against tests/rank_np.py on those records, and run_eval(rank_metrics=K) beside the plain run."""
import numpy as np
import pytest
import torch

from poco_amd import _lib, evaluate, ranking, synth
from tests import eval_np, rank_np, util

pytestmark = pytest.mark.gpu
U = 2.0 ** -52
V = 431
SEL = [0, 3, 4, 9, 17, 23]


def stepped(cuda, splits, sel=None, seed=9):
    """An Evaluator on a small random mesh (as tests/test_eval_gpu.py builds it) stepped in batches of `splits`."""
    r = np.random.default_rng(seed)
    Jr = np.zeros((5, V), np.float32)
    for j in range(5):
        Jr[j, r.choice(V, 6, replace=False)] = r.dirichlet(np.ones(6)).astype(np.float32)
    ev = evaluate.Evaluator(Jr, [4, 0, 3], capacity=sum(splits), pelvis=2, sel_uncert_part=sel, device=cuda)
    t = lambda a: torch.from_numpy(a).to(cuda)   # noqa: E731
    for B in splits:
        gt = r.uniform(-0.5, 0.5, (B, V, 3)).astype(np.float32)
        pred = (gt + 0.02 * r.standard_normal(gt.shape) * r.uniform(0.2, 3, (B, 1, 1))).astype(np.float32)
        pose = r.uniform(-1, 1, (B, 72)).astype(np.float32)
        pp = eval_np.rodrigues(pose.reshape(-1, 3) + 0.1 * r.standard_normal((B * 24, 3)), np.float64).reshape(B, 24, 3, 3).astype(np.float32)
        var = np.round(r.uniform(0, 1, (B, 24)), 2).astype(np.float32)        # rounded: ties among the per-joint keys
        ev.step({"smpl_vertices": t(pred), "pred_pose": t(pp), "var_pose": t(var)}, t(pose), gt_vertices=t(gt))
    return ev


def host_inputs(rec, sel):
    """What rank_inputs must hand out, from the records: mode 0 key = the 24 uncertainties added in joint order in fp64 / 24, rounded
    once; mode 1 = the corr_y / corr_x columns, crop-major."""
    unc = rec[:, evaluate.R_UNC:evaluate.R_UNC + 24]
    m = np.zeros(len(rec), np.float64)
    for j in range(24):
        m = m + unc[:, j].astype(np.float64)
    crop = ((m / 24.0).astype(np.float32), np.stack([rec[:, evaluate.R_MPJPE], rec[:, evaluate.R_PA], rec[:, evaluate.R_V2V]]))
    joint = (unc[:, sel].reshape(-1), rec[:, evaluate.R_POSE:evaluate.R_POSE + 24][:, sel].reshape(1, -1))
    return crop, joint


@pytest.mark.parametrize("splits,sel", [([5, 3], None), ([70], SEL), ([5, 3, 70], SEL[:1])])
def test_rank_inputs_are_the_records_columns(cuda, splits, sel):
    ev = stepped(cuda, splits, sel)
    before = ev.finish(return_records=True)
    want = host_inputs(before["records"], list(range(24)) if sel is None else sel)
    for mode in (0, 1):
        key, vals = ev.rank_inputs(mode)
        assert key.dtype == torch.float32 and vals.dtype == torch.float32 and vals.shape == (3 if mode == 0 else 1, key.shape[0])
        assert np.array_equal(key.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[mode][0]).view(np.uint32)), mode
        assert np.array_equal(vals.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[mode][1]).view(np.uint32)), mode
    assert np.array_equal(want[1][0], before["corr_y"]) and np.array_equal(want[1][1][0], before["corr_x"])
    after = ev.finish(return_records=True)
    assert np.array_equal(after["records"].view(np.uint32), before["records"].view(np.uint32))     # the records are only read
    assert after["val_corr"] == before["val_corr"]
    summ = ev.uncert_summary()
    assert abs(summ["val_var"] - float(np.mean(want[0][0].astype(np.float64)))) <= 1e-6 * summ["val_var"]      # the same u_i
    with pytest.raises(_lib.PocoHipError, match="mode"):
        ev.rank_inputs(2)
    ev.reset()
    with pytest.raises(_lib.PocoHipError, match="no crop"):
        ev.rank_inputs(0)
    ev.close()


@pytest.mark.parametrize("splits,K", [([5, 3], 20), ([70], 7), ([5, 3, 70], 1024)])
def test_rank_metrics_match_the_yardstick(cuda, splits, K):
    ev = stepped(cuda, splits, SEL, seed=21)
    rec = ev.finish(return_records=True)["records"]
    rm = ranking.RankMetrics(ev, K)
    got = rm.result
    assert set(got) == set(ranking.RANK_NPZ_KEYS)
    summ = dict(zip(ranking.RANK_SUMMARY_FIELDS, got["rank_summary"]))
    assert summ["K"] == K
    tol = lambda n, mag: (n + K + 2) * U * mag   # noqa: E731  the device's sum of n terms, then the host's of K
    for (key, vals), names, tag in zip(host_inputs(rec, SEL), (ranking.CROP_METRICS, ranking.JOINT_METRICS), ("crop", "joint")):
        n = len(key)
        cuts, mags, cut_keys = rank_np.cut_sums(key, vals, K)
        cnt = np.maximum(np.asarray(rank_np.cut_counts(n, K), np.float64), 1.0)
        for e, name in enumerate(names):
            curve = rank_np.sparsification(cuts[e + 1], n)
            oracle = rank_np.sparsification(rank_np.cut_sums(vals[e], None, K)[0][0], n)
            bound = tol(n, (mags[e + 1] / cnt)[:0:-1])
            ok = ~np.isnan(curve)
            for g, w in ((got[f"rank_spars_{name}"], curve), (got[f"rank_oracle_{name}"], oracle)):
                assert np.array_equal(np.isnan(g), np.isnan(w)) and np.all(np.abs(g - w)[ok] <= bound[ok]), name
            scale = (np.nansum(np.abs(curve)) + np.nansum(np.abs(oracle))) / abs(curve[0]) / K + 1.0
            assert abs(summ[f"ause_{name}"] - rank_np.ause(curve, oracle)) <= tol(n, scale), name
            assert abs(summ[f"aurg_{name}"] - rank_np.aurg(curve)) <= tol(n, scale), name
            want = rank_np.spearman(key, vals[e])
            print(f"{tag} {name} n={n} K={K}: spearman {summ['spearman_' + name]} (yardstick {want})")
            assert abs(summ[f"spearman_{name}"] - want) <= 64 * U, name
        rel, wrel = got[f"rank_reliab_{tag}"], rank_np.reliability(cuts, n)
        bins = np.maximum(np.diff(rank_np.cut_counts(n, K)), 1)
        rb = np.concatenate([np.zeros((K, 1)), tol(n, ((mags[:, 1:] + mags[:, :-1]) / bins[None, :]).T)], axis=1)
        assert rel.shape == wrel.shape and np.array_equal(np.isnan(rel), np.isnan(wrel))
        assert np.all(np.abs(rel - wrel)[~np.isnan(wrel)] <= rb[~np.isnan(wrel)]), tag
        if tag == "crop":
            thr, wthr = got["rank_thresholds"], rank_np.threshold_table(cut_keys, cuts, n)
            tb = np.concatenate([np.zeros((K, 2)), tol(n, (mags[1:, 1:] / cnt[1:]).T)], axis=1)
            assert thr.shape == wthr.shape and np.array_equal(np.isnan(thr), np.isnan(wthr))
            assert np.all(np.abs(thr - wthr)[~np.isnan(wthr)] <= tb[~np.isnan(wthr)])
    lines = rm.lines()
    assert lines[0].startswith("Uncert Error Spearman (per joint): ") and len(lines) == 7 + K
    assert sum(line.startswith("AUSE / AURG ") for line in lines) == 4
    again = ranking.RankMetrics(ev, K).result                                                  # run to run: the same bits
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got)
    ev.close()


@pytest.fixture(scope="module")
def model():
    return util.make_engine("resnet50-cliff", max_batch=16)


def test_run_eval_with_and_without_rank_metrics(cuda, model, tmp_path):
    """The headline numbers and every array of the plain run are what they are without the argument; the .npz gains exactly the
    documented keys."""
    n = 24
    r = np.random.default_rng(4)
    path = tmp_path / "ds.npz"
    np.savez(path, imgname=np.array([f"im{i}.png" for i in range(n)]), center=r.uniform(80, 200, (n, 2)).astype(np.float32),
             scale=r.uniform(0.5, 1.0, n).astype(np.float32), pose=(0.4 * r.standard_normal((n, 72))).astype(np.float32),
             shape=(0.5 * r.standard_normal((n, 10))).astype(np.float32), img=r.standard_normal((n, 3, 224, 224)).astype(np.float32),
             orig_shape=np.tile([[240.0, 320.0]], (n, 1)).astype(np.float32))
    ds = evaluate.EvalDataset(str(path), None, "3dpw")
    J = synth.synth_j_regressor_h36m(11)
    plain = evaluate.run_eval(model, ds, J, batch_size=16)
    ranked = evaluate.run_eval(model, ds, J, batch_size=16, rank_metrics=5)
    assert set(ranked) - set(plain) == set(ranking.RANK_NPZ_KEYS) and not set(plain) - set(ranked)
    for k, v in plain.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, ranked[k], equal_nan=v.dtype.kind == "f"), k
        else:
            assert v == ranked[k] or (v != v and ranked[k] != ranked[k]), k
    evaluate.save_npz(str(tmp_path / "plain.npz"), plain, "3dpw")
    evaluate.save_npz(str(tmp_path / "ranked.npz"), ranked, "3dpw")
    zp, zr = dict(np.load(tmp_path / "plain.npz")), dict(np.load(tmp_path / "ranked.npz"))
    assert set(zr) - set(zp) == set(ranking.RANK_NPZ_KEYS) and not any(k.startswith("rank_") for k in zp)
    assert all(np.array_equal(zp[k], zr[k], equal_nan=zp[k].dtype.kind == "f") for k in zp)
    assert zr["rank_spars_mpjpe"].shape == (5,) and zr["rank_reliab_crop"].shape == (5, 5) and zr["rank_reliab_joint"].shape == (5, 3)
    assert zr["rank_thresholds"].shape == (5, 5) and zr["rank_summary"].shape == (len(ranking.RANK_SUMMARY_FIELDS),)
    assert abs(1000.0 * zr["rank_spars_mpjpe"][0] - ranked["val_mpjpe"]) <= 1e-9 * ranked["val_mpjpe"]     # entry 0 keeps every crop
    lines = evaluate.rank_lines(ranked)
    assert len(lines) == 7 + 5 and lines[1].startswith("Uncert Error Spearman (per crop, MPJPE): ")


def test_eval_cli_prints_the_block_and_writes_the_keys(tmp_path, cuda, capsys):
    """eval.py --rank_metrics --rank_bins 4 on 40 synthetic samples: the usual lines, then the new block; the .npz with the flag is the
    .npz without it plus the documented keys."""
    import importlib.util
    from pathlib import Path
    from tests.test_eval_gpu import _synthetic_eval_files
    spec = importlib.util.spec_from_file_location("poco_eval_cli_rank_gpu", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    _synthetic_eval_files(tmp_path)
    argv = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp_path / "ckpt.pt"), "--smpl", str(tmp_path / "smpl.npz"),
            "--j_regressor", str(tmp_path / "J.npy"), "--dataset", str(tmp_path / "ds_img.npz"), "--batch_size", "16"]
    plain = cli.main(cli.parse_args(argv + ["--output_folder", str(tmp_path / "plain")]))
    before = capsys.readouterr().out.splitlines()
    res = cli.main(cli.parse_args(argv + ["--output_folder", str(tmp_path / "ranked"), "--rank_metrics", "--rank_bins", "4"]))
    printed = capsys.readouterr().out.splitlines()
    assert before[-5:] == evaluate.report_lines(plain) and not any("Spearman" in line or "AUSE" in line for line in before)
    assert printed[:len(before)] == before                                                      # nothing above the block changes
    assert printed[len(before):] == evaluate.rank_lines(res) and len(printed) - len(before) == 7 + 4
    zp = dict(np.load(tmp_path / "plain" / "evaluation_results_3dpw.npz"))
    zr = dict(np.load(tmp_path / "ranked" / "evaluation_results_3dpw.npz"))
    assert set(zr) - set(zp) == set(ranking.RANK_NPZ_KEYS) and set(zp) <= set(zr)
    assert all(np.array_equal(zp[k], zr[k], equal_nan=zp[k].dtype.kind == "f") for k in zp)
    summ = dict(zip(ranking.RANK_SUMMARY_FIELDS, zr["rank_summary"]))
    assert summ["K"] == 4 and all(-1.0 <= summ[k] <= 1.0 for k in summ if k.startswith("spearman_"))
    want = rank_np.spearman(res["corr_y"], res["corr_x"])
    assert abs(summ["spearman_pose"] - want) <= 64 * U
