"""GPU: the evaluator (csrc/eval_metrics.hip, poco_amd/evaluate.py) against the reference-made fixture tests/golden/eval.npz and
against tests/eval_np.py in float64.  Tolerance per quantity: 8 x d_ref of that quantity as stored in the fixture (d_ref = how far
the reference's own float32 results are from float64), never looser than the project's parity gate of 1e-3."""
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import evaluate, ops, postproc, synth
from tests import eval_np, util

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "eval.npz"
QUANTITY = {"mpjpe": "mpjpe", "mpjpe_mean": "mpjpe", "pampjpe": "pampjpe", "pampjpe_mean": "pampjpe", "v2v": "v2v",
            "pred_jnts3D": "joints", "gt_jnts3D": "joints", "pred_jnts3D_nonrel": "joints", "corr_x": "corr_x", "corr_y": "corr_y"}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def inp():
    return eval_np.fixture_inputs()


def tol(gold, q):
    return min(8.0 * float(gold["d_ref_" + q]), 1e-3)


def tile(inp, n):
    """n crops: the 16 fixture crops repeated (crop i = fixture crop i % 16)."""
    idx = np.arange(n) % eval_np.FIXTURE_CROPS
    out = {k: v[idx] for k, v in inp.items() if k not in ("J_regressor", "gt_joints", "rod_aa")}
    out["gt_joints"] = {k: v[idx] for k, v in inp["gt_joints"].items()}
    out["J_regressor"] = inp["J_regressor"]
    return out, idx


def run(cuda, data, form, name, splits=None, J=None, kinematic=True, capacity=None, ev=None, finish=True):
    """Step `data` through an evaluator in batches of `splits` (default: one step); returns finish(return_records=True)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    n = len(data["pred_vertices"])
    if ev is None:
        ev = evaluate.Evaluator(data["J_regressor"] if J is None else J, eval_np.joint_map(name), capacity=capacity or n,
                                kinematic=kinematic, device=cuda)
    lo = 0
    for b in (splits or [n]):
        sl = slice(lo, lo + b)
        pred = {"smpl_vertices": t(data["pred_vertices"][sl]), "pred_pose": t(data["pred_pose"][sl]), "var_pose": t(data["var_pose"][sl])}
        if form == "verts":
            ev.step(pred, t(data["gt_pose"][sl]), gt_vertices=t(data["gt_vertices"][sl]))
        else:
            ev.step(pred, t(data["gt_pose"][sl]), gt_joints=t(data["gt_joints"][name][sl]))
        lo += b
    assert lo == n
    return ev.finish(save_results=True, return_records=True) if finish else ev


@pytest.mark.parametrize("B", [1, 7, 16, 64, 130])
@pytest.mark.parametrize("form,name", eval_np.FIXTURE_COMBOS)
def test_records_match_golden_and_float64(cuda, gold, inp, B, form, name):
    """Both ground-truth forms x both joint maps x B = 1, 7, 16, 64, 130 against the reference's values and eval_np in float64."""
    data, idx = tile(inp, B)
    M = len(eval_np.joint_map(name))
    tag = f"{form}_{M}"
    res = run(cuda, data, form, name)
    got = eval_np.unpack(res["records"], M)
    y64 = eval_np.evaluate(**eval_np.fixture_case(inp, form, name), dtype=np.float64)
    for k, q in QUANTITY.items():
        want64 = np.asarray(y64[k])[idx]
        d64 = np.abs(got[k].astype(np.float64) - want64).max()
        line = f"B={B} {tag} {k}: vs float64 {d64:.3e}"
        assert d64 <= tol(gold, q), (k, d64, tol(gold, q))
        gk = {"corr_x": "corr_x", "corr_y": "corr_y_kin"}.get(k, f"{tag}_{k}")
        if gk in gold:
            dg = np.abs(got[k].astype(np.float64) - gold[gk][idx]).max()
            line += f", vs reference {dg:.3e}"
            assert dg <= tol(gold, q), (k, dg, tol(gold, q))
        print(line + f" (tolerance {tol(gold, q):.3e})")
    if form == "joints":
        assert np.all(res["v2v"] == 0.0)                                # exactly 0 with joint ground truth
    assert res["mpjpe"].shape == (B, M) and res["pred_jnts3D"].shape == (B, M, 3) and res["corr_x"].shape == (B * 24,)
    assert np.all(res["records"][:, eval_np.R_MPJPE_J + M:eval_np.R_PA_J] == 0)      # unused joint slots are 0


def test_fixture_is_not_vacuous_on_gpu_tolerance(gold, inp):
    """A kernel that skips the alignment or the reflection fix fails: both change the PA values by >= 100 x the tolerance."""
    t_pa = tol(gold, "pampjpe")
    for form, name in eval_np.FIXTURE_COMBOS:
        tag = f"{form}_{len(eval_np.joint_map(name))}"
        assert np.abs(gold[f"{tag}_pampjpe"] - gold[f"{tag}_mpjpe"]).mean(-1).min() >= 100 * t_pa
        nofix = eval_np.evaluate(**eval_np.fixture_case(inp, form, name), dtype=np.float64, sign_fix=False)["pampjpe"]
        m = list(eval_np.FIXTURE_MIRRORED)
        assert np.abs(nofix[m] - gold[f"{tag}_pampjpe"][m]).mean(-1).min() >= 100 * t_pa


def test_dense_regressor(cuda, gold, inp):
    """A regressor without a single zero (every row touches all 6890 vertices) against eval_np float64, and the sparse one given
    with its zeros spelled out in a dense matrix (the only way to give it) is what every other test uses."""
    r = np.random.default_rng(5)
    Jd = r.dirichlet(np.ones(6890), 17).astype(np.float32)
    assert (Jd != 0).all()
    data, idx = tile(inp, 16)
    res = run(cuda, data, "verts", "mpi-inf-3dhp", J=Jd)
    got = eval_np.unpack(res["records"], 17)
    kw = eval_np.fixture_case(inp, "verts", "mpi-inf-3dhp")
    kw["J_regressor"] = Jd
    y64 = eval_np.evaluate(**kw, dtype=np.float64)
    for k in ("mpjpe", "pampjpe", "v2v", "pred_jnts3D", "gt_jnts3D", "pred_jnts3D_nonrel"):
        d = np.abs(got[k].astype(np.float64) - y64[k]).max()
        print(f"dense regressor {k}: {d:.3e}")
        assert d <= tol(gold, QUANTITY[k]), (k, d)


def test_small_mesh_and_odd_sizes(cuda, gold):
    """V = 431 (one partial slice), V = 2500 (three slices, the last one partial), J = 5, M = 3, pelvis = 2."""
    r = np.random.default_rng(9)
    for V in (431, 2500):
        Jr = np.zeros((5, V), np.float32)
        for j in range(5):
            Jr[j, r.choice(V, 6, replace=False)] = r.dirichlet(np.ones(6)).astype(np.float32)
        B = 5
        gt = r.uniform(-0.5, 0.5, (B, V, 3)).astype(np.float32)
        pred = (gt + 0.02 * r.standard_normal(gt.shape)).astype(np.float32)
        pose = r.uniform(-1, 1, (B, 72)).astype(np.float32)
        pp = eval_np.rodrigues(pose.reshape(-1, 3) + 0.1, np.float64).reshape(B, 24, 3, 3).astype(np.float32)
        var = r.uniform(0, 1, (B, 24)).astype(np.float32)
        ev = evaluate.Evaluator(Jr, [4, 0, 3], capacity=B, pelvis=2, device=cuda)
        t = lambda a: torch.from_numpy(a).to(cuda)   # noqa: E731
        ev.step({"smpl_vertices": t(pred), "pred_pose": t(pp), "var_pose": t(var)}, t(pose), gt_vertices=t(gt))
        got = eval_np.unpack(ev.finish(return_records=True)["records"], 3)
        y64 = eval_np.evaluate(pred, pp, var, pose, Jr, [4, 0, 3], gt_vertices=gt, pelvis=2, dtype=np.float64)
        for k in ("mpjpe", "pampjpe", "v2v", "pred_jnts3D", "gt_jnts3D", "corr_x"):
            assert np.abs(got[k].astype(np.float64) - y64[k]).max() <= tol(gold, QUANTITY[k]), (V, k)


def test_rodrigues_op(cuda, gold, inp):
    """poco_op_rodrigues against the reference's batch_rodrigues (zero vector, tiny angles, angles up to pi) and orthonormal to
    the threshold the rot6d test uses (1e-5)."""
    out = ops.rodrigues(torch.from_numpy(inp["rod_aa"]).to(cuda)).cpu().numpy()
    d = np.abs(out.astype(np.float64) - gold["rodrigues"]).max()
    print(f"rodrigues vs reference {d:.3e} (tolerance {tol(gold, 'rodrigues'):.3e})")
    assert out.shape == (64, 3, 3) and d <= tol(gold, "rodrigues")
    R = out.astype(np.float64)
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-5
    assert np.array_equal(out[0], np.eye(3, dtype=np.float32))         # the zero vector
    assert ops.rodrigues(torch.from_numpy(inp["gt_pose"]).to(cuda)).shape == (16, 24, 3, 3)


def test_pose_distance_of_a_pose_against_itself(cuda, gold, inp):
    data, _ = tile(inp, 16)
    data = dict(data)
    data["pred_pose"] = ops.rodrigues(torch.from_numpy(inp["gt_pose"]).to(cuda)).cpu().numpy()
    res = run(cuda, data, "verts", "3dpw")
    assert np.abs(res["corr_x"]).max() <= tol(gold, "corr_x")


def test_processed_uncertainty_matches_host(cuda, inp):
    """[B,24] (the engine's var_pose), kinematic accumulation on and off: BITWISE postproc.prepare_uncert (the same fp32 adds in the
    same order).  With trailing axes the mean is a sum and a division on both sides: at most 1 ulp apart."""
    data, _ = tile(inp, 16)
    for kin in (True, False):
        res = run(cuda, data, "verts", "3dpw", kinematic=kin)
        assert np.array_equal(res["corr_y"].reshape(16, 24), postproc.prepare_uncert(inp["var_pose"], kin))
    r = np.random.default_rng(2)
    for shape in ((16, 24, 3), (16, 24, 2, 3)):
        d2 = dict(data)
        d2["var_pose"] = r.uniform(0.01, 0.3, shape).astype(np.float32)
        res = run(cuda, d2, "verts", "3dpw", kinematic=False)
        np.testing.assert_array_max_ulp(res["corr_y"].reshape(16, 24), postproc.prepare_uncert(d2["var_pose"], False), maxulp=1)


def test_bitwise_repeatable_and_independent_of_batching(cuda, inp):
    """Two runs, and 64 = 16 x 4 = 7 + 57, and 300 crops (two sub-batches inside one step): the same bits."""
    data, _ = tile(inp, 64)
    a = run(cuda, data, "verts", "3dpw")
    b = run(cuda, data, "verts", "3dpw")
    assert np.array_equal(a["records"], b["records"], equal_nan=True) and np.array_equal(a["summary"], b["summary"])
    for splits in ([16] * 4, [7, 57]):
        c = run(cuda, data, "verts", "3dpw", splits=splits)
        assert np.array_equal(a["records"], c["records"]) and np.array_equal(a["summary"], c["summary"])
    big, _ = tile(inp, 300)
    d = run(cuda, big, "joints", "3dpw")
    e = run(cuda, big, "joints", "3dpw", splits=[100, 200])
    assert np.array_equal(d["records"], e["records"])
    assert np.array_equal(d["records"][:12], d["records"][288:300])    # crop 288 + i is fixture crop i again


def test_finish_summary_reset_and_capacity(cuda, inp):
    data, _ = tile(inp, 40)
    ev = run(cuda, data, "verts", "3dpw", capacity=48, finish=False)
    res = ev.finish(return_records=True)
    n, mp, pa, vv, corr = eval_np.summary(res["records"])
    assert res["N"] == n == 40
    for got, want in ((res["val_mpjpe"], mp), (res["val_pampjpe"], pa), (res["val_v2v"], vv)):
        assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(res["val_corr"] - corr) <= 1e-9
    # capacity overflow: an error, the earlier records stay
    small, _ = tile(inp, 9)
    with pytest.raises(evaluate.PocoHipError):
        run(cuda, small, "verts", "3dpw", ev=ev, finish=False)
    again = ev.finish(return_records=True)
    assert again["N"] == 40 and np.array_equal(again["records"], res["records"])
    eight, _ = tile(inp, 8)
    full = run(cuda, eight, "verts", "3dpw", ev=ev)
    assert full["N"] == 48 and np.array_equal(full["records"][:40], res["records"]) and np.array_equal(full["records"][40:], res["records"][:8])
    # a subset of joints in the correlation
    ev.reset()
    assert ev.count == 0
    ev2 = evaluate.Evaluator(inp["J_regressor"], eval_np.joint_map("3dpw"), capacity=16, sel_uncert_part=[0, 3, 7, 23], device=cuda)
    r2 = run(cuda, tile(inp, 16)[0], "verts", "3dpw", ev=ev2)
    assert abs(r2["val_corr"] - eval_np.summary(r2["records"], [0, 3, 7, 23])[4]) <= 1e-9 and r2["corr_x"].shape == (64,)
    r1 = run(cuda, tile(inp, 16)[0], "verts", "3dpw", ev=ev)          # after reset: record 0 again
    assert r1["N"] == 16 and np.array_equal(r1["records"], res["records"][:16])


def test_degenerate_crop_does_not_disturb_the_others(cuda, inp):
    """One crop whose predicted joints all coincide (var1 = 0: the reference divides by zero) among 15 normal ones."""
    data, _ = tile(inp, 16)
    clean = run(cuda, data, "verts", "3dpw")
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in data.items()}
    bad["pred_vertices"][6] = np.float32(0.0)                          # every vertex at the origin: so is every joint, exactly
    res = run(cuda, bad, "verts", "3dpw")
    torch.cuda.synchronize()
    assert torch.cuda.is_available()                                   # the call returned and the device is alive
    keep = [i for i in range(16) if i != 6]
    assert np.array_equal(res["records"][keep], clean["records"][keep])
    assert np.isfinite(res["mpjpe"][6]).all() and not np.isfinite(res["pampjpe"][6]).all()


@pytest.fixture(scope="module")
def model():
    return util.make_engine("resnet50-cliff", max_batch=16)


def _host_metrics(out, gt_pose, gt_verts, J, name, kin):
    c = lambda t: t.cpu().numpy()   # noqa: E731
    return eval_np.evaluate(c(out["smpl_vertices"]), c(out["pred_pose"]), c(out["var_pose"]), gt_pose, J, eval_np.joint_map(name),
                            gt_vertices=gt_verts, kinematic=kin, dtype=np.float64)


def test_step_right_behind_the_forward(cuda, model, gold, inp):
    """The step enqueued on the forward's stream with no synchronisation in between == after a full synchronise."""
    J = inp["J_regressor"]
    batch = util.cuda_batch(synth.synth_batch(16, 77), cuda)
    gp = torch.from_numpy(inp["gt_pose"]).to(cuda)
    gv = torch.from_numpy(inp["gt_vertices"]).to(cuda)
    recs = []
    for sync in (False, True):
        ev = evaluate.Evaluator(J, eval_np.joint_map("3dpw"), capacity=16, device=cuda)
        out = model(batch, want_segm=False)
        if sync:
            torch.cuda.synchronize()
        ev.step(out, gp, gt_vertices=gv)
        recs.append(ev.finish(return_records=True)["records"])
    model.check_status()
    assert np.array_equal(recs[0], recs[1])
    y64 = _host_metrics(out, inp["gt_pose"], inp["gt_vertices"], J, "3dpw", True)
    assert np.abs(recs[0][:, eval_np.R_PA_J:eval_np.R_PA_J + 14] - y64["pampjpe"]).max() <= tol(gold, "pampjpe")


def _synthetic_eval_files(tmp_path, n=40):
    """Synthetic checkpoint, body model, joint regressor and a 40-sample SMPL-ground-truth dataset in both input forms."""
    from PIL import Image
    w = util.synth_weights("resnet50-cliff")
    sd = {"model." + k: torch.from_numpy(v) for k, v in w.items()}
    torch.save({"state_dict": sd}, tmp_path / "ckpt.pt")
    np.savez(tmp_path / "smpl.npz", **synth.synth_smpl(7))
    np.save(tmp_path / "J.npy", synth.synth_j_regressor_h36m(11))
    r = np.random.default_rng(4)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    frames = [r.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(4)]
    for i, f in enumerate(frames):
        Image.fromarray(f).save(imgs / f"im{i}.png")
    base = dict(imgname=np.array([f"im{i % 4}.png" for i in range(n)]), center=r.uniform(80, 200, (n, 2)).astype(np.float32),
                scale=r.uniform(0.5, 1.0, n).astype(np.float32), pose=(0.4 * r.standard_normal((n, 72))).astype(np.float32),
                shape=(0.5 * r.standard_normal((n, 10))).astype(np.float32))
    np.savez(tmp_path / "ds_files.npz", **base)
    np.savez(tmp_path / "ds_img.npz", img=r.standard_normal((n, 3, 224, 224)).astype(np.float32),
             orig_shape=np.tile([[240.0, 320.0]], (n, 1)).astype(np.float32), **base)
    return base


@pytest.mark.parametrize("form", ["img", "files"])
def test_eval_cli_end_to_end(tmp_path, cuda, gold, capsys, form):
    """eval.py on 40 synthetic samples, --batch_size 16 (ragged last batch of 8), against eval_np applied on the host to the
    model's own outputs for the same crops."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("poco_eval_cli", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = _synthetic_eval_files(tmp_path)
    argv = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp_path / "ckpt.pt"), "--smpl", str(tmp_path / "smpl.npz"),
            "--j_regressor", str(tmp_path / "J.npy"), "--dataset", str(tmp_path / f"ds_{form}.npz"), "--batch_size", "16",
            "--save_results", "--output_folder", str(tmp_path / "out")]
    if form == "files":
        argv += ["--img_dir", str(tmp_path / "imgs")]
    res = cli.main(cli.parse_args(argv))
    printed = capsys.readouterr().out.splitlines()
    assert printed[-5:] == evaluate.report_lines(res)
    z = dict(np.load(tmp_path / "out" / "evaluation_results_3dpw.npz"))
    assert int(z["N"]) == 40
    for k, shape in (("mpjpe", (40, 14)), ("pampjpe", (40, 14)), ("v2v", (40,)), ("corr_x", (960,)), ("corr_y", (960,)),
                     ("pred_jnts3D", (40, 14, 3)), ("gt_jnts3D", (40, 14, 3))):
        assert z[k].shape == shape and np.array_equal(z[k], res[k]), k
    assert all(v.dtype.kind in "fiu" for v in z.values())
    for k in ("val_mpjpe", "val_pampjpe", "val_v2v", "val_corr"):
        assert float(z[k]) == res[k]
    # the host path on the model's own outputs for the same crops
    from poco_amd.tester import POCOTester
    args = cli.parse_args(argv)
    tester = POCOTester(args)
    ds = evaluate.EvalDataset(args.dataset, args.img_dir, "3dpw")
    J = np.load(tmp_path / "J.npy")
    kin = bool(tester.model_cfg.POCO.KINEMATIC_UNCERT)
    host = {k: [] for k in ("mpjpe", "pampjpe", "v2v", "corr_x", "corr_y")}
    for lo in range(0, 40, 16):
        hi = min(lo + 16, 40)
        out = tester.model(ds.batch(lo, hi, cuda), want_segm=False)
        gp = torch.from_numpy(base["pose"][lo:hi]).to(cuda)
        gv, _ = tester.model.smpl_lbs(torch.from_numpy(base["shape"][lo:hi]).to(cuda), ops.rodrigues(gp))
        y = _host_metrics(out, base["pose"][lo:hi], gv.cpu().numpy(), J, "3dpw", kin)
        for k in host:
            host[k].append(y[k])
    for k in host:
        want = np.concatenate(host[k])
        assert np.abs(res[k].reshape(want.shape) - want).max() <= tol(gold, QUANTITY[k]), k
    mp = 1000.0 * np.concatenate(host["mpjpe"]).mean()
    assert abs(res["val_mpjpe"] - mp) <= 1000.0 * tol(gold, "mpjpe")
