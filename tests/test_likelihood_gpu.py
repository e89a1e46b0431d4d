"""GPU: the flow likelihood (csrc/eval_likelihood.hip, POCO.flow_context / flow_nll, evaluate.LikelihoodAccumulator) and the
evaluator's Var-MPJPE / Variance against the reference-made fixture tests/golden/likelihood.npz and tests/likelihood_np.py in
float64.  Tolerances: 8 x d_ref of the quantity as stored in the fixture (d_ref = how far the reference's own float32 results are
from float64; the factor 8 is the one tests/test_eval_gpu.py uses: the summation order differs from the reference's) for the
context, the residual, log sigma, the per-crop sums and the three means; for log_phi the rule tests/test_model_gpu.py::test_realnvp_op
applies to the same kernel: 1e-3 x max(1, max |log_phi|).  Every crop is compared."""
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import evaluate
from tests import eval_np, likelihood_np as lnp, util

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "likelihood.npz"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


class Case:
    def __init__(self, variant, cuda):
        self.variant, self.tag, self.cuda = variant, lnp.case_tag(variant), cuda
        self.model = util.make_engine(variant, max_batch=16)
        self.w = lnp.flow_weights(variant)
        self.inp = lnp.fixture_inputs(variant)
        self.valid = self.inp["has_smpl"].astype(bool)
        self.ctx64 = lnp.context(self.w, self.inp["uncert_feat"], np.float64)
        self.y64 = lnp.flow_nll(self.w, self.inp["pred_pose"], self.inp["gt_pose"], self.inp["var_pose"], self.ctx64, self.inp["has_smpl"],
                                np.float64)

    def dev(self, idx=None):
        """(pred dict, gt_pose, valid) of fixture crops `idx` (default: all 16) on the device."""
        idx = np.arange(lnp.FIXTURE_CROPS) if idx is None else np.asarray(idx)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[idx])).to(self.cuda)   # noqa: E731
        pred = {"pred_pose": t(self.inp["pred_pose"]), "var_pose": t(self.inp["var_pose"]), "uncert_feat": t(self.inp["uncert_feat"])}
        return pred, t(self.inp["gt_pose"]), t(self.inp["has_smpl"])

    def records(self, idx=None, valid=True):
        pred, gp, v = self.dev(idx)
        return self.model.flow_nll(pred, gp, v if valid else None).cpu().numpy()


@pytest.fixture(scope="module", params=[c[0] for c in lnp.FIXTURE_CASES])
def case(request, cuda):
    return Case(request.param, cuda)


def log_phi_tol(ref_lp):
    return 1e-3 * max(1.0, float(np.abs(ref_lp).max()))


def test_flow_context(case, gold):
    ctx = case.model.flow_context(torch.from_numpy(case.inp["uncert_feat"]).to(case.cuda)).cpu().numpy()
    tol = 8.0 * float(gold["d_ref_ctx"])
    d64 = np.abs(ctx.astype(np.float64) - case.ctx64).max()
    dg = np.abs(ctx[:, ::lnp.CTX_KEEP].astype(np.float64) - gold[f"{case.tag}_ctx"]).max()
    print(f"{case.tag} context: vs float64 {d64:.3e}, vs reference {dg:.3e} (tolerance {tol:.3e})")
    assert ctx.shape == (16, 512) and d64 <= tol and dg <= tol
    assert np.abs(case.ctx64).std() > 1000 * tol                       # not vacuous
    one = case.model.flow_context(torch.from_numpy(case.inp["uncert_feat"][5:6]).to(case.cuda)).cpu().numpy()
    assert np.array_equal(one[0], ctx[5])                              # a row does not depend on its neighbours


def test_records_and_summary_match_golden_and_float64(case, gold):
    rec = case.records()
    v, y, tag = case.valid, case.y64, case.tag
    want = lnp.records(y)
    g = {"log_phi": gold[f"{tag}_log_phi"], "log_sigma": gold[f"{tag}_log_sigma"], "sum": gold[f"{tag}_sum"],
         "bar": gold[f"{tag}_bar"].astype(np.float64).reshape(-1, 24, 9).mean(-1)}
    fields = {"bar": (lnp.N_BAR, 24, 8.0 * float(gold["d_ref_bar"])), "log_sigma": (lnp.N_LOGSIGMA, 24, 8.0 * float(gold["d_ref_log_sigma"])),
              "sum": (lnp.N_SUM, 1, 8.0 * float(gold["d_ref_sum"])), "log_phi": (lnp.N_LOGPHI, 24, log_phi_tol(y["log_phi"][v]))}
    ok = True
    for k, (o, n, tol) in fields.items():
        got = rec[:, o:o + n].astype(np.float64)
        d64 = np.abs(got - want[:, o:o + n]).max()                      # all 16 crops: the invalid ones are zero on both sides
        dg = np.abs(got[v] - g[k].reshape(int(v.sum()), n)).max()
        print(f"{tag} {k}: vs float64 {d64:.3e}, vs reference {dg:.3e} (tolerance {tol:.3e})")
        ok = ok and d64 <= tol and dg <= tol
    assert np.array_equal(rec[:, lnp.N_VALID], v.astype(np.float32)) and np.all(rec[:, 2:8] == 0)
    summ = case.model.flow_nll_summary(torch.from_numpy(rec).to(case.cuda))
    n64, *m64 = lnp.summary(want)
    tol = 8.0 * float(gold["d_ref_mean"])
    d64 = np.abs(summ[1:] - np.array(m64)).max()
    dg = np.abs(summ[1:] - gold[f"{tag}_mean"]).max()
    print(f"{tag} means (log phi, log sigma, loss_nf) {summ[1:]}: vs float64 {d64:.3e}, vs reference {dg:.3e} (tolerance {tol:.3e})")
    assert summ[0] == n64 == int(v.sum())
    assert ok and d64 <= tol and dg <= tol
    # the reduction itself, on the records it was given: fp64 in a fixed order
    assert np.abs(summ[1:] - np.array(lnp.summary(rec)[1:])).max() <= 1e-12 * np.abs(summ[1:]).max()


def test_invalid_crops(case):
    rec = case.records()
    for b in lnp.FIXTURE_INVALID:
        assert np.all(rec[b] == 0)
    allv = case.records(valid=False)                                    # NULL = every crop
    keep = case.valid
    assert np.array_equal(allv[keep], rec[keep]) and np.all(allv[:, lnp.N_VALID] == 1) and np.all(allv[~keep, lnp.N_SUM] != 0)
    s_some, s_all = (case.model.flow_nll_summary(torch.from_numpy(r).to(case.cuda)) for r in (rec, allv))
    assert s_some[0] == keep.sum() and s_all[0] == 16 and s_some[3] != s_all[3]
    # an invalid crop's inputs do not leak, whatever they are
    pred, gp, v = case.dev()
    gp = gp.clone()
    gp[lnp.FIXTURE_INVALID[0]] = float("nan")
    pred = dict(pred, var_pose=pred["var_pose"].clone())
    pred["var_pose"][lnp.FIXTURE_INVALID[1]] = 0.0
    assert np.array_equal(case.model.flow_nll(pred, gp, v).cpu().numpy(), rec)
    # no valid crop at all: count 0, NaN means
    none = case.model.flow_nll(pred, gp, torch.zeros_like(v))
    assert torch.all(none == 0)
    s = case.model.flow_nll_summary(none)
    assert s[0] == 0 and np.isnan(s[1:]).all()


def test_bitwise_repeatable_and_independent_of_batching(case):
    a, b = case.records(), case.records()
    assert np.array_equal(a, b)
    for idx in ([9], list(range(4, 11)), list(range(16))):              # B = 1, 7, 16
        assert np.array_equal(case.records(idx), a[idx]), len(idx)
    # 130 crops (crop i = fixture crop i % 16) in ragged steps through the accumulator
    lk = evaluate.LikelihoodAccumulator(case.model, capacity=130)
    assert lk.capacity == 130
    lo = 0
    for n in (16, 7, 1, 16, 16, 13, 16, 16, 16, 13):
        idx = np.arange(lo, lo + n) % lnp.FIXTURE_CROPS
        pred, gp, v = case.dev(idx)
        lk.step(pred, gp, v)
        lo += n
    assert lo == 130 == lk.count
    with pytest.raises(evaluate.PocoHipError, match="capacity"):
        lk.step(*case.dev([0]))
    res = lk.finish(return_records=True)
    assert np.array_equal(res["nll_records"], a[np.arange(130) % 16])
    assert res["log_phi"].shape == res["log_sigma"].shape == res["bar_pose"].shape == (130, 24)
    assert res["nll_N"] == int(case.valid[np.arange(130) % 16].sum())
    want = lnp.summary(res["nll_records"])
    assert abs(res["val_nll"] - want[3]) <= 1e-12 * abs(want[3]) and abs(res["val_log_phi"] - want[1]) <= 1e-12 * abs(want[1])
    again = lk.finish(return_records=True)
    assert np.array_equal(again["nll_records"], res["nll_records"]) and again["val_nll"] == res["val_nll"]
    lk.reset()
    assert lk.count == 0
    lk.step(*case.dev())
    assert np.array_equal(lk.finish(return_records=True)["nll_records"], a)
    with pytest.raises(evaluate.PocoHipError):                          # more crops than the engine was planned for
        case.model.flow_nll(*case.dev(np.arange(17) % 16))


def test_var_mpjpe_and_variance(cuda):
    """On the evaluator's own records, which the call leaves as they were."""
    from tests.test_eval_gpu import run, tile
    data, _ = tile(eval_np.fixture_inputs(), 40)
    for kin in (True, False):
        ev = run(cuda, data, "verts", "3dpw", kinematic=kin, finish=False)
        before = ev.finish(return_records=True)
        got = ev.uncert_summary()
        after = ev.finish(return_records=True)
        assert np.array_equal(before["records"], after["records"]) and np.array_equal(before["summary"], after["summary"])
        want = lnp.uncert_summary(before["records"])
        print(f"kinematic={kin}: Var-MPJPE {got['val_mpjpe_var']} (numpy {want[0]}), Variance {got['val_var']} (numpy {want[1]})")
        assert abs(got["val_mpjpe_var"] - want[0]) <= 1e-9 * abs(want[0]) and abs(got["val_var"] - want[1]) <= 1e-9 * abs(want[1])
        assert got == ev.uncert_summary()
        ev.close()


def test_eval_cli_likelihood_end_to_end(tmp_path, cuda, gold, capsys):
    """eval.py --likelihood on 40 synthetic samples with `img` crops, --batch_size 16 (ragged last batch of 8): the three new
    lines, then the unchanged five; values equal run_eval's; the .npz holds the new keys; without the flag nothing changes."""
    import importlib.util
    from tests.test_eval_gpu import _synthetic_eval_files
    spec = importlib.util.spec_from_file_location("poco_eval_cli", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = _synthetic_eval_files(tmp_path)
    argv = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp_path / "ckpt.pt"), "--smpl", str(tmp_path / "smpl.npz"),
            "--j_regressor", str(tmp_path / "J.npy"), "--dataset", str(tmp_path / "ds_img.npz"), "--batch_size", "16"]
    plain = cli.main(cli.parse_args(argv + ["--output_folder", str(tmp_path / "plain")]))
    printed = capsys.readouterr().out.splitlines()
    assert printed[-5:] == evaluate.report_lines(plain) and not any("Flow NLL" in p or "Var-MPJPE" in p for p in printed)
    assert "val_nll" not in plain and "val_nll" not in np.load(tmp_path / "plain" / "evaluation_results_3dpw.npz").files
    res = cli.main(cli.parse_args(argv + ["--likelihood", "--output_folder", str(tmp_path / "out")]))
    printed = capsys.readouterr().out.splitlines()
    assert printed[-8:-5] == evaluate.likelihood_lines(res) and printed[-5:] == evaluate.report_lines(res)
    assert printed[-8].startswith("Var-MPJPE: ") and printed[-7].startswith("Variance: ") and printed[-6].startswith("Flow NLL: ")
    assert evaluate.report_lines(res) == evaluate.report_lines(plain)                   # the five lines do not move
    for k in ("mpjpe", "pampjpe", "v2v", "corr_x", "corr_y"):
        assert np.array_equal(res[k], plain[k]), k
    z = dict(np.load(tmp_path / "out" / "evaluation_results_3dpw.npz"))
    for k in ("val_nll", "val_log_phi", "val_log_sigma", "val_mpjpe_var", "val_var"):
        assert float(z[k]) == res[k] and np.isfinite(res[k]), k
    for k in ("log_phi", "log_sigma", "bar_pose"):
        assert z[k].shape == (40, 24) and np.array_equal(z[k], res[k]), k
    assert res["nll_N"] == 40 and all(v.dtype.kind in "fiu" for v in z.values())
    # run_eval itself on the same files, and the numpy path on the model's own outputs for the same crops
    from poco_amd.tester import POCOTester
    args = cli.parse_args(argv)
    tester = POCOTester(args)
    ds = evaluate.EvalDataset(args.dataset, args.img_dir, "3dpw")
    J = np.load(tmp_path / "J.npy")
    kin = bool(tester.model_cfg.POCO.KINEMATIC_UNCERT)
    again = evaluate.run_eval(tester.model, ds, J, batch_size=16, kinematic=kin, likelihood=True, return_records=True)
    for k in ("val_nll", "val_log_phi", "val_log_sigma", "val_mpjpe_var", "val_var"):
        assert again[k] == res[k], k
    assert np.array_equal(again["log_phi"], res["log_phi"])
    vm, vv = lnp.uncert_summary(again["records"])
    assert abs(res["val_mpjpe_var"] - vm) <= 1e-9 * abs(vm) and abs(res["val_var"] - vv) <= 1e-9 * abs(vv)
    w = lnp.flow_weights("resnet50-cliff")
    host = {k: [] for k in ("log_phi", "log_sigma", "bar_pose")}
    for lo in range(0, 40, 16):
        hi = min(lo + 16, 40)
        out = tester.model(ds.batch(lo, hi, cuda), want_segm=False)
        c = lambda t: t.cpu().numpy()   # noqa: E731
        ctx = lnp.context(w, c(out["uncert_feat"]), np.float64)
        y = lnp.flow_nll(w, c(out["pred_pose"]), base["pose"][lo:hi], c(out["var_pose"]), ctx, None, np.float64)
        for k in host:
            host[k].append(y[k])
    host = {k: np.concatenate(v) for k, v in host.items()}
    lp_tol = log_phi_tol(host["log_phi"])
    d = {k: float(np.abs(res[k] - host[k]).max()) for k in host}
    print(f"end to end vs numpy float64 on the model's outputs: {d} (log_phi tolerance {lp_tol:.3e}); val_nll {res['val_nll']}")
    assert d["log_phi"] <= lp_tol and d["log_sigma"] <= 8.0 * float(gold["d_ref_log_sigma"])
    assert d["bar_pose"] <= 8.0 * float(gold["d_ref_bar"]) * max(1.0, float(np.abs(host["bar_pose"]).max()) / float(np.abs(gold["cliff_bar"]).max()))
    want_nll = float((host["log_sigma"] - host["log_phi"]).mean())
    assert abs(res["val_nll"] - want_nll) <= lp_tol
