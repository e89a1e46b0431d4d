"""CPU: the likelihood contract - tests/likelihood_np.py against the reference-made fixture tests/golden/likelihood.npz
(tools/gen_likelihood_golden.py), the C ABI's declarations and argument checks (every argument error is raised before any GPU
work: this file runs on a machine without one) and the eval.py command line."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import _lib, evaluate, model as pm
from tests import eval_np, likelihood_np as lnp, util

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "likelihood.npz"
SYMBOLS = ["poco_flow_context", "poco_flow_nll", "poco_flow_nll_reduce", "poco_evaluator_uncert_summary"]
ERR_ARG, ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_is_numbers_only_and_not_vacuous(gold):
    assert all(v.dtype.kind in "fi" for v in gold.values())
    assert GOLD.stat().st_size <= 100 * 1024
    for variant, L, in_ctx in lnp.FIXTURE_CASES:
        tag = lnp.case_tag(variant)
        inp = lnp.fixture_inputs(variant)
        nv = int(inp["has_smpl"].sum())
        assert len(inp["has_smpl"]) == 16 and 16 - nv >= 2
        assert inp["var_pose"].min() >= 0.05 and inp["var_pose"].max() <= 0.55 and inp["uncert_feat"].shape == (16, in_ctx)
        assert gold[f"{tag}_log_phi"].shape == (nv, 24) and gold[f"{tag}_bar"].shape == (nv * 24, 9)
        tol = 1e-3 * max(1.0, float(np.abs(gold[f"{tag}_log_phi"]).max()))          # the rule of tests/test_model_gpu.py::test_realnvp_op
        assert np.ptp(gold[f"{tag}_log_phi"].mean(1)) > 100 * tol                    # the crops differ ...
        assert gold[f"{tag}_moved"] > 100 * tol                                     # ... and so do permuted contexts (generator)
    assert {1, 3} == {L for _, L, _ in lnp.FIXTURE_CASES} and {2048, 3072} == {c for _, _, c in lnp.FIXTURE_CASES}


@pytest.mark.parametrize("variant,L,in_ctx", lnp.FIXTURE_CASES)
def test_likelihood_np_reproduces_golden(gold, variant, L, in_ctx):
    """float64: within d_ref of each quantity (true by construction for a fresh fixture: pins the restatement to the file)."""
    tag = lnp.case_tag(variant)
    w = lnp.flow_weights(variant)
    inp = lnp.fixture_inputs(variant)
    v = inp["has_smpl"].astype(bool)
    ctx = lnp.context(w, inp["uncert_feat"], np.float64)
    y = lnp.flow_nll(w, inp["pred_pose"], inp["gt_pose"], inp["var_pose"], ctx, inp["has_smpl"], np.float64)
    rec = lnp.records(y)
    got = {"ctx": ctx[:, ::lnp.CTX_KEEP], "bar": y["bar_rows"].reshape(-1, 24, 9)[v].reshape(-1, 9), "log_phi": y["log_phi"][v],
           "log_sigma": y["log_sigma"][v], "sum": y["sum"][v], "mean": np.array(lnp.summary(rec)[1:])}
    for k, a in got.items():
        err = np.abs(a - gold[f"{tag}_{k}"]).max()
        print(f"{tag} {k}: {err:.3e} (d_ref {gold['d_ref_' + k]:.3e})")
        assert err <= gold["d_ref_" + k], (k, err)
    assert np.all(rec[~v] == 0) and lnp.summary(rec)[0] == int(v.sum())
    n, lp, ls, loss = lnp.summary(np.zeros((3, 80)))
    assert n == 0 and np.isnan(lp) and np.isnan(ls) and np.isnan(loss)


def test_uncert_summary_reproduces_golden(gold):
    inp = lnp.fixture_inputs(lnp.FIXTURE_CASES[0][0])
    rec = np.zeros((lnp.FIXTURE_CROPS, eval_np.RECORD_FLOATS), np.float32)
    rec[:, eval_np.R_MPJPE] = gold["uncert_mpjpe"]
    rec[:, eval_np.R_UNC:eval_np.R_UNC + 24] = eval_np.processed_uncert(inp["var_pose"], True, np.float32)
    got = np.array(lnp.uncert_summary(rec))
    assert np.abs(got - gold["uncert_summary"]).max() <= gold["d_ref_uncert_summary"]
    assert got[0] > 0.05 and got[1] > 0.05          # metres over metres-scale sigma: O(0.1 .. 1), not scaled by 1000


def test_header_declares_the_entries_and_keeps_abi_4():
    syms = _lib.header_symbols()
    txt = _lib.HEADER.read_text()
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in syms and hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in txt
    assert f"#define POCO_FLOW_NLL_RECORD_FLOATS {lnp.RECORD_FLOATS}" in txt
    assert evaluate.NLL_RECORD_FLOATS == lnp.RECORD_FLOATS == pm.POCO.FLOW_NLL_RECORD_FLOATS
    assert (evaluate.N_VALID, evaluate.N_SUM, evaluate.N_LOGPHI, evaluate.N_LOGSIGMA, evaluate.N_BAR) == \
           (lnp.N_VALID, lnp.N_SUM, lnp.N_LOGPHI, lnp.N_LOGSIGMA, lnp.N_BAR)


def _engine(L, options=b"", max_batch=4, variant=b"resnet50-cliff"):
    h = C.c_void_p()
    assert L.poco_create_ex(variant, max_batch, 1, options, C.byref(h)) == 0, L.poco_last_error()
    return h


def test_argument_errors_without_a_gpu():
    """B > max_batch, null pointers, masked / excluded-joint variants: POCO_ERR_ARG; a checkpoint without cond_layer:
    POCO_ERR_STATE naming the tensor.  All before any GPU work (the engines here are never finalized)."""
    L = pm._bind()
    evaluate._bind()
    fake = C.c_void_p(4096)                        # never dereferenced
    h = _engine(L)
    try:
        nll = lambda B=2, pp=fake, gp=fake, var=fake, ctx=fake, out=fake, hh=h: L.poco_flow_nll(hh, B, pp, gp, var, ctx, None, out, None)   # noqa: E731
        assert nll(hh=None) == ERR_ARG
        assert nll(B=0) == ERR_ARG and nll(B=-1) == ERR_ARG
        assert nll(B=5) == ERR_ARG and b"max_batch" in L.poco_last_error()
        for k in ("pp", "gp", "var", "ctx", "out"):
            assert nll(**{k: None}) == ERR_ARG, k
        assert nll() == ERR_STATE                                       # a good call on an engine that is not finalized
        cx = lambda B=2, uf=fake, ctx=fake, hh=h: L.poco_flow_context(hh, B, uf, ctx, None)   # noqa: E731
        assert cx(hh=None) == ERR_ARG and cx(B=0) == ERR_ARG and cx(B=5) == ERR_ARG
        assert cx(uf=None) == ERR_ARG and cx(ctx=None) == ERR_ARG
        assert cx() == ERR_STATE and b"flow_head.cond_layer.weight" in L.poco_last_error()      # nothing loaded
        w = np.zeros((512, 2048), np.float32)
        shp = (C.c_int64 * 2)(512, 2048)
        assert L.poco_load_tensor(h, b"flow_head.cond_layer.weight", w.ctypes.data, shp, 2) == 0
        assert cx() == ERR_STATE and b"flow_head.cond_layer.bias" in L.poco_last_error()
        summ = (C.c_double * 4)()
        red = lambda N=4, rec=fake, s=summ, hh=h: L.poco_flow_nll_reduce(hh, N, rec, s, None)   # noqa: E731
        assert red(hh=None) == ERR_ARG and red(N=0) == ERR_ARG and red(rec=None) == ERR_ARG and red(s=None) == ERR_ARG
        assert red() == ERR_STATE
    finally:
        L.poco_destroy(h)
    for opt in (b"mask_params_id=1-4", b"exclude_uncert_idx=10-11", b"record_thr=0.3,mask_params_id=7"):
        h = _engine(L, opt)
        try:
            assert L.poco_flow_nll(h, 2, fake, fake, fake, fake, None, fake, None) == ERR_ARG
            assert b"MASK_PARAMS_ID" in L.poco_last_error()
        finally:
            L.poco_destroy(h)
    s2 = (C.c_double * 2)()
    assert L.poco_evaluator_uncert_summary(None, s2, None) == ERR_ARG
    Jr = np.ones((17, 50), np.float32) / 50
    jm = np.asarray(eval_np.H36M_TO_J14, np.int32)
    ev = C.c_void_p()
    assert L.poco_evaluator_create(Jr.ctypes.data, 17, 50, jm.ctypes.data, 14, 0, None, 0, 1, 8, C.byref(ev)) == 0
    try:
        assert L.poco_evaluator_uncert_summary(ev, None, None) == ERR_ARG
        assert L.poco_evaluator_uncert_summary(ev, s2, None) == ERR_STATE         # nothing stepped, still no GPU work
    finally:
        L.poco_evaluator_destroy(ev)


def test_masked_flow_is_declared_and_the_binding_passes_it_on():
    """POCO(mask_params_id=...) reaches the engine as a build option: the mask_params buffer of such a checkpoint loads strictly,
    and the default engine's tensor list is what it was."""
    base = pm.POCO(backbone="resnet50-cliff", num_flow_layers=1, max_batch=2)
    masked = pm.POCO(backbone="resnet50-cliff", num_flow_layers=1, max_batch=2, mask_params_id="1-4")
    nb, nm = [n for n, _, _ in base.expected_tensors()], [n for n, _, _ in masked.expected_tensors()]
    assert "flow_head.mask_params" not in nb and sorted(nm) == sorted(nb + ["flow_head.mask_params"])
    assert set(nb) == {n for n, _ in util.load_spec("resnet50-cliff")} | {n for n in nb if n.startswith("smpl.")}
    req = {n: r for n, _, r in base.expected_tensors()}
    assert req["flow_head.cond_layer.weight"] is False and req["flow_head.cond_layer.bias"] is False      # still required = 0
    with pytest.raises(pm.PocoHipError):
        pm.POCO(backbone="resnet50-cliff", num_flow_layers=1, max_batch=2, engine_options="no_such_option=1")


def test_report_lines_are_still_five_and_likelihood_lines_three():
    res = {"val_mpjpe": 1.0, "val_pampjpe": 2.0, "val_v2v": 3.0, "val_corr": 0.5, "N": 7, "val_mpjpe_var": 0.4, "val_var": 0.2,
           "val_nll": 8.25, "val_log_phi": -9.0, "val_log_sigma": -0.75, "nll_N": 6}
    lines = evaluate.report_lines(res)
    assert lines == ["MPJPE: 1.0", "PA-MPJPE: 2.0", "V2V (mm): 3.0", "Uncert Error Correlation: 0.5", "N: 7"]
    extra = evaluate.likelihood_lines(res)
    assert len(extra) == 3 and extra[0] == "Var-MPJPE: 0.4" and extra[1] == "Variance: 0.2" and extra[2].startswith("Flow NLL: 8.25")


def test_save_npz_stores_the_new_keys_when_present(tmp_path):
    base = {"val_mpjpe": 1.0, "val_pampjpe": 2.0, "val_v2v": 3.0, "val_corr": 0.5, "N": 2, "mpjpe": np.zeros((2, 14), np.float32)}
    evaluate.save_npz(str(tmp_path / "a.npz"), base, "3dpw")
    assert "val_nll" not in np.load(tmp_path / "a.npz").files
    more = dict(base, val_nll=8.0, val_log_phi=-9.0, val_log_sigma=-1.0, val_mpjpe_var=0.4, val_var=0.2,
                log_phi=np.ones((2, 24), np.float32), log_sigma=np.ones((2, 24), np.float32), bar_pose=np.ones((2, 24), np.float32))
    evaluate.save_npz(str(tmp_path / "b.npz"), more, "3dpw")
    z = np.load(tmp_path / "b.npz")
    for k in ("val_nll", "val_log_phi", "val_log_sigma", "val_mpjpe_var", "val_var"):
        assert float(z[k]) == more[k]
    for k in ("log_phi", "log_sigma", "bar_pose"):
        assert z[k].shape == (2, 24)


def test_eval_cli_lists_likelihood_and_refuses_early(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "--likelihood" in r.stdout
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--j_regressor", "none.npy", "--likelihood"]
    # joint ground truth without `pose`
    nopose = tmp_path / "nopose.npz"
    np.savez(nopose, imgname=np.array(["a.png"]), center=np.zeros((1, 2)), scale=np.ones(1), S=np.zeros((1, 24, 4)))
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), *common, "--ckpt", "none.pt", "--dataset", str(nopose)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "needs `pose`" in r.stderr
    # joint ground truth WITH `pose` passes that check; a checkpoint without the context layer is refused next
    withpose = tmp_path / "withpose.npz"
    np.savez(withpose, imgname=np.array(["a.png"]), center=np.zeros((1, 2)), scale=np.ones(1), S=np.zeros((1, 24, 4)),
             pose=np.zeros((1, 72)))
    torch.save({"state_dict": {"model.flow_head.flow.mask": torch.zeros(2, 9), "model.head.fc1.bias": torch.zeros(4)}}, tmp_path / "nocond.pt")
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), *common, "--ckpt", str(tmp_path / "nocond.pt"), "--dataset", str(withpose)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "flow_head.cond_layer.weight" in r.stderr and "no flow context layer" in r.stderr
