"""CPU: the evaluation contract - tests/eval_np.py against the reference-made fixture tests/golden/eval.npz
(tools/gen_eval_golden.py), the C ABI's declarations and argument checks (no GPU: poco_evaluator_create is host only and every
argument error is raised before any GPU work), the synthetic joint regressor and the eval.py CLI."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from poco_amd import _lib, evaluate, synth
from tests import eval_np

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "eval.npz"
SYMBOLS = ["poco_op_rodrigues", "poco_evaluator_create", "poco_evaluator_step", "poco_evaluator_finish", "poco_evaluator_reset",
           "poco_evaluator_destroy"]
QUANTITY = {"mpjpe": "mpjpe", "pampjpe": "pampjpe", "v2v": "v2v", "pred_jnts3D": "joints", "gt_jnts3D": "joints",
            "pred_jnts3D_nonrel": "joints"}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def inp():
    return eval_np.fixture_inputs()


def test_fixture_is_numbers_only_and_well_conditioned(gold):
    assert all(v.dtype.kind == "f" for v in gold.values())
    assert GOLD.stat().st_size < 1 << 20
    assert gold["min_sigma_ratio"] > 0.05
    dets = gold["dets"].reshape(len(eval_np.FIXTURE_COMBOS), eval_np.FIXTURE_CROPS)
    for row in dets:
        assert sorted(np.nonzero(row < 0)[0].tolist()) == list(eval_np.FIXTURE_MIRRORED)      # at least four mirrored crops, in
    assert len(eval_np.FIXTURE_MIRRORED) >= 4                                                 # both forms and both maps


@pytest.mark.parametrize("dtype,factor", [(np.float64, 1.0), (np.float32, 8.0)])
def test_eval_np_reproduces_golden(gold, inp, dtype, factor):
    """float64: within d_ref of each quantity (true by construction for a fresh fixture: pins the restatement to the file);
    float32: within 8 x d_ref, the margin the GPU test uses (two fp32 evaluations of one formula)."""
    for form, name in eval_np.FIXTURE_COMBOS:
        tag = f"{form}_{len(eval_np.joint_map(name))}"
        got = eval_np.evaluate(**eval_np.fixture_case(inp, form, name), dtype=dtype)
        for k, q in QUANTITY.items():
            err = np.abs(np.asarray(got[k], np.float64) - gold[f"{tag}_{k}"]).max()
            print(f"{dtype.__name__} {tag} {k}: {err:.3e} (d_ref {gold['d_ref_' + q]:.3e})")
            assert err <= factor * gold["d_ref_" + q], (tag, k, err)
        if form == "joints":
            assert np.all(got["v2v"] == 0)
    cx = eval_np.pose_distance(inp["pred_pose"], inp["gt_pose"], dtype)
    assert np.abs(cx.astype(np.float64) - gold["corr_x"]).max() <= factor * gold["d_ref_corr_x"]
    for kin in (True, False):
        cy = eval_np.processed_uncert(inp["var_pose"], kin, dtype)
        assert np.abs(cy.astype(np.float64) - gold["corr_y_kin" if kin else "corr_y_nokin"]).max() <= factor * gold["d_ref_corr_y"]
    rod = eval_np.rodrigues(inp["rod_aa"], dtype)
    assert np.abs(rod.astype(np.float64) - gold["rodrigues"]).max() <= factor * gold["d_ref_rodrigues"]


def test_pearson_matches_scipy_value(gold):
    r = eval_np.pearson(gold["corr_x"], gold["corr_y_kin"])
    assert abs(r - float(gold["pearson"][0])) <= 1e-9
    rec = np.zeros((eval_np.FIXTURE_CROPS, eval_np.RECORD_FLOATS), np.float32)
    rec[:, eval_np.R_POSE:eval_np.R_POSE + 24] = gold["corr_x"]
    rec[:, eval_np.R_UNC:eval_np.R_UNC + 24] = gold["corr_y_kin"]
    assert abs(eval_np.summary(rec)[4] - float(gold["pearson"][0])) <= 1e-9


def test_fixture_is_not_vacuous(gold, inp):
    """PA-MPJPE differs from MPJPE, and the mirrored crops need the reflection fix, by >= 100 x the GPU tolerance."""
    tol = 8 * gold["d_ref_pampjpe"]
    for form, name in eval_np.FIXTURE_COMBOS:
        tag = f"{form}_{len(eval_np.joint_map(name))}"
        assert np.abs(gold[f"{tag}_pampjpe"] - gold[f"{tag}_mpjpe"]).mean(-1).min() >= 100 * tol
        nofix = eval_np.evaluate(**eval_np.fixture_case(inp, form, name), dtype=np.float64, sign_fix=False)["pampjpe"]
        m = list(eval_np.FIXTURE_MIRRORED)
        assert np.abs(nofix[m] - gold[f"{tag}_pampjpe"][m]).mean(-1).min() >= 100 * tol


def test_header_declares_evaluator_and_keeps_abi_4():
    syms = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in syms, s
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt
    assert f"#define POCO_EVAL_RECORD_FLOATS {evaluate.RECORD_FLOATS}" in txt and evaluate.RECORD_FLOATS == eval_np.RECORD_FLOATS
    L = _lib.lib()
    L.poco_abi_version.restype = C.c_int
    assert L.poco_abi_version() == 4
    for s in SYMBOLS:
        assert hasattr(L, s), s


def _create(L, J=17, V=50, jmap=None, pelvis=0, sel=None, capacity=8, reg=True, out=True):
    jmap = np.asarray(eval_np.H36M_TO_J14 if jmap is None else jmap, np.int32)
    Jr = np.ones((max(J, 1), max(V, 1)), np.float32) / max(V, 1)
    sel = None if sel is None else np.asarray(sel, np.int32)
    h = C.c_void_p()
    rc = L.poco_evaluator_create(Jr.ctypes.data if reg else None, J, V, jmap.ctypes.data, len(jmap), pelvis,
                                 None if sel is None else sel.ctypes.data, 0 if sel is None else len(sel), 1, capacity,
                                 C.byref(h) if out else None)
    return rc, h


def test_argument_errors_without_a_gpu():
    """Every listed argument error returns POCO_ERR_ARG (1) before any GPU work: this test runs on a machine without one."""
    L = evaluate._bind()
    L.poco_op_rodrigues.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fake = C.c_void_p(4096)                        # never dereferenced: every call below is refused before the pointers are used
    assert L.poco_op_rodrigues(None, fake, 4, None) == 1 and L.poco_op_rodrigues(fake, None, 4, None) == 1
    assert L.poco_op_rodrigues(fake, fake, 0, None) == 1
    assert _create(L, reg=False)[0] == 1                               # null regressor
    assert _create(L, out=False)[0] == 1                               # null handle pointer
    assert _create(L, J=0, jmap=[0])[0] == 1 and _create(L, J=33, jmap=[0])[0] == 1         # J out of range
    assert _create(L, J=4, jmap=[0, 1, 2, 3, 0])[0] == 1               # M > J
    assert _create(L, jmap=[])[0] == 1                                 # M = 0
    assert _create(L, jmap=[0, 17])[0] == 1 and _create(L, jmap=[-1])[0] == 1                # map index >= J
    assert _create(L, pelvis=17)[0] == 1 and _create(L, pelvis=-1)[0] == 1                   # pelvis index >= J
    assert _create(L, sel=[24])[0] == 1 and _create(L, V=0)[0] == 1 and _create(L, capacity=0)[0] == 1
    assert b"poco_evaluator_create" in L.poco_last_error()
    rc, h = _create(L, capacity=8)
    assert rc == 0 and h.value
    try:
        step = lambda B, pv=fake, gv=fake, gj=None, pp=fake, gp=fake, var=fake, hh=h: L.poco_evaluator_step(   # noqa: E731
            hh, B, pv, gv, gj, pp, gp, var, 1, 1, None)
        assert step(4, hh=None) == 1                                   # null handle
        assert step(0) == 1 and step(-3) == 1                          # B <= 0
        assert step(4, pv=None) == 1 and step(4, pp=None) == 1 and step(4, gp=None) == 1 and step(4, var=None) == 1
        assert step(4, gv=fake, gj=fake) == 1                          # both ground truths
        assert step(4, gv=None, gj=None) == 1                          # neither
        assert step(9) == 1                                            # capacity overflow
        assert b"capacity" in L.poco_last_error()
        summ = (C.c_double * 8)()
        assert L.poco_evaluator_finish(None, summ, None, 0, None) == 1 and L.poco_evaluator_finish(h, None, None, 0, None) == 1
        assert L.poco_evaluator_finish(h, summ, None, 0, None) == 3    # nothing stepped: POCO_ERR_STATE, still no GPU work
        assert L.poco_evaluator_reset(None) == 1 and L.poco_evaluator_reset(h) == 0
    finally:
        L.poco_evaluator_destroy(h)
    L.poco_evaluator_destroy(None)


def test_synth_j_regressor_h36m():
    for V in (6890, 431):
        J = synth.synth_j_regressor_h36m(11, V)
        assert J.shape == (17, V) and J.dtype == np.float32
        assert np.abs(J.astype(np.float64).sum(1) - 1.0).max() < 1e-6 and J.min() >= 0
        assert (J != 0).sum(1).max() <= 24                             # sparse
        assert np.array_equal(J, synth.synth_j_regressor_h36m(11, V))  # seeded
    assert not np.array_equal(synth.synth_j_regressor_h36m(11), synth.synth_j_regressor_h36m(12))


def test_joint_maps():
    assert evaluate.joint_map("mpi-inf-3dhp") == eval_np.H36M_TO_J17 and len(evaluate.joint_map("3dpw")) == 14
    assert evaluate.joint_map("h36m-p2") == eval_np.H36M_TO_J17[:14]


def test_eval_cli_help_and_dataset_refusal(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "--j_regressor" in r.stdout and "--dataset_name" in r.stdout
    bad = tmp_path / "bad.npz"
    np.savez(bad, imgname=np.array(["a.png"]), center=np.zeros((1, 2)), scale=np.ones(1))
    r = subprocess.run([sys.executable, str(ROOT / "eval.py"), "--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt",
                        "--j_regressor", "none.npy", "--dataset", str(bad)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "neither" in r.stderr                 # refused before the engine (or torch) is touched
    with pytest.raises(ValueError):
        evaluate.check_dataset_keys(["imgname", "center", "scale", "pose"])
    assert evaluate.check_dataset_keys(["imgname", "center", "scale", "pose", "shape"]) == "smpl"
    assert evaluate.check_dataset_keys(["imgname", "center", "scale", "S"]) == "joints"
