"""CPU: the evaluation contract - tests/eval_np.py against the reference-made fixture tests/golden/eval.npz
(tools/gen_eval_golden.py), the C ABI's declarations and argument checks (no GPU: poco_evaluator_create is host only and every
argument error is raised before any GPU work), the synthetic joint regressor and the eval.py CLI; and what the case generators of
tests/test_eval_solver_gpu.py promise (classes, conditioning, determinants, non-vacuity, the second oracle, the slice borders)."""
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


@pytest.fixture(scope="module")
def solver():
    """eval_np.solver_cases() with what the checks below share, per joint count: float64 conditioning / determinant per case and the
    float64 SVD route on the inputs tests/test_eval_solver_gpu.py hands the device."""
    out = {}
    for M, (S1, S2, tags) in eval_np.solver_cases().items():
        cd = np.array([eval_np.conditioning(a, g) for a, g in zip(S1, S2)])
        kw = eval_np.solver_inputs(M, S1, S2)
        out[M] = dict(S1=S1, S2=S2, tags=tags, cond=cd[:, 0], det=cd[:, 1], kw=kw, y64=eval_np.evaluate(**kw, dtype=np.float64))
    return out


def _full_rank_mirrored(c):
    """Mirrored cases whose K has rank 3.  With three joints, or a planar ground truth, sigma3 = 0: the mirror image is a rotated
    image as well, det(U V^T) is a coin toss and the reflection fix changes nothing, so those cases cannot need it."""
    return np.array([i for i, t in enumerate(c["tags"]) if t["mirrored"] and t["cls"] != "planar" and c["S1"].shape[1] >= 4], np.int64)


def test_solver_cases_are_seeded_and_hold_every_class(solver):
    again = eval_np.solver_cases()
    assert sorted(solver) == list(eval_np.SOLVER_JOINTS)
    bulk = 0
    for M, c in solver.items():
        S1, S2, tags = c["S1"], c["S2"], c["tags"]
        assert S1.dtype == S2.dtype == np.float32 and S1.shape == S2.shape == (len(tags), M, 3)
        assert np.array_equal(S1, again[M][0]) and np.array_equal(S2, again[M][1]) and tags == again[M][2]
        assert np.isfinite(S1).all() and np.isfinite(S2).all()
        combos = {(t["rot"], t["s"], t["noise"], t["mirrored"]) for t in tags if t["cls"] == "group"}
        assert combos == {(n, s, z, m) for n, _, _ in eval_np.SOLVER_ROTATIONS for s in (0.5, 1.3) for z in (0.0, 0.02) for m in (False, True)}
        assert len(eval_np.tag_index(tags, cls="group")) == len(combos) == 96
        assert np.abs(S1[eval_np.tag_index(tags, cls="group")]).max() > 5.0             # t of order metres
        u = [eval_np.tag_index(tags, cls="units", power=p) for p in eval_np.UNIT_POWERS]
        assert all(len(i) == 1 for i in u)
        for i, p in zip(u, eval_np.UNIT_POWERS):                                        # the same numbers times 2^p, exactly
            assert np.array_equal(S1[i], S1[u[1]] * np.float32(2.0 ** p)) and np.array_equal(S2[i], S2[u[1]] * np.float32(2.0 ** p))
        b = eval_np.tag_index(tags, cls="bulk")
        bulk += len(b)
        if M not in (14, 17):
            assert {t["cls"] for t in tags} == {"group", "exact", "units"}
            continue
        assert abs(3 * len(eval_np.tag_index(tags, cls="bulk", mirrored=True)) - len(b)) <= 2                      # a third mirrored
        ang = np.array([tags[i]["angle"] for i in b])
        assert ang.min() < 0.05 and ang.max() > np.pi - 0.05 and np.all(ang <= np.pi)
        for i in eval_np.tag_index(tags, cls="planar"):                                # one coordinate constant: K has rank 2
            assert (S2[i] == S2[i][0]).all(0).sum() == 1
            s = np.linalg.svd(eval_np.procrustes_parts(S1[i], S2[i])[4], compute_uv=False)
            assert s[2] <= 1e-14 * s[0] and s[1] > 0.05 * s[0]
        assert {(t["mirrored"], t["noise"]) for t in tags if t["cls"] == "planar"} == {(m, z) for m in (False, True) for z in (0.0, 0.02)}
        for eps in eval_np.ILL_EPS:
            assert len(eval_np.tag_index(tags, cls="ill", eps=eps)) == eval_np.ILL_SETS >= 24
    assert bulk == eval_np.BULK_SETS == 2000


def test_solver_cases_conditioning_determinants_and_half_turns(solver):
    """Every ill-conditioned bucket has the conditioning its construction sets (within a factor 2 of 0.16 eps; eps = 0: below 1e-7),
    every other class is far from it, mirrored full-rank cases have det(U V^T) < 0 and the others > 0, and each class built without
    noise holds a half-turn: |qw| < 1e-6 for the float64 optimal quaternion.  (The bulk and the units class carry 0.02 noise by
    definition, which moves the optimum ~1e-2 rad off any exact angle.)"""
    for M, c in solver.items():
        tags, cond, det = c["tags"], c["cond"], c["det"]
        ill = eval_np.tag_index(tags, cls="ill")
        well = np.setdiff1d(np.arange(len(tags)), ill)
        assert cond[well].min() > 1e-3
        m = _full_rank_mirrored(c)
        assert np.all(det[m] < 0)
        if M >= 4:
            rest = np.array([i for i in well if not tags[i]["mirrored"] and tags[i]["cls"] != "planar"])
            assert np.all(det[rest] > 0)
        for eps in eval_np.ILL_EPS:
            i = eval_np.tag_index(tags, cls="ill", eps=eps)
            if not len(i):
                continue
            print(f"M={M} eps={eps:g}: conditioning {cond[i].min():.3e} .. {cond[i].max():.3e}")
            if eps == 0.0:
                assert cond[i].max() < 1e-7
            else:
                assert 0.08 * eps <= cond[i].min() and cond[i].max() <= 0.32 * eps
        for cls in ("group", "planar", "ill"):
            i = eval_np.tag_index(tags, cls=cls, rot="rand_pi")
            if cls == "group" or len(i):
                # the optimum is the case's own rotation where the data are its exact image: no noise, and not mirrored - except in
                # the ill class, whose mirror is along a principal axis of the ground truth and leaves R^T the optimum (up to the
                # data's float32 rounding over the conditioning: at least one case, not every bucket)
                qw = [eval_np.optimal_qw(c["S1"][k], c["S2"][k]) for k in i
                      if tags[k]["noise"] == 0.0 and (cls == "ill" or not tags[k]["mirrored"])]
                assert len(qw) >= 1 and min(qw) < 1e-6, (M, cls, qw)
        for name in ("pi_x", "pi_y", "pi_z", "pi_111"):
            i = eval_np.tag_index(tags, cls="group", rot=name, noise=0.0, mirrored=False)
            assert len(i) == 2 and max(eval_np.optimal_qw(c["S1"][k], c["S2"][k]) for k in i) < 1e-6


def test_exact_cases_skip_every_rotation_of_the_optimal_row(solver):
    """The exact class, not mirrored: Horn's matrix has exact zeros beside the diagonal entry of the optimal quaternion's row, which is
    the largest - row 0 for the aligned pair, row 1, 2, 3 for the half-turn about x, y, z - so the device's route skips those
    rotations, picks a unit vector (qw = 1 or exactly 0) and returns PA = 0 exactly."""
    row = {"exact_identity": 0, "exact_pi_x": 1, "exact_pi_y": 2, "exact_pi_z": 3}
    for M, c in solver.items():
        assert len(eval_np.tag_index(c["tags"], cls="exact")) == 16
        i = eval_np.tag_index(c["tags"], cls="exact", mirrored=False)
        X1, X2 = c["y64"]["pred_jnts3D"][i], c["S2"][i].astype(np.float64)
        K = np.einsum("nmr,nmc->nrc", X1 - X1.mean(1, keepdims=True), X2 - X2.mean(1, keepdims=True))
        N = eval_np._horn_matrix(K)
        for n, k in enumerate(i):
            r = row[c["tags"][k]["rot"]]
            assert np.count_nonzero(N[n, r]) == 1 and np.argmax(np.diag(N[n])) == r and np.count_nonzero(N[n]) > 4
        assert np.all(eval_np.pampjpe_jacobi(X1, X2) == 0.0)
        # the half-turns need the pick: column 0 ends as whichever eigenvector the rotations' path leaves there, seldom the optimal one
        assert (eval_np.pampjpe_jacobi(X1, X2, pick="first")[2:].max(1) > 0.01).sum() >= 4


def test_solver_cases_are_not_vacuous(gold, solver):
    """A kernel that skips the alignment fails every rotated case of the group sweep, and one that skips the reflection fix fails
    every mirrored case it can matter for: both move the mean PA by >= 100 x the tolerance of tests/test_eval_solver_gpu.py."""
    tol = min(8.0 * float(gold["d_ref_pampjpe"]), 1e-3)
    for M, c in solver.items():
        tags, y = c["tags"], c["y64"]
        moved = np.array([i for i in eval_np.tag_index(tags, cls="group") if tags[i]["rot"] != "identity"])
        assert len(moved) == 88 and (y["mpjpe_mean"][moved] - y["pampjpe_mean"][moved]).min() >= 100 * tol
        m = _full_rank_mirrored(c)
        if M >= 4:
            assert len(m) >= 48
            nofix = eval_np.evaluate(**{k: (v[m] if isinstance(v, np.ndarray) and k not in ("J_regressor",) else v) for k, v in c["kw"].items()},
                                     dtype=np.float64, sign_fix=False)["pampjpe"]
            assert np.abs(nofix - y["pampjpe"][m]).mean(-1).min() >= 100 * tol


def test_pa_residual_invariant(solver):
    """var2 - (sigma1 + sigma2 + d sigma3)^2 / var1 == sum_j PA_j^2 of the float64 SVD route, to 1e-12 of var2 (the invariant is a
    difference from var2 and 0 for an exact fit, so var2 is the scale its rounding is relative to) on the well-conditioned classes;
    and it is the pelvis-free quantity: the same from the raw joint sets and from the device's pelvis-relative ones."""
    for M, c in solver.items():
        well = np.array([i for i, t in enumerate(c["tags"]) if t["cls"] != "ill"])
        inv = eval_np.pa_residual_invariant(c["S1"][well], c["S2"][well])
        var2 = ((c["S2"][well].astype(np.float64) - c["S2"][well].astype(np.float64).mean(1, keepdims=True)) ** 2).sum((1, 2))
        got = (c["y64"]["pampjpe"][well] ** 2).sum(1)
        print(f"M={M}: max |sum PA^2 - invariant| / var2 = {(np.abs(got - inv) / var2).max():.3e}")
        assert np.all(np.abs(got - inv) <= 1e-12 * var2)
        rel = eval_np.pa_residual_invariant(c["y64"]["pred_jnts3D"][well], c["S2"][well])
        assert np.all(np.abs(rel - inv) <= 1e-12 * var2)


def test_device_route_in_numpy_and_the_breaks_the_cases_catch(gold, inp, solver):
    """eval_np.pampjpe_jacobi restates the device's route (Horn's 4x4, 10 cyclic Jacobi sweeps from E = I, the largest diagonal entry's
    column).  It agrees with the SVD route to 64 eps x the data's scale / conditioning wherever the conditioning is >= 1e-6 (both are
    backward stable in float64; the rotation's sensitivity is the reciprocal of the eigenvalue gap).  Broken on purpose - 3 sweeps, the
    wrong sign in N[1][3], the first column instead of the largest diagonal's - it leaves the tolerance on the solver cases; the
    3-sweep one stays inside it on the 0.6 rad fixture crops, which is why those alone do not pin the sweep count."""
    tol = min(8.0 * float(gold["d_ref_pampjpe"]), 1e-3)
    caught = {"sweeps": 0, "n13_sign": 0, "pick": 0}
    for M, c in solver.items():
        ok = np.nonzero(c["cond"] >= 1e-6)[0]
        scale = np.array([2.0 ** c["tags"][i]["power"] for i in ok])
        want = c["y64"]["pampjpe"][ok]
        S1, S2 = c["y64"]["pred_jnts3D"][ok], c["S2"][ok]
        d = np.abs(eval_np.pampjpe_jacobi(S1, S2) - want).max(1)
        print(f"M={M}: Jacobi route vs SVD route {d.max():.3e} (largest share of its bound {(d * c['cond'][ok] / (64 * 2.3e-16 * scale)).max():.3f})")
        assert np.all(d <= 64 * 2.3e-16 * scale / c["cond"][ok])
        for k, kw in (("sweeps", dict(sweeps=3)), ("n13_sign", dict(n13_sign=-1.0)), ("pick", dict(pick="first"))):
            caught[k] += int((np.abs(eval_np.pampjpe_jacobi(S1, S2, **kw) - want).max(1) > tol * scale).sum())
    print(f"cases a broken solver fails: {caught}")
    assert min(caught.values()) >= 100
    worst = 0.0
    for form, name in eval_np.FIXTURE_COMBOS:
        y = eval_np.evaluate(**eval_np.fixture_case(inp, form, name), dtype=np.float64)
        worst = max(worst, np.abs(eval_np.pampjpe_jacobi(y["pred_jnts3D"], y["gt_jnts3D"], sweeps=3) - y["pampjpe"]).max())
    print(f"3 sweeps on the fixture crops: {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol


def test_slicing_cases_hold_the_slice_borders():
    cases = eval_np.slicing_cases(meshes=False)
    again = eval_np.slicing_cases(meshes=False)
    assert sorted(cases) == [1024, 1025, 2048, 17409]
    assert eval_np.slice_borders(1025) == [0, 1023, 1024] and eval_np.slice_borders(2048) == [0, 1023, 1024, 2047]
    for V, c in cases.items():
        Jr = c["J_regressor"]
        J = Jr.shape[0]
        assert Jr.dtype == np.float32 and Jr.shape == ((32, V) if V < 17409 else (5, V)) and np.array_equal(Jr, again[V]["J_regressor"])
        assert c["jmap"] == again[V]["jmap"] and len(set(c["jmap"])) == len(c["jmap"]) == (32 if V < 17409 else 3)
        assert c["pelvis"] not in (c["zero_row"], c["last_only"]) and c["last_only"] in c["jmap"]
        borders, last = eval_np.slice_borders(V), eval_np.SLICE * ((V - 1) // eval_np.SLICE)
        for j in range(J):
            if j == c["zero_row"]:
                assert not Jr[j].any()
            elif j == c["last_only"]:
                assert not Jr[j, :last].any() and all(Jr[j, v] != 0 for v in borders if v >= last)
            else:
                assert all(Jr[j, v] != 0 for v in borders) and (Jr[j] != 0).sum() > len(borders)
        if V < 17409:
            assert c["zero_row"] in c["jmap"]
    small = eval_np.slicing_cases(only=(1025,))[1025]
    assert small["pred_vertices"].shape == small["gt_vertices"].shape == (5, 1025, 3) and small["pred_vertices"].dtype == np.float32
    assert np.abs(small["gt_vertices"]).max() <= 0.5 and 0.01 < np.abs(small["pred_vertices"] - small["gt_vertices"]).std() < 0.03


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
