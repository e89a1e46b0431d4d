"""CPU: the keypoint refit's contract (tests/refit_np.py restates DESIGN.md section 31) and its host side (poco_amd/refit.py): the
analytic Jacobian against central finite differences, the restatement's invariants, the joint tables against the body model, the
flag errors and the symbol's presence in the built library."""
import argparse

import numpy as np

from poco_amd import _lib, refit, synth
from tests import refit_np as rn


def _good_row(i=1):
    d = rn.gpu_case(N=8)
    return {k: v[i] for k, v in d.items()}


def test_analytic_jacobian_matches_central_differences():
    """d r / d (delta, kappa, dtx, dty) at a point away from the network's pose.  Central differences with h = 1e-6 carry a
    truncation error of h^2 |r'''| / 6 ~ 1e-12 and a rounding error of eps |r| / h ~ 1e-10 for residuals of order one: 1e-8
    leaves two digits of room.  The formula -[p_k - p_j]x G_j uses G (d x v) = (G d) x (G v), which holds for rotations: the
    matrices are made orthonormal in float64 first.  With the network's fp32 matrices as they come (orthonormal to 6e-8) the same
    comparison shows 1.5e-8, whatever the step: the third approximation of DESIGN.md section 31, which moves no fixed point."""
    r = np.random.default_rng(3)
    d = _good_row()
    row = rn.Row(d["pose"], d["u"], d["jrest"], d["kp"], d["cam"], d["norm"], rn.BODY25_TO_SMPL, rn.SMPL_PARENTS, 0.1, 0.3, 0.1, 1.0, 0.3, np.float64)
    U, _, Vt = np.linalg.svd(row.Rnet)
    row.Rnet = U @ Vt                                      # see below: the formula is exact for orthonormal matrices
    R = np.stack([row.Rnet[j] @ rn.exp_so3(0.2 * r.standard_normal(3)) for j in range(24)])
    x = np.array([0.1, -0.05, 0.03])
    J = row.jacobian(row.evaluate(R, x))
    assert np.abs(J).max() > 0.1 and (np.abs(J).sum((0, 1)) > 0).sum() > 30
    h = 1e-6

    def res(step):
        Rs = np.stack([R[j] @ rn.exp_so3(step[3 * j:3 * j + 3]) for j in range(24)])
        return row.evaluate(Rs, x + step[72:])["r"]
    num = np.zeros_like(J)
    for i in range(rn.NU):
        e = np.zeros(rn.NU)
        e[i] = h
        num[:, :, i] = (res(e) - res(-e)) / (2 * h)
    assert np.abs(J - num).max() < 1e-8, np.abs(J - num).max()
    # a joint's own rotation does not move it: MidHip (joint 0) has no rotation column at all, the wrist none of its own
    assert not J[8, :, :72].any() and not J[4, :, 3 * 21:3 * 22].any() and J[4, :, 3 * 19:3 * 20].any()


def test_prior_jacobian_is_the_identity_to_first_order():
    """q(R exp(d)) - q(R) = d + O(|q| |d|): the approximation the contract states."""
    r = np.random.default_rng(4)
    Rn = rn.rot_axis(r.standard_normal(3), 0.7)
    q0 = 0.05 * r.standard_normal(3)
    R = Rn @ rn.exp_so3(q0)
    for i in range(3):
        e = np.zeros(3)
        e[i] = 1e-6
        dq = (rn.log_so3(Rn.T @ R @ rn.exp_so3(e)) - rn.log_so3(Rn.T @ R @ rn.exp_so3(-e))) / 2e-6
        assert np.abs(dq - np.eye(3)[i]).max() < np.linalg.norm(q0)


def test_cost_never_increases_and_skipped_rows_copy_through():
    d = rn.gpu_case(N=8)
    for rho in (0.1, 0.0):
        trace = []
        out = [rn.refit_row(d["pose"][i], d["u"][i], d["jrest"][i], d["kp"][i], d["cam"][i], d["norm"][i], rho=rho, trace=trace) for i in range(8)]
        assert [o["flag"] for o in out] == [1, 0, 0, 1, 0, 2, 0, 0]
        for o in out:
            assert o["cost"][1] <= o["cost"][0]
            if o["flag"] == 0:
                assert o["accepted"] >= 1 and o["cost"][1] < o["cost"][0]
        assert any(t < f for f, t in trace) and any(not t < f for f, t in trace)     # both branches of the accept rule are taken
    for i in (3, 5):
        o = rn.refit_row(d["pose"][i], d["u"][i], d["jrest"][i], d["kp"][i], d["cam"][i], d["norm"][i])
        assert np.array_equal(o["pose"].astype(np.float32).view(np.uint32), d["pose"][i].view(np.uint32))
        assert np.array_equal(o["cam"].astype(np.float32), d["cam"][i, :3]) and not o["shift"].any() and not o["cost"].any()


def test_all_zero_confidences_copy_through_with_flag_1():
    d = _good_row()
    kp = d["kp"].copy()
    kp[:, 2] = 0.0
    o = rn.refit_row(d["pose"], d["u"], d["jrest"], kp, d["cam"], d["norm"])
    assert o["flag"] == 1 and o["accepted"] == 0 and np.array_equal(o["pose"].astype(np.float32), d["pose"])


def test_a_row_that_fits_its_keypoints_stays_put():
    """Keypoints that are the row's own projection, handed to the restatement unrounded (float64): every residual is exactly zero
    - the projection and the residual are the same operations in the same order - so F = 0, the gradient is zero, the step is
    zero, no trial point is lower: cost 0, shift 0 (the issue's bound: below 1e-6 degrees), nothing accepted.
    Rounded to fp32 pixels the same keypoints are off by up to 2^-24 x 400 px / 120 px of box = 2e-7 of the box: the cost is
    5e-13, not 0, the fit accepts steps and the doubtful joints turn by up to 4.3e-4 degrees towards the rounded pixels.  The
    invariant as the issue words it holds for exact keypoints only (NOTEBOOK.md); the second half pins the
    rounded case to what that rounding explains: a turn of 2e-7 of the box over a bone of 0.1 of the box is 2e-6 rad = 1.1e-4
    degrees per keypoint, a few of them add up along a limb, 1e-3 degrees bounds it."""
    d = _good_row()
    kp = np.zeros((25, 3))
    kp[:, :2] = rn.project(d["pose"], d["jrest"], d["cam"].astype(np.float64))
    kp[:, 2] = 1.0
    for rho in (0.1, 0.0):
        o = rn.refit_row(d["pose"], d["u"], d["jrest"], kp, d["cam"], d["norm"], rho=rho)
        assert o["flag"] == 0 and o["accepted"] == 0
        assert o["cost"][0] == 0.0 and o["cost"][1] == 0.0 and o["shift"].max() < 1e-6
        assert np.array_equal(o["pose"].astype(np.float32).view(np.uint32), d["pose"].view(np.uint32))
    o = rn.refit_row(d["pose"], d["u"], d["jrest"], kp.astype(np.float32), d["cam"], d["norm"], rho=0.0)
    assert o["flag"] == 0 and 0.0 < o["cost"][0] < 14 * (2.0 ** -24 * 400 / 120) ** 2 * 2 and o["cost"][1] <= o["cost"][0]
    assert o["shift"].max() < 1e-3


def test_float64_and_longdouble_differ_by_no_more_than_the_gpu_tests_table():
    """tests/test_refit_gpu.py's tolerance is 100 x D_LD, the restatement's own float64 / longdouble difference on gpu_case.  The
    table is re-derived here (ten steps, where the accept decisions diverge, on every row; one step likewise), so a change to the
    material or to the restatement cannot leave it stale."""
    from tests.test_refit_gpu import D_LD
    d = rn.gpu_case()
    for iters in (1, 10):
        for rho in (0.1, 0.0):
            a, b = rn.refit(**d, rho=rho, iters=iters), rn.refit(**d, rho=rho, iters=iters, ft=np.longdouble)
            assert np.array_equal(a["info"][:, 1], b["info"][:, 1])
            ok = a["info"][:, 1] == 0
            for k in ("pose", "cam", "shift", "cost"):
                diff = np.abs(a[k + "64"][ok].astype(np.longdouble) - b[k + "64"][ok])
                if k == "cam":
                    diff = diff / np.maximum(np.abs(b[k + "64"][ok]), 1)
                assert float(diff.max()) <= D_LD[iters][k], (iters, rho, k, float(diff.max()))


def test_joint_tables_are_the_regressed_rest_joints():
    smpl = synth.synth_smpl(7)
    Jt, Jd, parents = refit.joint_tables(smpl)
    assert Jt.shape == (24, 3) and Jd.shape == (24, 3, 10) and Jt.dtype == np.float64
    assert np.array_equal(parents, rn.SMPL_PARENTS)
    r = np.random.default_rng(5)
    Jr, vt, sd = (np.asarray(smpl[k], np.float64) for k in ("J_regressor", "v_template", "shapedirs"))
    for _ in range(3):
        beta = r.standard_normal(10)
        want = Jr @ (vt + sd[:, :, :10] @ beta)
        assert np.abs(Jt + Jd @ beta - want).max() < 1e-12
    import torch
    betas = torch.from_numpy(r.standard_normal((4, 10)).astype(np.float32))
    got = refit.rest_joints((Jt, Jd, parents), betas).numpy()
    want = np.stack([Jr @ (vt + sd[:, :, :10] @ b.astype(np.float64)) for b in betas.numpy()])
    assert np.abs(got - want).max() < 1e-5                 # one fp32 matmul of 11 terms of order one
    assert np.array_equal(refit.BODY25_TO_SMPL, rn.BODY25_TO_SMPL) and (refit.BODY25_TO_SMPL >= 0).sum() == 14


def _args(**kw):
    base = dict(kp_refit=None, kp_refit_ref=0.3, kp_refit_rho=0.1, kp_refit_iters=10, mode="video", gpus=1, cfg2=None, ckpt2=None)
    return argparse.Namespace(**{**base, **kw})


def test_flag_errors_are_one_sentence():
    assert refit.flag_error(_args(), "demo") is None and refit.flag_error(_args(kp_refit=0.1), "demo") is None
    assert refit.flag_error(_args(kp_refit=0.1), "eval") is None
    bad = [(_args(kp_refit_rho=0.2), "demo"), (_args(kp_refit=0.0), "demo"), (_args(kp_refit=float("nan")), "demo"),
           (_args(kp_refit=0.1, kp_refit_ref=0.0), "demo"), (_args(kp_refit=0.1, kp_refit_iters=0), "demo"),
           (_args(kp_refit=0.1, kp_refit_iters=33), "eval"), (_args(kp_refit=0.1, kp_refit_rho=float("inf")), "demo"),
           (_args(kp_refit=0.1, mode="folder"), "demo"), (_args(kp_refit=0.1, mode="directory"), "demo"), (_args(kp_refit=0.1, mode="webcam"), "demo"),
           (_args(kp_refit=0.1, cfg2="x.yaml"), "demo"), (_args(kp_refit=0.1, cfg2="x.yaml"), "eval"), (_args(kp_refit=0.1, gpus=2), "demo")]
    bad += [(_args(kp_refit=0.1, **{f: v}), "eval") for f, v in (("tta", "flip"), ("segm", True), ("likelihood", True), ("sequences", True),
                                                                 ("rank_metrics", True), ("visibility", True), ("aug_rot", 10.0), ("aug_scale", 0.1),
                                                                 ("aug_flip", True), ("aug_noise", 0.1), ("aug_occlude", 0.3), ("augment", True))]
    for a, prog in bad:
        msg = refit.flag_error(a, prog)
        assert isinstance(msg, str) and "kp_refit" in msg and "\n" not in msg and msg.count(". ") == 0, (a, msg)
    j25 = np.zeros((5, 25, 3))
    assert refit.tracking_error({"0": {"joints2d": j25, "bbox": np.zeros((5, 4))}}) is None
    for tr in (None, {}, {"0": {"bbox": np.zeros((5, 4))}}, {"0": {"joints2d": j25}, "1": {"joints2d": np.zeros((5, 17, 3))}}):
        msg = refit.tracking_error(tr)
        assert isinstance(msg, str) and "kp_refit" in msg and msg.count(". ") == 0


def test_demo_refuses_the_flag_before_the_engine(tmp_path):
    import pytest

    import demo
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt", "--vid_file", str(tmp_path)]
    for flags, word in ((["--mode", "folder", "--kp_refit", "0.1"], "folder"), (["--mode", "video", "--kp_refit_iters", "5"], "need --kp_refit"),
                        (["--mode", "video", "--kp_refit", "0.1", "--gpus", "2"], "--gpus"),
                        (["--mode", "video", "--kp_refit", "0.1"], "joints2d")):          # no --tracking: the default box track has no keypoints
        with pytest.raises(SystemExit) as e:
            demo.main(demo.parse_args(common + flags))
        assert word in str(e.value), (flags, e.value)


def test_the_built_library_exports_the_operator():
    assert "poco_op_kp_refit" in _lib.header_symbols()
    assert hasattr(_lib.lib(), "poco_op_kp_refit")
