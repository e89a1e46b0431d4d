"""GPU: the rotation solver of csrc/eval_metrics.hip (eval_crop: Horn's 4x4, 10 cyclic Jacobi sweeps) and the slice / sub-batch edges
of eval_partial, eval_crop and eval_finish off the fixture - tests/eval_np.solver_cases() and slicing_cases() against tests/eval_np.py
in float64 (the SVD route).  The solver gets joints the test controls exactly: a J-vertex "mesh" under the identity regressor and joint
ground truth (eval_np.solver_inputs).  Tolerance per quantity as in tests/test_eval_gpu.py: 8 x d_ref of tests/golden/eval.npz, times the
data's power-of-two scale in the units class; where the rotation itself is ill conditioned, the residual invariant instead."""
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import evaluate
from tests import eval_np

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "eval.npz"
QUANTITY = {"pampjpe": "pampjpe", "pampjpe_mean": "pampjpe", "mpjpe": "mpjpe", "mpjpe_mean": "mpjpe", "pred_jnts3D": "joints",
            "gt_jnts3D": "joints", "pred_jnts3D_nonrel": "joints"}
MESH_QUANTITY = dict(QUANTITY, v2v="v2v", corr_x="corr_x")
WELL = 1e-6                                 # conditioning from which the rotation, and so each joint's PA, is compared


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def tol(gold, q):
    return min(8.0 * float(gold["d_ref_" + q]), 1e-3)


def step_all(cuda, kw, splits=None):
    """The crops of the evaluate() arguments `kw` through one Evaluator in steps of `splits` (default: one step) -> finish()."""
    n = len(kw["pred_vertices"])
    dev = {k: torch.from_numpy(np.ascontiguousarray(kw[k])).to(cuda) for k in ("pred_vertices", "pred_pose", "var_pose", "gt_pose")}
    form = "gt_vertices" if kw.get("gt_vertices") is not None else "gt_joints"
    gt = torch.from_numpy(np.ascontiguousarray(kw[form])).to(cuda)
    ev = evaluate.Evaluator(kw["J_regressor"], kw["jmap"], capacity=n, pelvis=kw["pelvis"], device=cuda)
    lo = 0
    for b in (splits or [n]):
        sl = slice(lo, lo + b)
        ev.step({"smpl_vertices": dev["pred_vertices"][sl], "pred_pose": dev["pred_pose"][sl], "var_pose": dev["var_pose"][sl]},
                dev["gt_pose"][sl], **{form: gt[sl]})
        lo += b
    assert lo == n
    res = ev.finish(return_records=True)
    ev.close()
    return res


@pytest.fixture(scope="module")
def solver(cuda):
    """Per joint count M: the cases, their float64 conditioning, the float64 SVD route and - ONE step of all the cases of that M -
    the device's records.  Made on first use, shared by every test below, never changed."""
    cases, memo = eval_np.solver_cases(), {}

    def get(M):
        if M not in memo:
            S1, S2, tags = cases[M]
            kw = eval_np.solver_inputs(M, S1, S2)
            memo[M] = dict(S1=S1, S2=S2, tags=tags, kw=kw, cond=np.array([eval_np.conditioning(a, g)[0] for a, g in zip(S1, S2)]),
                           y64=eval_np.evaluate(**kw, dtype=np.float64), rec=step_all(cuda, kw)["records"])
        return memo[M]
    return get


def sub_kw(kw, idx):
    """The evaluate() arguments restricted to the crops idx."""
    return {k: (v[idx] if isinstance(v, np.ndarray) and k != "J_regressor" else v) for k, v in kw.items()}


@pytest.mark.parametrize("M", eval_np.SOLVER_JOINTS)
def test_solver_matches_float64(cuda, gold, solver, M):
    """Per-joint and mean PA, per-joint and mean MPJPE and the three joint sets of every case whose conditioning is >= 1e-6 - the group
    sweep (half-turns, aligned pairs, 2 pi / 3, angles up to pi, both scales, mirrored), the exact pairs, the 2000 random sets, planar ground truth,
    mm / m / km-like units and the ill-conditioned buckets down to eps = 1e-4 - against the SVD route in float64."""
    c = solver(M)
    got = eval_np.unpack(c["rec"], M)
    assert len(c["rec"]) == len(c["tags"])
    for cls in ("group", "exact", "bulk", "planar", "units", "ill"):
        i = eval_np.tag_index(c["tags"], cls=cls)
        i = i[c["cond"][i] >= WELL] if len(i) else i
        if not len(i):
            assert M not in (14, 17)
            continue
        assert cls != "ill" or len(i) == 4 * eval_np.ILL_SETS                   # eps = 1e-1 .. 1e-4
        scale = np.array([2.0 ** c["tags"][k]["power"] for k in i])
        line = []
        for k, q in QUANTITY.items():
            d = np.abs(got[k][i].astype(np.float64) - c["y64"][k][i]).reshape(len(i), -1).max(1) / scale
            line.append(f"{k} {d.max():.2e}")
            assert d.max() <= tol(gold, q), (M, cls, k, d.max(), tol(gold, q), c["tags"][i[d.argmax()]])
        print(f"M={M} {cls} ({len(i)} cases): " + ", ".join(line))
    assert np.all(c["rec"][:, eval_np.R_PA_J + M:eval_np.R_POSE] == 0) and np.all(c["rec"][:, eval_np.R_V2V] == 0)


@pytest.mark.parametrize("M", eval_np.SOLVER_JOINTS)
def test_exact_pairs_align_to_zero(solver, M):
    """An exactly aligned pair and exact half-turns about x, y and z, every sum exact in fp64: the off-diagonal entries of the optimal
    quaternion's row of Horn's matrix are exactly 0, so jacobi_rotate takes its `apq == 0` branch for all of them, the quaternion is
    the unit vector of the largest diagonal entry (column 0, or 1, 2, 3 with qw = 0) and every PA value is exactly 0
    (tests/test_eval_cpu.py shows the same of the route restated in numpy).  Mirrored, the PA is that of the SVD route (above)."""
    c = solver(M)
    i = eval_np.tag_index(c["tags"], cls="exact", mirrored=False)
    assert len(i) == 8 and {c["tags"][k]["rot"] for k in i} == {"exact_identity", "exact_pi_x", "exact_pi_y", "exact_pi_z"}
    assert np.all(c["rec"][i, eval_np.R_PA_J:eval_np.R_PA_J + M] == 0.0) and np.all(c["rec"][i, eval_np.R_PA] == 0.0)
    assert c["rec"][i, eval_np.R_MPJPE].min() > 0.1


@pytest.mark.parametrize("M", eval_np.SOLVER_JOINTS)
def test_units_scale_bit_for_bit(solver, M):
    """The same joints times 2^-10 and 2^10: every step from the joints to the PA values is exact under a power-of-two scaling in
    fp64 (sums, the Jacobi angles are ratios, square roots of even powers) and the fp32 results stay normal, so the records are the
    scale-1 records times that power of two, bit for bit."""
    c = solver(M)
    base = c["rec"][eval_np.tag_index(c["tags"], cls="units", power=0)]
    fields = [(eval_np.R_MPJPE, 2), (eval_np.R_MPJPE_J, 64), (eval_np.R_PRED, 288)]       # means; per joint; the three joint sets
    for p in (-10, 10):
        rec = c["rec"][eval_np.tag_index(c["tags"], cls="units", power=p)]
        for o, w in fields:
            want = base[:, o:o + w] * np.float32(2.0 ** p)
            assert np.all((want == 0) | (np.abs(want) >= np.finfo(np.float32).tiny)) and np.isfinite(want).all()
            assert np.array_equal(rec[:, o:o + w], want), (M, p, o)
    assert base[0, eval_np.R_PA] > 0.005 and np.count_nonzero(base[:, eval_np.R_PRED:eval_np.R_PRED + 288]) >= 9 * M - 3


@pytest.mark.parametrize("M", [14, 17])
def test_ill_conditioned_residual_invariant(solver, M):
    """sigma2 -> sigma3 with a mirrored prediction: the two largest eigenvalues of Horn's matrix meet and the rotation is ill
    defined (at eps = 0: not defined), but sum_j PA_j^2 is the same for every maximiser.  Each PA_j is one fp32 rounding (2^-24
    relative) of an fp64 value, so the sum of squares carries <= 2^-23; 8 x that is allowed.  PA stays ~0.08 m here: nothing cancels."""
    c = solver(M)
    for eps in eval_np.ILL_EPS:
        i = eval_np.tag_index(c["tags"], cls="ill", eps=eps)
        assert len(i) == eval_np.ILL_SETS
        pa = c["rec"][i, eval_np.R_PA_J:eval_np.R_PA_J + M].astype(np.float64)
        assert np.isfinite(c["rec"][i]).all()
        inv = eval_np.pa_residual_invariant(c["S1"][i], c["S2"][i])
        rel = np.abs((pa ** 2).sum(1) - inv) / inv
        print(f"M={M} eps={eps:g} (conditioning {c['cond'][i].min():.1e} .. {c['cond'][i].max():.1e}): "
              f"|sum PA^2 - invariant| / invariant {rel.max():.2e} (bound {2.0 ** -20:.2e}), mean PA {pa.mean():.3f} m")
        assert inv.min() > 1e-3 and rel.max() <= 2.0 ** -20, (eps, rel.max())
        assert np.abs(c["rec"][i, eval_np.R_PA] - pa.mean(1)).max() <= 1e-7


def test_bulk_is_independent_of_batching(cuda, solver):
    """The 2000 random sets (1000 of 14 joints, then 1000 of 17) in one step per joint count, and the same sequence cut into steps of
    [1, 255, 256, 257, 1231] - the last 1000 of them, one step again, also as [231, 257, 256, 255, 1]: identical records.  256 crops
    is one launch pair, so the cuts fall before, on and behind its border and the 769-crop remainder of M = 14 loops over four."""
    for M, splits in ((14, [1, 255, 256, 257, 231]), (17, [1000]), (17, [231, 257, 256, 255, 1])):
        c = solver(M)
        i = eval_np.tag_index(c["tags"], cls="bulk")
        assert len(i) == 1000 and sum(splits) == 1000
        kw = sub_kw(c["kw"], i)
        assert np.array_equal(step_all(cuda, kw, splits)["records"], c["rec"][i]), (M, splits)


def _poses(n, seed):
    r = np.random.default_rng(seed)
    pose = r.uniform(-1, 1, (n, 72)).astype(np.float32)
    pp = eval_np.rodrigues(pose.reshape(-1, 3) + 0.1, np.float64).reshape(n, 24, 3, 3).astype(np.float32)
    return dict(gt_pose=pose, pred_pose=pp, var_pose=r.uniform(0, 1, (n, 24)).astype(np.float32))


def _mesh_kw(V):
    c = eval_np.slicing_cases(only=(V,))[V]
    return dict(pred_vertices=c["pred_vertices"], gt_vertices=c["gt_vertices"], J_regressor=c["J_regressor"], jmap=c["jmap"],
                pelvis=c["pelvis"], **_poses(c["B"], V))


def _assert_matches_float64(gold, kw, rec, label):
    M = len(kw["jmap"])
    got = eval_np.unpack(rec, M)
    y64 = eval_np.evaluate(**kw, dtype=np.float64)
    line = []
    for k, q in MESH_QUANTITY.items():
        d = np.abs(got[k].astype(np.float64) - y64[k]).max()
        line.append(f"{k} {d:.2e}")
        assert d <= tol(gold, q), (label, k, d, tol(gold, q))
    print(f"{label}: " + ", ".join(line))


@pytest.mark.parametrize("V", [1024, 1025, 2048])
def test_slice_borders(cuda, gold, V):
    """One full slice, a second slice that holds ONE vertex, two full slices; 32 regressor rows through a shuffled 32-entry map, each
    with an entry in the first and the last column of every slice, one row in the last slice alone, one row without an entry."""
    kw = _mesh_kw(V)
    _assert_matches_float64(gold, kw, step_all(cuda, kw)["records"], f"V={V}")


def test_eighteen_slices_and_a_sub_batch_of_227(cuda, gold):
    """V = 17409: 18 slices (the last one a single vertex), so a launch pair takes 4096 // 18 = 227 crops and a step of 230 is the
    first configuration that loops over sub-batches of another size than 256.  Against float64, and bitwise against the same crops
    stepped as [227, 3] and [3, 227]."""
    kw = _mesh_kw(17409)
    assert len(kw["pred_vertices"]) == 230 and kw["J_regressor"].shape == (5, 17409)
    rec = step_all(cuda, kw)["records"]
    _assert_matches_float64(gold, kw, rec, "V=17409 B=230")
    for splits in ([227, 3], [3, 227]):
        assert np.array_equal(step_all(cuda, kw, splits)["records"], rec), splits


def test_finish_over_one_record_more_than_its_block(cuda, solver):
    """eval_finish is one block of 1024 threads: 1025 records give thread 0 a second one.  The summary against eval_np.summary of the
    records, to the bounds of test_finish_summary_reset_and_capacity."""
    c = solver(17)
    kw = dict(sub_kw(c["kw"], np.arange(1025)), **_poses(1025, 3))
    res = step_all(cuda, kw, [512, 513])
    n, mp, pa, vv, corr = eval_np.summary(res["records"])
    assert res["N"] == n == 1025 and res["val_v2v"] == vv == 0.0
    for got, want in ((res["val_mpjpe"], mp), (res["val_pampjpe"], pa)):
        assert want > 1.0 and abs(got - want) <= 1e-12 * abs(want)
    assert np.isfinite(corr) and abs(res["val_corr"] - corr) <= 1e-9
    m = eval_np.R_POSE                       # the solver fields do not depend on the poses: the records of the shared step again
    assert np.array_equal(res["records"][:, :m], c["rec"][:1025, :m])
