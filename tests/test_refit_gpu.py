"""GPU: ops.kp_refit (poco_op_kp_refit, csrc/kp_refit.hip) against its float64 numpy restatement tests/refit_np.py, which builds the
dense Jacobian and normal matrix and solves with numpy.linalg.cholesky where the kernel keeps a packed triangle and factors it
root-free.

Material (refit_np.gpu_case): 65 rows, K = 25 BODY_25 keypoints with confidences either side of the threshold, u from [0.05, 3] with
1e-8, 0.3, 1e4 and inf sprinkled in; rows 3, 19, 35, 51 keep two keypoints (under min_kp = 4; the seeded confidences leave rows 0, 18
and 53 under it too), row 5 has a NaN in its pose, row 37 an infinity in its keypoints, all between good rows.  N = 1 and 2 are rows 1
and 1 .. 2 of the same buffer; rho 0.1 and off; iters 1 and 10.

Tolerance (the issue's rule): 100 x the largest difference the restatement itself shows on these cases between numpy.float64 and
numpy.longdouble, floored at 1e-10, on the float64 value; the output's one rounding to fp32 (2^-24 relative) comes on top.  Measured
on the CPU over rho in {0.1, off} (NOTEBOOK.md, "Keypoint refit"):
    iters  1: pose 7.0e-13, cam 2.1e-16 (relative to max(|value|, 1)), shift 3.0e-11 deg, cost 1.5e-15: the floor governs all but the
              shift (3.0e-9 deg).
    iters 10: pose 1.87e-6, cam 2.6e-11, shift 2.6e-7 deg, cost 1.3e-14.  The two arithmetics take a different accept decision in 5 of
              the 65 rows (a trial point whose cost differs from the current one in the last bits); the rows then differ along the
              directions the keypoints do not see (a turn about a bone's own axis), which is why the pose moves and the cost does
              not.  Tolerance: pose 1.87e-4, cam 2.6e-9, shift 2.6e-5 deg, cost 1e-10.
The accepted-step count is therefore not compared; the flags are."""
import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import refit_np as rn

pytestmark = pytest.mark.gpu

D_LD = {1: dict(pose=7.0e-13, cam=2.1e-16, shift=3.0e-11, cost=1.5e-15), 10: dict(pose=1.87e-6, cam=2.6e-11, shift=2.6e-7, cost=1.3e-14)}
TOL = {it: {k: max(100.0 * v, 1e-10) for k, v in d.items()} for it, d in D_LD.items()}
EPS32 = 2.0 ** -24
KEYS = ("pose", "cam", "shift", "cost")
SKIPPED = {3: 1, 19: 1, 35: 1, 51: 1, 5: 2, 37: 2}
README_LAMBDA = 0.1


@pytest.fixture(scope="module")
def data():
    return rn.gpu_case()


_REF = {}


def _ref(data, rho, iters):
    if (rho, iters) not in _REF:
        _REF[rho, iters] = rn.refit(**data, rho=rho, iters=iters)
    return _REF[rho, iters]


def _run(d, dev, n=None, max_blocks=0, lo=0, **kw):
    """Through outputs poisoned with NaN (info: -7): an element the kernel leaves out fails every comparison."""
    n = len(d["pose"]) if n is None else n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:lo + n])).to(dev)                       # noqa: E731
    out = {"pose": torch.full((n, 24, 3, 3), float("nan"), device=dev), "cam": torch.full((n, 3), float("nan"), device=dev),
           "shift": torch.full((n, 24), float("nan"), device=dev), "cost": torch.full((n, 2), float("nan"), device=dev),
           "info": torch.full((n, 2), -7, device=dev, dtype=torch.int32)}
    args = dict(rn.DEFAULTS, **kw)
    res = ops.kp_refit(t(d["pose"]), t(d["u"]), t(d["jrest"]), t(d["kp"]), t(d["cam"]), t(d["norm"]), rn.BODY25_TO_SMPL, rn.SMPL_PARENTS,
                       out=out, max_blocks=max_blocks, **args)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _compare(got, ref, data, n, iters, what, lo=0):
    figs = {}
    assert np.array_equal(got["info"][:, 1], ref["info"][lo:lo + n, 1]), what
    fit = got["info"][:, 1] == 0
    for i in np.nonzero(~fit)[0]:                          # the designed rows, and those the seeded confidences left under min_kp
        assert got["info"][i, 0] == 0, (what, i)
        assert np.array_equal(_bits(got["pose"][i]), _bits(data["pose"][lo + i])), (what, i)
        assert np.array_equal(_bits(got["cam"][i]), _bits(data["cam"][lo + i, :3])), (what, i)
        assert not got["shift"][i].any() and not got["cost"][i].any()
    for k in KEYS:
        r64 = ref[k + "64"][lo:lo + n][fit].astype(np.float64)
        g = got[k][fit].astype(np.float64)
        assert np.isfinite(g).all(), (what, k)
        scale = np.maximum(np.abs(r64), 1.0) if k == "cam" else 1.0
        bound = TOL[iters][k] * scale + EPS32 * np.abs(r64)
        figs[k] = float((np.abs(g - r64) / bound).max())
    print(f"kp_refit {what}: " + ", ".join(f"{k} {v:.3f} of its bound" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= 1.0, (what, k, v)


@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("rho", [0.1, 0.0])
def test_rows_match_the_restatement(data, rho, iters, cuda):
    ref = _ref(data, rho, iters)
    assert {i: int(ref["info"][i, 1]) for i in SKIPPED} == SKIPPED and int((ref["info"][:, 1] == 0).sum()) >= 50
    assert all((data["u"] == np.float32(v)).sum() >= 10 for v in rn.U_VALUES)       # the material is what the docstring says
    assert ref["shift64"].max() > 5.0 and (ref["cost64"][:, 1] <= ref["cost64"][:, 0]).all()
    whole = _run(data, cuda, 65, rho=rho, iters=iters)
    _compare(whole, ref, data, 65, iters, f"rho={rho:g} iters={iters} N=65")
    for n in (1, 2):                                                                 # rows 1 .. n: row 0 is one of the skipped ones
        got = _run(data, cuda, n, lo=1, rho=rho, iters=iters)
        _compare(got, ref, data, n, iters, f"rho={rho:g} iters={iters} N={n}", lo=1)
        for k in got:                                                                # a row's bits do not depend on the other rows
            assert np.array_equal(_bits(got[k]), _bits(whole[k][1:1 + n])), (k, n)
    # the same call again, and on grids of one and seven blocks: the same bits
    for kw in ({}, {"max_blocks": 1}, {"max_blocks": 7}):
        again = _run(data, cuda, 65, rho=rho, iters=iters, **kw)
        for k in whole:
            assert np.array_equal(_bits(whole[k]), _bits(again[k])), (k, kw)
    R = whole["pose"][whole["info"][:, 1] == 0].astype(np.float64).reshape(-1, 3, 3)
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 4 * EPS32       # rotations to fp32 rounding (tests/test_usmooth_gpu.py)


def test_doubtful_joints_are_recovered_and_confident_ones_stay(cuda):
    """Knees and elbows turned by 25 degrees about the camera axis with var 3.0, everything else exact with var 0.05, keypoints the
    true pose's projection.  What the restatement achieves at the README's LAMBDA = 0.1 on these six rows (NOTEBOOK.md): the turned
    joints end 12.06 degrees nearer the truth on average (from 25.00 to 12.94; the rest of the error is the turn about the bone and
    in depth that a 2-D keypoint does not see), the least gain of a joint is 0.19 degrees, the largest shift of an untouched joint
    is 0.020 degrees, the least of a turned one 2.98 degrees."""
    rc = rn.recovery_case()
    d = {k: v for k, v in rc.items() if k != "truth"}
    ref = rn.refit(**d, lam=README_LAMBDA)
    got = _run(d, cuda, lam=README_LAMBDA)
    assert (got["info"][:, 1] == 0).all()
    assert (got["cost"][:, 1] < got["cost"][:, 0]).all()                              # exact: a step is accepted only if F falls
    cam5 = lambda c3: np.concatenate([c3, rc["cam"][:, 3:]], 1)                       # noqa: E731
    e0 = rn.reprojection_error(rc["pose"], rc["jrest"], rc["kp"], rc["cam"][:, :3], rc["cam"], rc["norm"])
    e1 = rn.reprojection_error(got["pose"], rc["jrest"], rc["kp"], got["cam"], cam5(got["cam"]), rc["norm"])
    assert (e1 < e0).all(), (e0, e1)
    turned, other = list(rn.TURNED), [j for j in range(24) if j not in rn.TURNED]
    ang = lambda P: np.array([[rn.angle_deg(rc["truth"][i, j], P[i, j].astype(np.float64)) for j in turned] for i in range(len(P))])   # noqa: E731
    before, after, want = ang(rc["pose"]), ang(got["pose"]), ang(ref["pose64"])
    tol = TOL[10]["shift"] + 180.0 * EPS32
    print(f"kp_refit recovery: turned joints {before.mean():.2f} -> {after.mean():.2f} deg from the truth (restatement {want.mean():.2f}), "
          f"least gain {(before - after).min():.2f} deg; shift of the others <= {got['shift'][:, other].max():.3f} deg, of the turned >= "
          f"{got['shift'][:, turned].min():.2f} deg")
    assert (after < before).all()
    assert (after <= want + tol).all(), np.abs(after - want).max()
    assert (got["shift"][:, other].max(1) < got["shift"][:, turned].min(1)).all()


def test_argument_errors(data, cuda):
    from poco_amd._lib import PocoHipError
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)                              # noqa: E731
    base = dict(pose=t(data["pose"]), u=t(data["u"]), jrest=t(data["jrest"]), kp=t(data["kp"]), cam=t(data["cam"]), norm=t(data["norm"]),
                kp_joint=rn.BODY25_TO_SMPL, parents=rn.SMPL_PARENTS, **rn.DEFAULTS)
    bad_par = rn.SMPL_PARENTS.copy()
    bad_par[4] = 9
    bad_kpj = rn.BODY25_TO_SMPL.copy()
    bad_kpj[0] = 24
    N = len(data["pose"])
    for kw in (dict(pose=base["pose"][:, :23]), dict(pose=base["pose"].double()), dict(u=base["u"][:-1]), dict(jrest=base["jrest"][:, :, :2]),
               dict(kp=torch.zeros(N, 33, 3, device=cuda)), dict(cam=base["cam"][:, :3]), dict(norm=base["norm"][:-1]), dict(kp_joint=bad_kpj),
               dict(kp_joint=rn.BODY25_TO_SMPL[:24]), dict(parents=bad_par), dict(lam=0.0), dict(lam=float("nan")), dict(u_ref=0.0),
               dict(rho=float("inf")), dict(cam_prior=0.0), dict(min_kp=1), dict(iters=0), dict(iters=33), dict(max_blocks=-1),
               dict(out={"pose": torch.empty(1, device=cuda)})):
        with pytest.raises(PocoHipError, match="kp_refit"):
            ops.kp_refit(**{**base, **kw})
    # the C entry refuses an output that is its own input
    out = {"pose": base["pose"], "cam": torch.empty(N, 3, device=cuda), "shift": torch.empty(N, 24, device=cuda),
           "cost": torch.empty(N, 2, device=cuda), "info": torch.empty(N, 2, device=cuda, dtype=torch.int32)}
    with pytest.raises(PocoHipError, match="overlap"):
        ops.kp_refit(**base, out=out)
