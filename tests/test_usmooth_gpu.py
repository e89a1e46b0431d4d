"""GPU: ops.track_smooth (poco_op_track_smooth, csrc/track_smooth.hip) against its float64 numpy restatement tests/usmooth_np.py,
which solves the dense system where the kernel factors the bands.

Material (usmooth_np.gpu_case): tracks of 1, 2, 3, 4, 5, 63, 64, 65 and 130 rows in one ragged buffer (P = 9) - no penalty row,
one, two, three, rows either side of the eight-row chunks in which the kernel loads its inputs, more than two chunks of a wave -
u in [0.05, 3] with a few NaN and +Inf, frame gaps from {1, 1, 1, 2, 3, 40} with max_gap 30, L = 0 and 14, lambda 1 and 100.

Tolerance: the output is a float64 result rounded once to fp32, so the yardstick's own rounding is the
unit: d_ref = max |ref64 - fp32(ref64)| on these inputs, and the kernel may deviate from fp32(ref64) by 8 d_ref - for pose, for the
linear block and for the shift in degrees, each with its own d_ref.  Measured figures: NOTEBOOK.md, "Uncertainty-weighted
smoothing"."""
import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import infill_np, usmooth_np as unp

pytestmark = pytest.mark.gpu

U_REF = 0.3
EPS = 2.0 ** -24              # half an fp32 ulp at 1.0: the rounding of a matrix entry


@pytest.fixture(scope="module")
def data():
    return unp.gpu_case()


_REF = {}


def _ref(data, lam):
    """The restatement with L = 14, once per lambda (the pose does not depend on L)."""
    if lam not in _REF:
        _REF[lam] = unp.smooth(**data, lam=lam, u_ref=U_REF, max_gap=unp.MAX_GAP)
    return _REF[lam]


def _run(d, lam, dev, L=14, max_gap=unp.MAX_GAP, max_blocks=0):
    """Through outputs poisoned with NaN: an element the kernel leaves out fails every comparison."""
    N = d["pose"].shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                               # noqa: E731
    out = [torch.full(s, float("nan"), device=dev) for s in ((N, 24, 3, 3), (N, L), (N, 24))]
    res = ops.track_smooth(t(d["pose"]), t(d["u"]), t(d["frames"]), torch.from_numpy(d["offsets"]), t(d["lin"][:, :L]), lam, U_REF, max_gap,
                           out=out, max_blocks=max_blocks)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in zip(("pose", "lin", "shift"), res)}
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _compare(got, ref, L, what):
    """-> {key: (observed deviation, d_ref)}; asserts observed <= 8 d_ref."""
    figs = {}
    for k in ("pose", "lin", "shift"):
        r64, r32 = ref[k + "64"], ref[k]
        if k == "lin":
            r64, r32 = r64[:, :L], r32[:, :L]
            if L == 0:
                continue
        d_ref = float(np.abs(r64 - r32.astype(np.float64)).max())
        obs = float(np.abs(got[k].astype(np.float64) - r32.astype(np.float64)).max())
        figs[k] = (obs, d_ref)
    print(f"track_smooth {what}: " + ", ".join(f"{k} deviation {o:.3e} (d_ref {d:.3e}, {o / d:.2f} x)" for k, (o, d) in figs.items()))
    for k, (o, d) in figs.items():
        assert d > 0 and o <= 8.0 * d, (what, k, o, d)
    return figs


@pytest.mark.parametrize("L", [0, 14])
@pytest.mark.parametrize("lam", [1.0, 100.0])
def test_ragged_call_matches_the_restatement(data, lam, L, cuda):
    ref = _ref(data, lam)
    assert np.isnan(data["u"]).sum() > 20 and np.isinf(data["u"]).sum() > 20      # the material is what the docstring says
    gaps = np.concatenate([np.diff(data["frames"][lo:hi]) for lo, hi in zip(data["offsets"][:-1], data["offsets"][1:])])
    assert set(np.unique(gaps)) == {1, 2, 3, 40}
    assert ref["shift64"].max() > 1.0                                              # something is smoothed
    got = _run(data, lam, cuda, L)
    _compare(got, ref, L, f"lambda={lam:g} L={L}")
    # every output is a rotation to fp32 rounding.  The fp64 result is orthonormal to 1e-15; rounding moves each entry by at most
    # EPS, so to first order |R^T R - I| <= 2 sqrt(3) EPS per entry (two sums of three products with a unit column) and
    # |det R - 1| <= sum |cofactor| EPS <= 3 sqrt(3) EPS; 4 EPS and 6 EPS leave room for the second order.
    R = got["pose"].astype(np.float64).reshape(-1, 3, 3)
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 4 * EPS
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 6 * EPS
    # T <= 2: no penalty row, the output is the projected input
    short = int(data["offsets"][2])
    want = unp.project_batch(data["pose"][:short].reshape(-1, 3, 3).astype(np.float64)).reshape(short, 24, 3, 3)
    assert np.abs(got["pose"][:short].astype(np.float64) - want).max() <= 8 * EPS
    if L:
        assert np.array_equal(_bits(got["lin"][:short]), _bits(data["lin"][:short]))   # w y / w rounds back to the fp32 it came from
    # the same call again, and on a grid of three blocks: the same bits
    for kw in ({}, {"max_blocks": 3}):
        again = _run(data, lam, cuda, L, **kw)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(again[k])), (k, kw)


def test_each_track_alone_gives_the_same_bits(data, cuda):
    whole = _run(data, 100.0, cuda)
    off = data["offsets"]
    for p, T in enumerate(unp.LENGTHS):
        lo, hi = int(off[p]), int(off[p + 1])
        d = {k: data[k][lo:hi] for k in ("pose", "u", "frames", "lin")}
        got = _run(dict(d, offsets=np.array([0, T], np.int32)), 100.0, cuda)
        for k in got:
            assert np.array_equal(_bits(got[k]), _bits(whole[k][lo:hi])), (T, k)


def test_a_hole_wider_than_max_gap_splits_the_track(data, cuda):
    """One track of 70 rows with a hole of 40 frames after row 37 = its two halves as separate tracks: no penalty row spans the
    hole, so A is block diagonal.  Both sides are the kernel; the tolerance is that of the comparison with the restatement."""
    lo = int(data["offsets"][-2])                                                   # rows of the 130-row track
    d = {k: data[k][lo:lo + 70].copy() for k in ("pose", "u", "lin")}
    frames = np.arange(70, dtype=np.int32)
    frames[38:] += 39
    one = _run(dict(d, frames=frames, offsets=np.array([0, 70], np.int32)), 100.0, cuda)
    two = _run(dict(d, frames=frames, offsets=np.array([0, 38, 70], np.int32)), 100.0, cuda)
    ref = unp.smooth(**d, frames=frames, offsets=np.array([0, 38, 70], np.int32), lam=100.0, u_ref=U_REF, max_gap=unp.MAX_GAP)
    for k in ("pose", "lin", "shift"):
        d_ref = float(np.abs(ref[k + "64"] - ref[k].astype(np.float64)).max())
        assert np.abs(one[k].astype(np.float64) - two[k].astype(np.float64)).max() <= 8 * d_ref, k
    # with the hole bridged (max_gap 40) the halves do talk to each other
    bridged = _run(dict(d, frames=frames, offsets=np.array([0, 70], np.int32)), 100.0, cuda, max_gap=40)
    assert np.abs(bridged["pose"] - one["pose"]).max() > 1e-4


def test_a_linear_sequence_in_the_linear_block_comes_back(data, cuda):
    r = np.random.default_rng(5)
    T = 130
    frames = np.cumsum(r.choice((1, 1, 2, 3, 7), T)).astype(np.int32)               # holes, none wider than max_gap
    a, b = r.standard_normal(14), r.standard_normal(14) * 0.05
    lin = (a + b * frames[:, None]).astype(np.float32)
    lo = int(data["offsets"][-2])
    d = dict(pose=data["pose"][lo:lo + T], u=data["u"][lo:lo + T], frames=frames, offsets=np.array([0, T], np.int32), lin=lin)
    for lam in (1.0, 100.0):
        got = _run(d, lam, cuda)
        # D annihilates a + b f exactly; what is left is the input's own fp32 rounding (<= 2^-24 relative, smoothed: 2^-23 bounds
        # it in tests/test_usmooth_cpu.py) and the rounding of the store (2^-24): together below 2^-22 of the largest entry
        assert np.abs(got["lin"].astype(np.float64) - lin.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(lin).max()


def test_an_outlier_moves_by_its_uncertainty(cuda):
    T = 21
    R0 = infill_np.rot_axis([1, 2, 3], 0.4).astype(np.float32)
    pose = np.tile(R0, (T, 24, 1, 1))
    pose[10, :] = (R0.astype(np.float64) @ infill_np.rot_axis([0, 0, 1], np.deg2rad(20.0))).astype(np.float32)
    moved = {}
    for uo in (0.05, 3.0):
        u = np.full((T, 24), 0.1, np.float32)
        u[10] = uo
        d = dict(pose=pose, u=u, frames=np.arange(T, dtype=np.int32), offsets=np.array([0, T], np.int32), lin=np.zeros((T, 14), np.float32))
        moved[uo] = _run(d, 10.0, cuda)["shift"]
    assert (moved[3.0][10] > moved[0.05][10]).all()                                 # the doubtful outlier is drawn further
    assert (moved[3.0][10] > moved[3.0][[9, 11]].max(0)).all()                      # than its confident neighbours
    assert (moved[3.0][10] > 19.0).all() and (moved[0.05][10] < 10.0).all()


def test_argument_errors(data, cuda):
    from poco_amd._lib import PocoHipError
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)                              # noqa: E731
    N = data["pose"].shape[0]
    base = dict(pose=t(data["pose"]), u=t(data["u"]), frames=t(data["frames"]), offsets=torch.from_numpy(data["offsets"]), lin=t(data["lin"]),
                lam=10.0, u_ref=0.3, max_gap=8)
    bad_off = data["offsets"].copy()
    bad_off[3] = bad_off[2]
    for kw in (dict(pose=base["pose"][:, :23]), dict(pose=base["pose"].double()), dict(u=base["u"][:-1]), dict(frames=base["frames"].long()),
               dict(lin=torch.zeros(N, 17, device=cuda)), dict(lin=base["lin"][:-1]), dict(max_gap=0), dict(max_gap=2.5), dict(lam=0.0),
               dict(lam=2e4), dict(lam=float("nan")), dict(u_ref=0.0), dict(u_ref=float("inf")), dict(offsets=torch.from_numpy(bad_off)),
               dict(offsets=torch.from_numpy(data["offsets"][:-1].copy())), dict(out=[torch.empty(1, device=cuda)] * 3)):
        with pytest.raises(PocoHipError, match="track_smooth"):
            ops.track_smooth(**{**base, **kw})
