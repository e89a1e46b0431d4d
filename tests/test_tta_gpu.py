"""GPU: ops.tta_fuse (poco_op_tta_fuse, csrc/tta_fuse.hip) against its float64 restatement tests/tta_np.py.

Shapes (B, K) = (1, 2), (3, 3), (65, 8), (130, 2) with both weights: one lane, part of a wave, 1560 lanes on 7 blocks with every view
slot in use, 3120 lanes on 13 blocks.  The view tables mix flip, rot in {0, 15, -90} and both together.  Every (crop, joint) is a
common rotation perturbed by at most 0.6 rad per view (the smallest singular value of M / W stays above 0.8, tests/test_tta_cpu.py)
and sent forward into its view's frame, so the operator has to undo the flip, the joint permutation and the root's rotation to
bring the views together.  Where B >= 3 one view of crop 1 has NaN in its var, one view of crop 2 has a NaN in its pose, one
(crop, joint) is dropped in every view, and so is the root of crop 2: its shape is the base view's words.  Inputs lie in NaN-filled
ops.Rows buffers of exactly K * B rows, outputs between poisoned guard bands with NaN where the kernel must write.

Tolerances against the float64 restatement: pose' max-abs 2^-22 (entries at most 1 in magnitude, one fp32 rounding is 2^-24, the
margin of 4 covers the fixed-sweep solve whose float64 residual the CPU test bounds at 1e-12); var', spread and betas' relative
2^-22, with an absolute floor of 2^-40 for spread."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from poco_amd import _lib, ops
from tests import tta_np

pytestmark = pytest.mark.gpu

TABLES = {2: [(0, 0.0), (1, 15.0)], 3: [(0, 0.0), (1, 0.0), (0, -90.0)],
          8: [(0, 0.0), (1, 0.0), (0, 15.0), (1, 15.0), (0, -90.0), (1, -90.0), (1, 0.0), (0, 15.0)]}
TABLE_130 = [(0, 0.0), (1, -90.0)]
SHAPES = [(1, 2), (3, 3), (65, 8), (130, 2)]
POSE_TOL, REL_TOL, SPREAD_FLOOR = 2.0 ** -22, 2.0 ** -22, 2.0 ** -40
NAN_BITS = 0x7FC00000


def _table(B, K):
    return TABLE_130 if B == 130 else TABLES[K]


def _rodrigues(axis, angle):
    k = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def _forward(R, j, flip, rot):
    """What pose_processing does to joint j's rotation, on matrices: the root turns by Rz(-rot), then the flip."""
    if j == 0 and rot != 0:
        c, s = tta_np.view_cs(-rot)
        R = tta_np.unrotate(R, c, s)
    return tta_np.unflip(R) if flip else R


def _material(B, K):
    r = np.random.default_rng(1000 * B + K)
    views = _table(B, K)
    pose = np.zeros((K, B, 24, 3, 3))
    for b in range(B):
        for j in range(24):
            R0 = _rodrigues(r.standard_normal(3), r.uniform(0, math.pi))
            for k, (flip, rot) in enumerate(views):
                Rk = R0 @ _rodrigues(r.standard_normal(3), r.uniform(0, 0.6))
                pose[k, b, tta_np.FLIP_PERM[j] if flip else j] = _forward(Rk, j, flip, rot)
    var = r.uniform(0.005, 0.5, (K, B, 24))
    betas = r.standard_normal((1, B, 10)) + 0.1 * r.standard_normal((K, B, 10))
    pose, var, betas = pose.astype(np.float32), var.astype(np.float32), betas.astype(np.float32)
    if B >= 3:
        var[K - 1, 1, :] = np.nan                                    # a view without a usable uncertainty
        pose[1, 2, :, 2, 1] = np.nan                                 # a view with a broken rotation in every joint
        var[:, 0, 3] = np.nan                                        # joint 3 (its own mirror) of crop 0: dropped in every view
        var[0, 0, 7], var[1, 0, 9] = -1.0, np.inf                    # a negative and an infinite var: dropped
        var[:, 2, 0] = np.nan                                        # the root of crop 2 in every view: its shape has no weight either
    return pose.reshape(K * B, 24, 3, 3), var.reshape(K * B, 24), betas.reshape(K * B, 10), views


_CACHE = {}


def _case(B, K, weight):
    """Material and restatement, once per case."""
    if (B, K) not in _CACHE:
        _CACHE[(B, K)] = {"mat": _material(B, K)}
    c = _CACHE[(B, K)]
    if weight not in c:
        pose, var, betas, views = c["mat"]
        c[weight] = tta_np.fuse(pose, var, betas, views, weight)
    return c["mat"], c[weight]


class _Out:
    """`shape` floats the kernel must write (NaN on entry) in the middle of a poisoned Rows buffer."""

    def __init__(self, shape, dev):
        self.n = int(np.prod(shape))
        self.rows = ops.Rows(1, self.n + 8, dev, "poison").mark(4, self.n)
        self.t = self.rows.body.view(-1)[4:4 + self.n].view(shape)

    def intact(self):
        return self.rows.untouched([(4, self.n)])


def _run(mat, weight, dev, max_blocks=0):
    pose, var, betas, views = mat
    K = len(views)
    B = len(pose) // K
    up = lambda a, w: ops.Rows(K * B, w, dev, "nan").put(0, torch.from_numpy(a).to(dev))   # noqa: E731
    dp, dv, db = up(pose, 216), up(var, 24), up(betas, 10)
    o = {"pose": _Out((B, 24, 3, 3), dev), "var": _Out((B, 24), dev), "spread": _Out((B, 24), dev), "betas": _Out((B, 10), dev)}
    ops.tta_fuse(dp.body.view(K * B, 24, 3, 3), dv.body, db.body, views, weight, out={k: v.t for k, v in o.items()}, max_blocks=max_blocks)
    torch.cuda.synchronize()
    for k, v in o.items():
        assert v.intact(), (k, B, K, weight)
    return {k: v.t.cpu().numpy() for k, v in o.items()}


def _rel(got, want):
    return np.abs(got.astype(np.float64) - want) / np.abs(want)


def _compare(got, ref, what):
    W = ref["W"]
    live = W > 0
    assert not np.isnan(got["pose"]).any() or not live.all()
    d_pose = np.abs(got["pose"].astype(np.float64) - ref["pose"])[live].max()
    d_var = _rel(got["var"], ref["var"])[live].max()
    sp = np.abs(got["spread"].astype(np.float64) - ref["spread"])[live]
    d_spread = (sp / np.maximum(np.abs(ref["spread"][live]), 1e-300))[sp > SPREAD_FLOOR].max(initial=0.0)
    d_betas = _rel(got["betas"], ref["betas"]).max()
    print(f"{what}: pose' max-abs {d_pose:.3e} (2^-22 = {POSE_TOL:.3e}), var' rel {d_var:.3e}, spread rel {d_spread:.3e}, betas' rel {d_betas:.3e} "
          f"(2^-22 = {REL_TOL:.3e})")
    assert d_pose <= POSE_TOL and d_var <= REL_TOL and d_spread <= REL_TOL and d_betas <= REL_TOL, what
    # every view dropped: the base view's words, bit for bit, and the one quiet NaN
    dead = ~live
    assert (got["spread"].view(np.uint32)[dead] == NAN_BITS).all() and not np.isnan(got["spread"][live]).any()
    assert np.array_equal(got["pose"].view(np.uint32)[dead], ref["pose"].astype(np.float32).view(np.uint32)[dead])
    assert np.array_equal(got["var"].view(np.uint32)[dead], ref["var"].astype(np.float32).view(np.uint32)[dead])
    # a root dropped in every view: no weight for the shape either, the base view's ten words
    no_root = dead[:, 0]
    assert np.array_equal(got["betas"].view(np.uint32)[no_root], ref["betas"].astype(np.float32).view(np.uint32)[no_root])


def test_the_material_holds_every_case():
    """Without these the comparisons below show nothing."""
    for B, K in SHAPES:
        (pose, var, betas, views), ref = _case(B, K, 1)
        assert len(views) == K and views[0] == (0, 0.0) and any(f for f, _ in views) and any(r for _, r in views)
        d = ref["dropped"]
        if B >= 3:
            assert d[K - 1, 1].all() and d[1, 2].all() and d[:, 0, 3].all() and d[:, 2, 0].all()
            dead = ref["W"] == 0
            assert dead.sum() == 2 and dead[0, 3] and dead[2, 0] and np.isnan(ref["spread"]).sum() == 2
            base = betas.reshape(K, B, 10)[0]
            assert np.array_equal(ref["betas"][2], base[2].astype(np.float64)) and not np.array_equal(ref["betas"][1], base[1].astype(np.float64))
            assert d[0, 0, 7] and d[1, 0, 9 if not views[1][0] else tta_np.FLIP_PERM[9]]
            assert not d[0, 1].any()
        else:
            assert not d.any()
        # undoing the views matters: fused without the inverse transforms the root is somewhere else
        plain = tta_np.fuse(pose, var, betas, [(0, 0.0)] * K, 1)
        assert np.abs(plain["pose"][:, 0] - ref["pose"][:, 0]).max() > 0.05
        live = ref["W"] > 0
        # the views disagree by the 0.6 rad they were given (an entry left with a single view has no spread to speak of)
        assert 1e-4 < np.median(ref["spread"][live]) and ref["spread"][live].max() < 0.2
    assert any(v == (1, 15.0) for v in TABLES[8]) and any(v == (1, -90.0) for v in TABLES[8])    # flip and rotation together


@pytest.mark.parametrize("weight", [1, 0], ids=["uncert", "uniform"])
@pytest.mark.parametrize("B,K", SHAPES)
def test_operator_matches_the_restatement(B, K, weight, cuda):
    mat, ref = _case(B, K, weight)
    _compare(_run(mat, weight, cuda), ref, (B, K, weight))


@pytest.mark.parametrize("B,K", [(130, 2), (65, 8)])
def test_the_result_does_not_depend_on_the_grid(B, K, cuda):
    """13 (7) blocks by default against one block whose grid-stride loop takes 13 (7) turns: the same bits."""
    mat, _ = _case(B, K, 1)
    a, b = _run(mat, 1, cuda), _run(mat, 1, cuda, max_blocks=1)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_views_half_a_turn_apart_still_give_a_rotation(cuda):
    """K = 2, uniform weights, the second view half a turn about x from the first: M has rank 1, the maximiser is not unique, and
    the contract promises only a proper rotation."""
    r = np.random.default_rng(2)
    B = 2
    R1 = np.stack([_rodrigues(r.standard_normal(3), r.uniform(0, math.pi)) for _ in range(B * 24)]).reshape(B, 24, 3, 3)
    pose = np.concatenate([R1, R1 @ np.diag([1.0, -1.0, -1.0])]).astype(np.float32)
    var = np.full((2 * B, 24), 0.1, np.float32)
    betas = np.zeros((2 * B, 10), np.float32)
    got = _run((pose, var, betas, [(0, 0.0), (0, 0.0)]), 0, cuda)
    R = got["pose"].astype(np.float64).reshape(-1, 3, 3)
    assert np.isfinite(R).all() and np.isfinite(got["spread"]).all()
    assert np.abs(np.einsum("nij,nik->njk", R, R) - np.eye(3)).max() <= 2.0 ** -20
    assert (np.linalg.det(R) > 0).all()


def test_wrapper_refuses_other_shapes(cuda):
    z = lambda *s: torch.zeros(*s, device=cuda)                                     # noqa: E731
    good = dict(pose=z(4, 24, 3, 3), var=z(4, 24), betas=z(4, 10), views=[(0, 0.0), (1, 0.0)])
    for kw in (dict(var=z(4, 24, 1)), dict(var=z(2, 24)), dict(betas=z(4, 9)), dict(pose=z(5, 24, 3, 3)), dict(pose=z(4, 24, 9)),
               dict(views=[(0, 0.0)]), dict(views=[(0, 0.0)] * 9), dict(views=[(1, 0.0), (0, 0.0)]), dict(views=[(0, 15.0), (1, 0.0)]),
               dict(views=[(0, 0.0), (2, 0.0)]), dict(views=[(0, 0.0), (0, float("nan"))]), dict(weight="median"), dict(weight=2),
               dict(pose=z(4, 24, 3, 3).double()), dict(out={"pose": z(2, 24, 3, 3), "var": z(2, 24), "spread": z(2, 24), "betas": z(2, 9)})):
        with pytest.raises(ops.PocoHipError, match="tta_fuse"):
            ops.tta_fuse(**{**good, **kw})


def test_every_argument_error_leaves_the_outputs_untouched(cuda):
    """The C entry with real device buffers and one bad argument at a time: POCO_ERR_ARG naming the entry, nothing launched."""
    (pose, var, betas, views), _ = _case(3, 3, 1)
    K, B = 3, 3
    up = lambda a, w: ops.Rows(K * B, w, cuda, "nan").put(0, torch.from_numpy(a).to(cuda))   # noqa: E731
    dp, dv, db = up(pose, 216), up(var, 24), up(betas, 10)
    o = {"pose": _Out((B, 24, 3, 3), cuda), "var": _Out((B, 24), cuda), "spread": _Out((B, 24), cuda), "betas": _Out((B, 10), cuda)}
    L = _lib.lib()
    fn = L.poco_op_tta_fuse
    fn.argtypes = ops.TTA_ARGTYPES
    good = [(f, *tta_np.view_cs(r)) for f, r in views]
    ptr = dict(pose=dp.body.data_ptr(), var=dv.body.data_ptr(), betas=db.body.data_ptr(), pose_out=o["pose"].t.data_ptr(), var_out=o["var"].t.data_ptr(),
               spread=o["spread"].t.data_ptr(), betas_out=o["betas"].t.data_ptr())

    def call(B=B, views=good, weight=1, **kw):
        a = {**ptr, **kw}
        return fn(a["pose"], a["var"], a["betas"], B, ops.tta_views(views), weight, a["pose_out"], a["var_out"], a["spread"], a["betas_out"], 0,
                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [dict(pose=None), dict(var=None), dict(betas=None), dict(pose_out=None), dict(var_out=None), dict(spread=None), dict(betas_out=None),
           dict(views=good[:1]), dict(views=good * 3), dict(B=0), dict(B=(1 << 24) + 1), dict(weight=2), dict(views=[good[0], (2, 1.0, 0.0), good[2]]),
           dict(views=[good[0], (0, float("nan"), 0.0), good[2]]), dict(views=[good[0], (0, 0.6, 0.6), good[2]]), dict(views=[good[1], good[0], good[2]]),
           dict(views=[(0, 0.0, 1.0), good[1], good[2]]), dict(pose_out=ptr["pose"]), dict(var_out=ptr["var"]), dict(betas_out=ptr["betas"]),
           dict(spread=ptr["var_out"]), dict(var_out=ptr["var"] + 4 * 24)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "poco_op_tta_fuse" in L.poco_last_error().decode(), kw
    torch.cuda.synchronize()
    for k, v in o.items():
        assert v.intact() and bool(torch.isnan(v.t).all()), k
    assert call() == 0                                                              # and the same buffers with good arguments run
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(v.t).all()) for v in o.values()) and all(v.intact() for v in o.values())
