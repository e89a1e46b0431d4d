"""CPU: the uncertainty-weighted smoother's contract pinned on its numpy restatement tests/usmooth_np.py -
the yardstick of tests/test_usmooth_gpu.py - plus the C ABI's declaration and argument checks (fake pointers, refused before any
GPU work) and demo.py's flags."""
import ctypes as C

import numpy as np
import pytest

from poco_amd import _lib
from tests import tta_np, usmooth_np as unp


@pytest.fixture(scope="module")
def case():
    return unp.gpu_case()


def test_dense_solve_matches_a_plain_banded_ldl_on_the_gpu_tests_inputs(case):
    """Two routes to A X = diag(w) Y on the material of the GPU test: LU with pivoting on the dense matrix and L D L^T on its bands.
    The issue measured 1e-12 between them for lambda <= 100."""
    for lam in (1.0, 100.0):
        worst = 0.0
        for p, T in enumerate(unp.LENGTHS):
            lo, hi = int(case["offsets"][p]), int(case["offsets"][p + 1])
            D, om = unp.penalty(case["frames"][lo:hi], unp.MAX_GAP)
            for j in (0, 7, 23):
                w = unp.weights(case["u"][lo:hi, j], 0.3)
                Y = np.concatenate([case["pose"][lo:hi, j].reshape(T, 9), case["lin"][lo:hi]], 1).astype(np.float64)
                A = unp.system(w, D, om, lam)
                assert np.array_equal(A, A.T) or np.abs(A - A.T).max() < 1e-9
                assert np.linalg.eigvalsh(A).min() > 0.0                      # positive definite whatever the data
                if T > 4:
                    assert np.abs(np.triu(A, 3)).max() == 0.0                  # pentadiagonal
                dense = np.linalg.solve(A, w[:, None] * Y)
                worst = max(worst, float(np.abs(dense - unp.solve_banded_ldl(w, D, om, lam, Y)).max()))
        assert worst < 1e-11, (lam, worst)


def test_weights_clamp_and_non_finite():
    u = np.array([0.3, 0.05, 3.0, 0.0, -1.0, 1e-9, 1e9, np.nan, np.inf, -np.inf], np.float32)
    w = unp.weights(u, 0.3)
    assert abs(w[0] - (0.3 / np.float64(np.float32(0.3))) ** 2) < 1e-15
    assert w[1] > 35.9 and abs(w[2] - 0.01) < 1e-8
    assert w[3] == 1e6 and w[4] == 1e6 and w[5] == 1e6                         # max(u, 1e-6), then the upper clamp
    assert w[6] == 1e-6 and w[7] == 1e-6 and w[8] == 1e-6 and w[9] == 1e-6


def test_penalty_rows_unit_spacing_holes_and_uneven_steps():
    D, om = unp.penalty(np.arange(5), 30)
    assert np.array_equal(D[2], [0, 1, -2, 1, 0]) and om.tolist() == [0, 1, 1, 1, 0] and not D[0].any() and not D[4].any()
    D, om = unp.penalty([0, 1, 3, 4, 44, 45, 46], 30)                          # steps 1, 2, 1, 40, 1, 1
    assert np.allclose(D[1, :3], [2 / 3, -1.0, 1 / 3]) and om[1] == 1.5
    assert not D[3].any() and not D[4].any() and om[3] == 0 and om[4] == 0      # either side of the hole
    assert np.array_equal(D[5, 4:], [1, -2, 1])
    f = np.array([0, 1, 3, 4, 44, 45, 46], np.float64)
    assert np.abs(D @ f).max() < 1e-14 and np.abs(D @ np.ones(7)).max() < 1e-15   # D annihilates what is linear in the frame index
    assert np.allclose((D @ (f * f))[[1, 2, 5]], 2.0)                            # and gives a parabola its second derivative


def test_a_linear_sequence_in_the_linear_block_comes_back_unchanged(case):
    r = np.random.default_rng(5)
    T = 60
    frames = np.cumsum(r.choice((1, 1, 2, 3, 7), T)).astype(np.int32)           # holes, none wider than max_gap
    a, b = r.standard_normal(14), r.standard_normal(14) * 0.05
    lin = (a + b * frames[:, None]).astype(np.float32)                           # (the fp32 rounding is part of the input)
    lin64 = a + b * frames[:, None]
    pose = np.tile(np.eye(3, dtype=np.float32), (T, 24, 1, 1))
    u = r.uniform(0.05, 3.0, (T, 24)).astype(np.float32)
    u[r.random((T, 24)) < 0.05] = np.nan
    for lam in (1.0, 100.0, 1e4):
        out = unp.smooth(pose, u, frames, np.array([0, T], np.int32), lin, lam, 0.3, 30)
        # exactly linear data would return exactly; the input's fp32 rounding (<= 2^-24 relative) is smoothed, not amplified
        assert np.abs(out["lin64"] - lin64).max() <= 2.0 ** -23 * np.abs(lin64).max()
        assert np.abs(out["pose64"] - np.eye(3)).max() < 1e-14 and out["shift64"].max() < 1e-6


def test_short_tracks_are_the_projected_input(case):
    for p in (0, 1):                                                             # T = 1 and T = 2: no penalty row
        lo, hi = int(case["offsets"][p]), int(case["offsets"][p + 1])
        out = unp.smooth(case["pose"][lo:hi], case["u"][lo:hi], case["frames"][lo:hi], np.array([0, hi - lo], np.int32), case["lin"][lo:hi],
                         100.0, 0.3, 30)
        want = unp.project_batch(case["pose"][lo:hi].reshape(-1, 3, 3).astype(np.float64)).reshape(hi - lo, 24, 3, 3)
        assert np.abs(out["pose64"] - want).max() < 1e-14 and np.abs(out["lin64"] - case["lin"][lo:hi]).max() < 1e-14


def test_batched_projection_is_tta_np_project_bit_for_bit(case):
    r = np.random.default_rng(9)
    M = np.concatenate([case["pose"][:40, 3].astype(np.float64) + 0.05 * r.standard_normal((40, 3, 3)), [np.eye(3), np.zeros((3, 3))]])
    got = unp.project_batch(M)
    for i in range(len(M)):
        assert np.array_equal(got[i], tta_np.project(M[i])), i
    ok = got[:-1]
    assert np.abs(ok @ ok.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14 and np.abs(np.linalg.det(ok) - 1).max() < 1e-14
    assert np.abs(got[:40] - np.stack([tta_np.project_svd(m) for m in M[:40]])).max() < 1e-12


def test_an_outlier_moves_by_its_uncertainty():
    T = 21
    R0 = unp.infill_np.rot_axis([1, 2, 3], 0.4).astype(np.float32)
    pose = np.tile(R0, (T, 24, 1, 1))
    pose[10, :] = (R0.astype(np.float64) @ unp.infill_np.rot_axis([0, 0, 1], np.deg2rad(20.0))).astype(np.float32)
    moved = {}
    for uo in (0.05, 3.0):
        u = np.full((T, 24), 0.1, np.float32)
        u[10] = uo
        out = unp.smooth(pose, u, np.arange(T), np.array([0, T], np.int32), np.zeros((T, 0), np.float32), 10.0, 0.3, 30)
        moved[uo] = out["shift64"][:, 5]
    assert moved[3.0][10] > moved[3.0][[9, 11]].max()                            # a doubtful outlier: its confident neighbours move less
    assert moved[3.0][10] > 19.0 and moved[0.05][10] < 10.0 and moved[3.0][10] > moved[0.05][10]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_c_abi_declares_exports_and_checks_its_arguments():
    L = _lib.lib()
    assert "poco_op_track_smooth" in _lib.header_symbols() and hasattr(L, "poco_op_track_smooth")
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and "#define POCO_SMOOTH_MAX_LIN 16" in txt and "POCO_SMOOTH_SCRATCH_DOUBLES(N, L)" in txt
    fake, null = C.c_void_p(4096), C.c_void_p(0)

    def call(pose=fake, u=fake, frames=fake, offsets=fake, P=2, N=10, lin=fake, Ln=14, lam=10.0, ref=0.3, gap=30, scratch=fake,
             pose_out=C.c_void_p(8192), lin_out=C.c_void_p(8192), shift=fake):
        return L.poco_op_track_smooth(pose, u, frames, offsets, P, N, lin, Ln, C.c_double(lam), C.c_double(ref), gap, scratch, pose_out,
                                      lin_out, shift, 0, null)
    for kw in (dict(pose=null), dict(u=null), dict(frames=null), dict(offsets=null), dict(scratch=null), dict(pose_out=null),
               dict(shift=null), dict(lin=null), dict(lin_out=null), dict(Ln=0), dict(Ln=17), dict(Ln=-1), dict(gap=0), dict(gap=-3),
               dict(P=0), dict(N=1), dict(N=(1 << 31) // 216 + 1), dict(lam=0.0), dict(lam=-1.0), dict(lam=1.0001e4),
               dict(lam=float("nan")), dict(lam=float("inf")), dict(ref=0.0), dict(ref=-0.3), dict(ref=float("nan")),
               dict(ref=float("inf")), dict(pose_out=fake), dict(lin_out=fake)):
        assert call(**kw) == 1, kw
        assert "poco_op_track_smooth" in L.poco_last_error().decode(), kw


def test_ops_track_smooth_refuses_bad_arguments_without_a_gpu():
    import torch
    from poco_amd import ops
    assert ops.smooth_scratch_doubles(10, 14) == 10 * 280
    with pytest.raises(_lib.PocoHipError, match="CUDA"):
        ops.track_smooth(torch.zeros(4, 24, 3, 3), torch.zeros(4, 24), torch.zeros(4, dtype=torch.int32),
                         torch.tensor([0, 4], dtype=torch.int32), torch.zeros(4, 14), 10.0, 0.3, 30)


# ---- demo.py ---------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]


def test_demo_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    import demo
    a = demo.parse_args(BASE)
    assert a.smooth_uncert is None and a.smooth_uncert_ref == 0.3 and a.smooth_uncert_max_gap == 30
    a = demo.parse_args(BASE + ["--mode", "video", "--smooth_uncert", "10", "--smooth_uncert_ref", "0.5", "--smooth_uncert_max_gap", "8"])
    assert a.smooth_uncert == 10.0 and a.smooth_uncert_ref == 0.5 and a.smooth_uncert_max_gap == 8
    with pytest.raises(SystemExit):
        demo.parse_args(BASE + ["--smooth_uncert"])                              # the stiffness is the user's to state
    vid = ["--mode", "video", "--smooth_uncert", "10"]
    for flags, word in ((["--mode", "folder", "--smooth_uncert", "10"], "--mode video"),
                        (["--mode", "video", "--smooth_uncert_ref", "0.5"], "--smooth_uncert LAMBDA"),
                        (["--mode", "video", "--smooth_uncert_max_gap", "8"], "--smooth_uncert LAMBDA"),
                        (vid + ["--smooth"], "two smoothers"),
                        (vid + ["--gpus", "2"], "--gpus"),
                        (["--mode", "video", "--smooth_uncert", "0"], "(0, 1e4]"),
                        (["--mode", "video", "--smooth_uncert", "20000"], "(0, 1e4]"),
                        (["--mode", "video", "--smooth_uncert", "nan"], "(0, 1e4]"),
                        (vid + ["--smooth_uncert_ref", "0"], "smooth_uncert_ref"),
                        (vid + ["--smooth_uncert_max_gap", "0"], "smooth_uncert_max_gap")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work: no engine, no input folder needed
            demo.main(demo.parse_args(BASE + flags + ["--vid_file", str(tmp_path / "missing"), "--image_folder", str(tmp_path / "missing")]))
        assert word in str(e.value), (flags, e.value)
