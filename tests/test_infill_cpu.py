"""CPU: the in-fill's contract pinned on hand-checkable cases of its numpy restatement tests/infill_np.py -
the yardstick of tests/test_infill_gpu.py - plus the C ABI's declaration and argument checks (fake pointers, refused before any GPU
work) and demo.py's two flags."""
import ctypes as C

import numpy as np
import pytest

from poco_amd import _lib
from tests import infill_np as inp

EYE = np.eye(3, dtype=np.float32)
THR = 0.5


def _case(T, bad, frames=None, P=None, L=3, seed=0, max_gap=30, pose=None, u=None):
    """One or more tracks (P = offsets) of T rows; `bad` = [(row, joint)] unreliable entries (joint None = all 24)."""
    r = np.random.default_rng(seed)
    pose = inp.smooth_rotations(r, T, 3.0) if pose is None else pose
    uu = np.full((T, 24), 0.1, np.float32) if u is None else u
    for t, j in bad:
        uu[t, slice(None) if j is None else j] = 0.9
    frames = np.arange(T) if frames is None else np.asarray(frames)
    lin = r.standard_normal((T, L)).astype(np.float32)
    offsets = np.array([0, T] if P is None else P, np.int32)
    return dict(pose=pose, u=uu, frames=frames.astype(np.int32), offsets=offsets, lin=lin, thresh=THR, max_gap=max_gap)


def _rz(deg):
    return inp.rot_axis([0, 0, 1], np.deg2rad(deg)).astype(np.float32)


def test_quarter_turn_halfway_is_the_eighth_turn():
    pose = np.tile(EYE, (3, 24, 1, 1))
    pose[2, :] = _rz(90)
    pose[1, :] = _rz(-33)                                  # what the network said at the unreliable row: must not matter
    out = inp.infill(**_case(3, [(1, 5)], pose=pose))
    assert out["flags"][1, 5] == 1 and out["flags"].sum() == 1 and out["touched"].tolist() == [0, 1, 0]
    assert np.abs(out["pose64"][1, 5] - inp.rot_axis([0, 0, 1], np.pi / 4)).max() < 1e-7       # (the anchors are fp32 roundings)
    assert np.array_equal(out["pose"][1, 5], out["pose64"][1, 5].astype(np.float32))
    # s from the frame indices, holes included: frames 10, 12, 16 put the middle row a third of the way
    out = inp.infill(**_case(3, [(1, 5)], pose=pose, frames=[10, 12, 16]))
    assert np.abs(out["pose64"][1, 5] - inp.rot_axis([0, 0, 1], np.pi / 6)).max() < 1e-7


def test_quaternion_branches_flip_and_near_identical_anchors():
    # every Shepperd branch gives the rotation back
    for axis, ang in (([1, 2, 3], 0.3), ([1, 0, 0], 3.0), ([0, 1, 0], 3.0), ([0, 0, 1], 3.0), ([1, 1, 0], np.pi)):
        R = inp.rot_axis(axis, ang)
        q = inp.quat_of(R)
        assert abs(np.linalg.norm(q) - 1) < 1e-15 and np.abs(inp.rotmat_of(q) - R).max() < 1e-14
    branches = {int(np.argmax([np.trace(R), R[0, 0], R[1, 1], R[2, 2]])) for R in
                (inp.rot_axis(a, g) for a, g in (([1, 2, 3], 0.3), ([1, 0, 0], 3.0), ([0, 1, 0], 3.0), ([0, 0, 1], 3.0)))}
    assert branches == {0, 1, 2, 3}
    # antipodal representatives: -80 degrees about z leaves the trace branch with w > 0, -100 degrees the m22 branch with z > 0
    # and w < 0: two rotations 20 degrees apart whose quaternions point away from each other.  The short way is taken
    qa, qb = inp.quat_of(_rz(-80)), inp.quat_of(_rz(-100))
    assert float(qa @ qb) < -0.98                           # the branch is entered
    mid = inp.rotmat_of(inp.slerp(qa, qb, 0.5))
    assert np.abs(mid - inp.rot_axis([0, 0, 1], -np.pi / 2)).max() < 1e-7       # through -90, not the 340 degrees round
    assert np.allclose(inp.slerp(qa, -qb, 0.5), inp.slerp(qa, qb, 0.5), atol=0, rtol=0)
    # near-identical anchors: the linear blend, normalised, no 0 / 0
    q = inp.quat_of(inp.rot_axis([1, 2, 3], 0.7))
    out = inp.slerp(q, q, 0.3)
    assert np.isfinite(out).all() and np.abs(out - q).max() < 1e-15 and abs(np.linalg.norm(out) - 1) < 1e-15
    q2 = inp.quat_of(inp.rot_axis([1, 2, 3], 0.7 + 1e-7))                        # |q.q2| = 1 - 1.25e-15: still the blend
    assert float(q @ q2) > 1 - 1e-12 and np.isfinite(inp.slerp(q, q2, 0.5)).all()
    q3 = inp.quat_of(inp.rot_axis([1, 2, 3], 0.7 + 1e-5))                        # 1 - 1.25e-11: acos and sin
    assert float(q @ q3) <= 1 - 1e-12 and np.abs(inp.slerp(q, q3, 0.5) - inp.quat_of(inp.rot_axis([1, 2, 3], 0.7 + 5e-6))).max() < 1e-9


def test_gap_limits_hold_limits_and_the_tie():
    # anchors exactly max_gap apart interpolate; one frame more and the rule falls through to the hold
    c = _case(12, [(t, 0) for t in range(1, 10)], max_gap=9)                     # anchors at rows 0 and 10: 10 frames apart
    assert (inp.infill(**{**c, "max_gap": 10})["flags"][1:10, 0] == 1).all()
    f = inp.infill(**c)["flags"][1:10, 0]                                        # hold limit 9 // 2 = 4
    assert f.tolist() == [2, 2, 2, 2, 3, 2, 2, 2, 2]
    out = inp.infill(**c)
    for t, src in ((1, 0), (4, 0), (6, 10), (9, 10)):
        assert np.array_equal(out["pose"][t, 0].view(np.uint32), c["pose"][src, 0].view(np.uint32))
        assert np.array_equal(out["lin"][t].view(np.uint32), c["lin"][src].view(np.uint32))
    assert np.array_equal(out["pose"][5, 0].view(np.uint32), c["pose"][5, 0].view(np.uint32))         # flag 3: as it was
    # the tie goes to a.  (A tied entry is never held: a tie means frames[b] - frames[a] = 2 d, rule 1 failing means 2 d > max_gap,
    # so d > max_gap // 2.  The rule still names the anchor, and the decision function shows which.)
    rel = np.array([True, False, False, False, True])
    assert inp.decide(np.array([0, 1, 2, 3, 4]), rel, 2, 0, 5, 3)[:4] == (3, 0, 4, 0)                  # 2 from both: c = a
    assert inp.decide(np.array([0, 1, 2, 3, 4]), rel, 3, 0, 5, 3)[:4] == (2, 0, 4, 4)                  # nearer to b, 1 <= 3 // 2
    assert inp.decide(np.array([0, 1, 2, 3, 4]), rel, 2, 0, 5, 4)[0] == 1                              # gap exactly met
    # the hold limit exactly met and exceeded by one: a tail run after a single anchor, max_gap 7 -> 3 frames
    c = _case(8, [(t, 2) for t in range(1, 8)], max_gap=7)
    assert inp.infill(**c)["flags"][:, 2].tolist() == [0, 2, 2, 2, 3, 3, 3, 3]
    c = _case(8, [(t, 2) for t in range(0, 7)], max_gap=7)                       # a head run before a single anchor
    assert inp.infill(**c)["flags"][:, 2].tolist() == [3, 3, 3, 3, 2, 2, 2, 0]
    # max_gap 1: nothing can lie between anchors one frame apart, and 1 // 2 = 0 holds nothing
    c = _case(5, [(2, 0)], max_gap=1)
    assert inp.infill(**c)["flags"][:, 0].tolist() == [0, 0, 3, 0, 0]


def test_nan_tracks_and_untouched_rows():
    c = _case(10, [(3, 1), (4, 1)], P=[0, 5, 10])
    c["u"][7, 2] = np.nan                                                        # a NaN is unreliable
    c["frames"] = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4], np.int32)
    out = inp.infill(**c)
    assert out["flags"][7, 2] == 1
    # rows 3, 4 end track 0: their only anchor is row 2; row 5 (track 1, reliable) is across the boundary and is not used
    assert out["flags"][:, 1].tolist() == [0, 0, 0, 2, 2, 0, 0, 0, 0, 0]
    assert np.array_equal(out["pose"][4, 1], c["pose"][2, 1])
    # reliable entries and whole untouched rows keep their bits; the inputs are not modified
    keep = out["flags"] == 0
    assert np.array_equal(out["pose"].view(np.uint32)[keep], c["pose"].view(np.uint32)[keep])
    assert out["touched"].tolist() == [0, 0, 0, 1, 1, 0, 0, 1, 0, 0]
    assert np.array_equal(out["lin"].view(np.uint32), c["lin"].view(np.uint32))  # column 0 is reliable everywhere: lin as it was
    # none reliable: flag 3 everywhere, nothing changes; all reliable: flag 0
    c = _case(6, [(t, None) for t in range(6)])
    out = inp.infill(**c)
    assert (out["flags"] == 3).all() and not out["touched"].any() and np.array_equal(out["pose"].view(np.uint32), c["pose"].view(np.uint32))
    out = inp.infill(**_case(6, []))
    assert not out["flags"].any()


def test_linear_block_follows_column_zero_only():
    c = _case(7, [(2, 0), (3, 0), (4, 5), (5, 7)], frames=[0, 2, 3, 7, 8, 9, 11], L=14)
    out = inp.infill(**c)
    s = {2: (3 - 2) / (8 - 2), 3: (7 - 2) / (8 - 2)}
    for t in (2, 3):
        want = c["lin"][1].astype(np.float64) + s[t] * (c["lin"][4].astype(np.float64) - c["lin"][1].astype(np.float64))
        assert np.array_equal(out["lin"][t], want.astype(np.float32))
    for t in (0, 1, 4, 5, 6):                                                    # other columns' flags do not move lin
        assert np.array_equal(out["lin"][t].view(np.uint32), c["lin"][t].view(np.uint32))
    assert out["flags"][4, 5] == 1 and out["flags"][5, 7] == 1


def test_every_result_is_orthonormal():
    r = np.random.default_rng(3)
    T = 40
    u = r.uniform(0, 1, (T, 24)).astype(np.float32)
    c = _case(T, [], u=u, seed=3, max_gap=12)
    out = inp.infill(**c)
    assert (out["flags"] == 1).sum() > 100
    R = out["pose64"][out["flags"] == 1]
    err = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max()
    assert err < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12, err


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_c_abi_declares_and_exports_the_infill():
    L = _lib.lib()
    assert "poco_op_track_infill" in _lib.header_symbols() and hasattr(L, "poco_op_track_infill")
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and "#define POCO_INFILL_MAX_LIN 16" in txt      # additions only
    fake, null = C.c_void_p(4096), C.c_void_p(0)

    def call(pose=fake, u=fake, frames=fake, offsets=fake, P=2, N=10, lin=fake, Ln=14, gap=30, scratch=fake, pose_out=C.c_void_p(8192),
             lin_out=C.c_void_p(8192), flags=fake, touched=fake, rows=null, count=null):
        return L.poco_op_track_infill(pose, u, frames, offsets, P, N, lin, Ln, C.c_float(0.5), gap, scratch, pose_out, lin_out, flags,
                                      touched, rows, count, null)
    for kw in (dict(pose=null), dict(u=null), dict(frames=null), dict(offsets=null), dict(scratch=null), dict(pose_out=null),
               dict(flags=null), dict(touched=null), dict(lin=null), dict(lin_out=null), dict(Ln=0), dict(Ln=17), dict(Ln=-1),
               dict(gap=0), dict(gap=-3), dict(P=0), dict(N=1), dict(N=(1 << 31) // 216 + 1), dict(rows=fake), dict(count=fake),
               dict(pose_out=fake), dict(lin_out=fake)):
        assert call(**kw) == 1, kw
        assert "poco_op_track_infill" in L.poco_last_error().decode(), kw


def test_ops_track_infill_refuses_bad_arguments_without_a_gpu():
    """The wrapper's own checks come before any GPU work; host tensors are refused as such."""
    import torch
    from poco_amd import ops
    with pytest.raises(_lib.PocoHipError, match="CUDA"):
        ops.track_infill(torch.zeros(4, 24, 3, 3), torch.zeros(4, 24), torch.zeros(4, dtype=torch.int32),
                         torch.tensor([0, 4], dtype=torch.int32), torch.zeros(4, 14), 0.5, 30)


# ---- demo.py ---------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]


def test_demo_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    import demo
    a = demo.parse_args(BASE)
    assert a.infill is None and a.infill_max_gap == 30                           # no default threshold
    a = demo.parse_args(BASE + ["--mode", "video", "--infill", "0.25", "--infill_max_gap", "8"])
    assert a.infill == 0.25 and a.infill_max_gap == 8
    with pytest.raises(SystemExit):
        demo.parse_args(BASE + ["--infill"])                                     # the threshold is the user's to state
    for flags, word in ((["--mode", "folder", "--infill", "0.3"], "--mode video"),
                        (["--mode", "folder", "--infill_max_gap", "8"], "--infill"),
                        (["--mode", "video", "--infill", "0.3", "--gpus", "2"], "--gpus"),
                        (["--mode", "video", "--infill", "0.3", "--infill_max_gap", "0"], "infill_max_gap"),
                        (["--mode", "video", "--infill", "nan"], "number")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work: no engine, no input folder needed
            demo.main(demo.parse_args(BASE + flags + ["--vid_file", str(tmp_path / "missing"), "--image_folder", str(tmp_path / "missing")]))
        assert word in str(e.value), (flags, e.value)
