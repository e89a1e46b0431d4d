"""GPU: poco_op_rotmat_to_aa and the pseudo-labeler's step (csrc/pseudo_gt.hip) against the reference-made fixture
tests/golden/pseudo.npz and the numpy restatement tests/pseudo_np.py.  Synthetic tensors: no engine is built.

Tolerance: a device axis-angle is compared within 8 x the fixture's d_ref_aa (the evaluator's rule, DESIGN.md section 10: the
device computes in fp64 from the same float32 inputs, so its distance to the reference is the reference's own rounding).  `var` is
compared bitwise for [B,24] input and within 1 ulp with a trailing axis; everything else - flags, counts, order, center, scale,
keypoints, source_id, padding, unwritten memory - bit for bit."""
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import ops, pseudo
from poco_amd._lib import PocoHipError
from tests import pseudo_np

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "pseudo.npz"
NONE_THR = 1e-6                # below every var of step_inputs (>= 0.05): keeps nothing


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("N", [1, 24, 255, 256, 257, 0])
def test_rotmat_to_aa_op(cuda, gold, N):
    """The last N fixture matrices (the special rows sit at the end; N = 0: all of them)."""
    R, cls, ref = gold["rotmat"][-N:], gold["cls"][-N:], gold["aa"][-N:]
    out = ops.rotmat_to_aa(torch.from_numpy(R.copy()).to(cuda)).cpu().numpy()
    d = np.abs(out.astype(np.float64) - ref).max()
    y64 = pseudo_np.rotmat_to_aa(R, np.float64)
    print(f"N={len(R)}: vs reference {d:.3e} (tolerance {8 * gold['d_ref_aa']:.3e}), vs float64 restatement "
          f"{np.abs(out.astype(np.float64) - y64).max():.3e}")
    assert out.shape == (len(R), 3) and d <= 8 * gold["d_ref_aa"]
    special = np.isin(cls, [pseudo_np.CLASSES.index(c) for c in pseudo_np.SPECIAL])
    assert np.array_equal(out[special], y64[special])               # NaN, zero, identity, pi: exactly the restatement's values
    if N == 0:
        assert special.sum() >= 22 and np.array_equal(out[cls == pseudo_np.CLASSES.index("nan")], np.zeros((1, 3), np.float32))
        assert np.array_equal(out[cls == pseudo_np.CLASSES.index("zero")], np.array([[0, np.pi, 0]], np.float32))
        # [..., 3, 3] in, [..., 3] out
        assert ops.rotmat_to_aa(torch.from_numpy(R[:48].copy()).to(cuda).view(2, 24, 3, 3)).shape == (2, 24, 3)


def _pred(x, cuda):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)          # noqa: E731
    return {"pred_pose": t(x["pred_pose"]), "pred_shape": t(x["pred_shape"]), "var_pose": t(x["var_pose"]),
            "smpl_joints2d": t(x["joints2d"]), "smpl_joints3d": t(x["joints3d"])}


def _offer(pl, x, cuda):
    pl.step(_pred(x, cuda), torch.from_numpy(x["boxes"]).to(cuda), x["source_id"])


def _check_records(res, want, gold, T, what):
    """res = PseudoLabeler.finish(return_records=True); want = the restatement's records of the kept crops (float64 arithmetic)."""
    rec, n = res["records"], len(want)
    assert res["kept"] == n, (what, res["kept"], n)
    got = rec[:n]
    exact = np.ones(pseudo_np.RECORD_FLOATS, bool)
    exact[pseudo_np.P_POSE:pseudo_np.P_SHAPE] = False
    exact[pseudo_np.P_VAR:pseudo_np.P_OPENPOSE] = False
    assert np.array_equal(bits(got[:, exact]), bits(want[:, exact])), what
    gv, wv = got[:, pseudo_np.P_VAR:pseudo_np.P_OPENPOSE], want[:, pseudo_np.P_VAR:pseudo_np.P_OPENPOSE]
    if T == 1:
        assert np.array_equal(bits(gv), bits(wv)), what
    else:
        ulps = np.abs(bits(gv).astype(np.int64) - bits(wv).astype(np.int64)).max() if n else 0
        print(f"{what}: var within {ulps} ulp")
        assert ulps <= 1, what
    if n:
        d = np.abs(got[:, pseudo_np.P_POSE:pseudo_np.P_SHAPE].astype(np.float64) - want[:, pseudo_np.P_POSE:pseudo_np.P_SHAPE]).max()
        print(f"{what}: pose vs float64 restatement {d:.3e} (tolerance {8 * gold['d_ref_aa']:.3e})")
        assert d <= 8 * gold["d_ref_aa"], what
    assert np.all(bits(rec[n:]) == pseudo_np.UNWRITTEN), what       # memory past the kept records still holds the fill pattern


@pytest.mark.parametrize("mode", ["all", "none", "median"])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 256, 257, 300])
def test_step(cuda, gold, B, mode):
    """One step: the wave edge (63, 64, 65), the block edge (256, 257) and the loop (300).  T = 9 trailing elements at B = 2, 65
    and 300, the PARE keypoint conversion at odd B.  The median threshold is computed here, on the host, from the inputs; at B = 1
    the median is the only value, `<` keeps nothing, and no share can be asserted."""
    T, in_crop = (9 if B in (2, 65, 300) else 1), bool(B % 2)
    x = pseudo_np.step_inputs(B, T, seed=B)
    thr = {"all": None, "none": NONE_THR, "median": float(np.median(pseudo_np.trailing_mean(x["var_pose"])[:, 0]))}[mode]
    want, keep = pseudo_np.step(**x, threshold=thr, joints_in_crop=in_crop)
    if mode == "median" and B >= 2:
        assert 0.4 <= keep.mean() <= 0.6, keep.mean()               # on the numpy side first: dropping everything cannot pass
    if mode == "none":
        assert not keep.any()
    pl = pseudo.PseudoLabeler(B, thr, "hrnet_w32-pare" if in_crop else "hrnet_w48_cls-cliff", device=cuda)
    _offer(pl, x, cuda)
    res = pl.finish(return_records=True)
    assert res["offered"] == B and res["records"].shape == (B, pseudo_np.RECORD_FLOATS)
    _check_records(res, want, gold, T, f"B={B} {mode}")
    assert np.array_equal(res["source_id"], x["source_id"][keep])                                 # stable: source order
    if mode == "none":
        assert res["kept"] == 0 and np.all(bits(res["records"]) == pseudo_np.UNWRITTEN)           # untouched record memory
    if mode == "all":
        assert res["kept"] == B and all(v.shape[0] == B for k, v in res.items() if isinstance(v, np.ndarray) and k != "records")
    pl.close()


def test_steps_append_capacity_reset_and_errors(cuda, gold):
    """Three steps of different B == one restatement call on the concatenation, and == one device step on it, bit for bit; a step
    past the capacity and a step with a bad argument are refused and leave records and counts as they were; reset rewinds."""
    import ctypes as C
    parts = [pseudo_np.step_inputs(b, 1, seed=100 + b) for b in (70, 1, 300)]
    cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    n = len(cat["source_id"])
    thr = float(np.median(cat["var_pose"][:, 0]))
    want, keep = pseudo_np.step(**cat, threshold=thr)
    assert 0.4 <= keep.mean() <= 0.6
    pl = pseudo.PseudoLabeler(n + 5, thr, "hrnet_w48_cls-cliff", device=cuda)
    for p in parts:
        _offer(pl, p, cuda)
    res = pl.finish(return_records=True)
    assert res["offered"] == n and res["records"].shape[0] == n
    _check_records(res, want, gold, 1, "three steps")
    one = pseudo.PseudoLabeler(n, thr, "hrnet_w48_cls-cliff", device=cuda)
    _offer(one, cat, cuda)
    assert np.array_equal(bits(one.finish(return_records=True)["records"]), bits(res["records"]))
    one.close()
    # refused: 6 more crops exceed the capacity; null pointer; B < 1
    with pytest.raises(PocoHipError, match="capacity"):
        _offer(pl, pseudo_np.step_inputs(6, 1, seed=1), cuda)
    L, fake = pseudo._bind(), C.c_void_p(4096)
    assert L.poco_pseudo_step(pl._h, 2, None, fake, fake, 1, fake, fake, fake, fake, None) == 1
    assert L.poco_pseudo_step(pl._h, 0, fake, fake, fake, 1, fake, fake, fake, fake, None) == 1
    again = pl.finish(return_records=True)
    assert (again["offered"], again["kept"]) == (n, res["kept"]) and np.array_equal(bits(again["records"]), bits(res["records"]))
    # 5 crops still fit
    tail = pseudo_np.step_inputs(5, 1, seed=2)
    _offer(pl, tail, cuda)
    more = pl.finish(return_records=True)
    w5, k5 = pseudo_np.step(**tail, threshold=thr)
    assert more["offered"] == n + 5 and more["kept"] == res["kept"] + int(k5.sum())
    assert np.array_equal(bits(more["records"][:res["kept"]]), bits(res["records"][:res["kept"]]))
    # reset: counts 0, the records unwritten again, the next step starts at record 0
    pl.reset()
    empty = pl.finish(return_records=True)
    assert (empty["offered"], empty["kept"]) == (0, 0) and empty["pose"].shape == (0, 72)
    _offer(pl, parts[0], cuda)
    res0 = pl.finish(return_records=True)
    w0, _ = pseudo_np.step(**parts[0], threshold=thr)
    _check_records(res0, w0, gold, 1, "after reset")
    pl.close()


def test_imgname_and_person_id_follow_source_id(cuda):
    x = pseudo_np.step_inputs(9, 1, seed=7)
    x["source_id"] = np.arange(9, dtype=np.int32)[::-1].copy()
    thr = float(np.median(x["var_pose"][:, 0]))
    _, keep = pseudo_np.step(**x, threshold=thr)
    pl = pseudo.PseudoLabeler(9, thr, "resnet50-cliff", device=cuda)
    _offer(pl, x, cuda)
    names, ids = [f"f{i}.png" for i in range(9)], list(range(100, 109))
    res = pl.finish(imgname=names, person_id=ids)
    sid = x["source_id"][keep]
    assert list(res["imgname"]) == [names[i] for i in sid] and list(res["person_id"]) == [ids[i] for i in sid]
    assert res["person_id"].dtype == np.int32 and np.all(res["has_smpl"] == 1)
    pl.close()
