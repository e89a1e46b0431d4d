"""GPU: ops.track_accel (poco_op_track_accel, csrc/track_accel.hip) against its plain-loop float64 restatement tests/accel_np.py.

Shapes: tracks of 1, 2 and 3 rows; one call with tracks of 1, 2, 70 and 300 rows (a track crosses the 64-row edges of a wave and of a
block's tile); a track with a hole in its frame ids; two adjacent tracks whose frame ids run on across the seam; M in {1, 14, 17,
32}; dense rows and rows of stride 416 (the evaluator's records) with NaN in every float the operator may not read; no ground truth.
Every output lies between poisoned guard rows.

Tolerances.  Per row the NaN pattern is the restatement's and the value is the restatement's float64 value
rounded to float32, within 1 ulp of float32: the device's float64 chain adds the joints in a tree where the restatement adds them in
order, which moves the float64 value by a few units of 2^-52 and can only flip the final rounding.  Sums: |device - fsum| <=
(n + M + 4) 2^-52 sum|terms| for n summed rows - n additions of the sum itself, and each term carries the M additions over the joints,
the stencil, the square root and the division of its own evaluation.  The sums are bitwise equal for max_blocks 1, 7 and the
default, and from run to run."""
import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import accel_np

pytestmark = pytest.mark.gpu
U = 2.0 ** -52
POISON = ops.POISON_BITS
REC, R_PRED, R_GT = 416, 116, 212                                          # the evaluator's record (include/poco_hip.h)


def _tracks(lengths, frames=None, seed=0):
    """A ragged buffer: smooth random motion plus jitter per track; frames default to 5, 6, 7, ... per track."""
    r = np.random.default_rng(seed)
    fr, off = [], [0]
    for k, T in enumerate(lengths):
        fr += list(frames[k]) if frames is not None and frames[k] is not None else list(range(5, 5 + T))
        off.append(off[-1] + T)
    return np.asarray(fr, np.int32), np.asarray(off, np.int32), r


def _joints(r, frames, M):
    t = frames[:, None, None].astype(np.float64)
    a, b, c = r.standard_normal((3, M, 3))
    pred = (a + 0.02 * b * t + 0.001 * c * t * t + 0.01 * r.standard_normal((len(frames), M, 3))).astype(np.float32)
    gt = (a + 0.02 * b * t + 0.0008 * c * t * t + 0.002 * r.standard_normal((len(frames), M, 3))).astype(np.float32)
    return pred, gt


CASES = {
    "short": dict(lengths=[1, 2, 3]),
    "long": dict(lengths=[1, 2, 70, 300]),
    "hole_and_seam": dict(lengths=[7, 4, 4, 3], frames=[[0, 1, 2, 4, 5, 6, 7], [10, 11, 12, 13], [14, 15, 16, 17], None]),
}


def _guarded(n, dtype, dev, cols=None):
    """A buffer of n rows between two guard rows, every word poisoned; -> (buffer, the view of the n rows)."""
    shape = (n + 2,) if cols is None else (n + 2, cols)
    words = 1 if dtype == torch.float32 else 2
    raw = torch.full((int(np.prod(shape)) * words,), POISON, dtype=torch.int32, device=dev)
    buf = raw.view(dtype).view(shape)
    return buf, buf[1:n + 1]


def _run(pred, gt, frames, offsets, layout, dev, max_blocks=0):
    N, M = pred.shape[:2]
    P = len(offsets) - 1
    if layout == "dense":
        dp, dg = torch.from_numpy(pred).to(dev), None if gt is None else torch.from_numpy(gt).to(dev)
    else:
        rec = np.full((N, REC), np.nan, np.float32)
        rec[:, R_PRED:R_PRED + 3 * M] = pred.reshape(N, -1)
        if gt is not None:
            rec[:, R_GT:R_GT + 3 * M] = gt.reshape(N, -1)
        drec = torch.from_numpy(rec).to(dev)
        dp, dg = drec[:, R_PRED:R_PRED + 3 * M], None if gt is None else drec[:, R_GT:R_GT + 3 * M]
    bufs = [_guarded(N, torch.float32, dev), _guarded(N, torch.float32, dev), _guarded(P, torch.float64, dev, 3),
            _guarded(1, torch.float64, dev, 3)]
    out = (bufs[0][1], None if gt is None else bufs[1][1], bufs[2][1], bufs[3][1].view(3))
    res = ops.track_accel(dp, dg, torch.from_numpy(frames).to(dev), torch.from_numpy(offsets), out=out, max_blocks=max_blocks)
    torch.cuda.synchronize()
    host = {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}
    host["raw"] = [b.view(-1).view(torch.int32).cpu().numpy().reshape(b.shape[0], -1) for b, _ in bufs]
    return host


def _check(got, want, N, M, P, with_gt, what):
    for k, (raw, n) in enumerate(zip(got["raw"], (N, N, P, 1))):
        assert (raw[0] == POISON).all() and (raw[-1] == POISON).all(), (what, "guard row", k)
        if k == 1 and not with_gt:
            assert (raw == POISON).all(), (what, "accel_err is not written without ground truth")
        else:
            assert not (raw[1:n + 1] == POISON).all(axis=1).any(), (what, "unwritten row", k)
    pairs = [("accel", "accel64")] + ([("accel_err", "accel_err64")] if with_gt else [])
    worst = 0
    for a, b in pairs:
        assert np.array_equal(np.isnan(got[a]), ~want["valid"]), (what, a)
        assert (got[a].view(np.uint32)[~want["valid"]] == 0x7fc00000).all(), (what, a, "quiet NaN")
        ulp = accel_np.ulp_distance(got[a], want[b])[want["valid"]]
        worst = max(worst, int(ulp.max(initial=0)))
    assert worst <= 1, (what, worst)
    lens = np.diff(want["offsets"])
    dev_t, dev_tot = 0.0, 0.0
    for c in range(3):
        tol = (lens + M + 4) * U * want["abs_track"][:, c]
        d = np.abs(got["track_sums"][:, c] - want["track_sums"][:, c])
        assert (d <= tol).all(), (what, "track_sums", c, d, tol)
        dev_t = max(dev_t, float((d / np.maximum(want["abs_track"][:, c], 1e-300)).max()))
        dt = abs(got["total"][c] - want["total"][c])
        assert dt <= (N + M + 4) * U * want["abs_total"][c], (what, "total", c, dt)
        dev_tot = max(dev_tot, dt / max(want["abs_total"][c], 1e-300))
    assert np.array_equal(got["track_sums"][:, 2], want["track_sums"][:, 2]) and got["total"][2] == want["total"][2]   # counts: exact
    if not with_gt:
        assert (got["track_sums"][:, 0] == 0).all() and got["total"][0] == 0
    print(f"track_accel {what}: rows within {worst} ulp, track sums within {dev_t / U:.2f} x 2^-52 (relative), total within "
          f"{dev_tot / U:.2f} x 2^-52, {int(want['total'][2])} of {N} rows valid")


_REF = {}


def _reference(case, M):
    """The inputs and the restatement of a case, computed once and shared (read only)."""
    if (case, M) not in _REF:
        spec = CASES[case]
        frames, offsets, r = _tracks(spec["lengths"], spec.get("frames"), seed=len(case) * 100 + M)
        pred, gt = _joints(r, frames, M)
        want = {g is not None: {**accel_np.track_accel(pred, g, frames, offsets), "offsets": offsets} for g in (gt, None)}
        _REF[(case, M)] = (pred, gt, frames, offsets, want)
    return _REF[(case, M)]


@pytest.mark.parametrize("layout", ["dense", "records"])
@pytest.mark.parametrize("M", [1, 14, 17, 32])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_and_sums_equal_the_restatement(case, M, layout, cuda):
    pred, gt, frames, offsets, want = _reference(case, M)
    N, P = len(frames), len(offsets) - 1
    got = _run(pred, gt, frames, offsets, layout, cuda)
    _check(got, want[True], N, M, P, True, f"{case} M={M} {layout}")


def test_the_valid_rows_are_the_ones_the_issue_names():
    _, _, _, _, want = _reference("short", 14)
    assert want[True]["valid"].tolist() == [False, False, False, False, True, False]            # the 3-row track: one valid row
    _, _, frames, offsets, want = _reference("hole_and_seam", 14)
    v = want[True]["valid"]
    assert frames[:7].tolist() == [0, 1, 2, 4, 5, 6, 7] and np.nonzero(v[:7])[0].tolist() == [1, 4, 5]   # frames 1, 5 and 6
    assert frames[10] + 1 == frames[11] and not v[10] and not v[11]                               # the seam: ids run on, rows invalid
    _, _, _, offsets, want = _reference("long", 14)
    assert np.diff(offsets).tolist() == [1, 2, 70, 300] and want[True]["valid"].sum() == 68 + 298


@pytest.mark.parametrize("layout", ["dense", "records"])
def test_without_ground_truth_only_accel_is_written(layout, cuda):
    pred, _, frames, offsets, want = _reference("long", 17)
    got = _run(pred, None, frames, offsets, layout, cuda)
    assert got["accel_err"] is None
    _check(got, want[False], len(frames), 17, len(offsets) - 1, False, f"long M=17 {layout}, no ground truth")


def test_bits_do_not_depend_on_the_grid_or_the_run(cuda):
    pred, gt, frames, offsets, _ = _reference("long", 14)
    runs = [_run(pred, gt, frames, offsets, "records", cuda, max_blocks=mb) for mb in (0, 1, 7, 0)]
    for other in runs[1:]:
        for k in ("track_sums", "total"):
            assert np.array_equal(runs[0][k].view(np.uint64), other[k].view(np.uint64)), k
        for k in ("accel", "accel_err"):
            assert np.array_equal(runs[0][k].view(np.uint32), other[k].view(np.uint32)), k
    dense = _run(pred, gt, frames, offsets, "dense", cuda)
    for k in ("track_sums", "total"):
        assert np.array_equal(runs[0][k].view(np.uint64), dense[k].view(np.uint64)), k        # the row stride never reaches the arithmetic


def test_a_track_gives_the_same_bits_alone_and_among_others(cuda):
    """The summation tree is a function of the track's own length: the 70-row track scored alone equals its rows in the long call."""
    pred, gt, frames, offsets, _ = _reference("long", 14)
    whole = _run(pred, gt, frames, offsets, "dense", cuda)
    lo, hi = int(offsets[2]), int(offsets[3])
    alone = _run(pred[lo:hi], gt[lo:hi], frames[lo:hi], np.array([0, hi - lo], np.int32), "dense", cuda)
    assert np.array_equal(alone["track_sums"][0].view(np.uint64), whole["track_sums"][2].view(np.uint64))
    assert np.array_equal(alone["accel_err"].view(np.uint32), whole["accel_err"][lo:hi].view(np.uint32))
    assert np.array_equal(alone["total"].view(np.uint64), alone["track_sums"][0].view(np.uint64))
